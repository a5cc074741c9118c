"""
Frame-level pitch annotations next to the hot path: what ``PitchDataset.__getitem__`` (reference
``timbre_trap/datasets/PitchDataset.py:164-192``) does per item of an ``MPEDataset`` -- ``resample_multi_pitch`` (``:194-231``), then
``multi_pitch_to_activations`` (``:233-307``), then the ``.float()`` of ``train.py:394`` -- and the reference lists of ``evaluate()`` on
such a dataset (``experiments/evaluate.py:76-78,116``).

``PitchBank`` keeps the annotations of a whole dataset on the device, uploaded once: per value the nearest bin and the scorer's MIDI
number, per source frame the row offsets and the 'lost' byte, per track the frame times -- all formed on the host, vectorised over every
value, with the very expressions of the list-based code (``utils/targets.py``, ``utils/metrics/multipitch.py``), so equality with that code holds
by construction.  What scales with the items runs in HIP kernels (csrc/pitch.hip):

  tt_pitch_nearest   (item, frame) -> the source frame it reads, ``nearest_indices``' float64 comparisons by binary search
  tt_pitch_targets   the blurred, renormalised, clipped (B, F, T) targets of a batch, float64 or float32, and one warning flag per item

``resample_multi_pitch`` + ``multi_pitch_to_activations`` stay the yardstick the device route is tested against, and the route a track
with unsorted or non-finite times, more bins or a wider blur than the kernels hold takes.
"""

import warnings

import numpy as np
import torch

from .. import _hip
from .metrics.multipitch import MAX_FREQ, MIN_FREQ, frequencies_to_midi
from .notes import _cuda_device, _is_sorted, _note_bins
from .slicing import resample_multi_pitch
from .targets import _gaussian_weights, multi_pitch_to_activations

__all__ = ['PitchBank', 'pitch_to_activations', 'pitch_tiles']

_WARNING = 'Could not fully represent ground-truth with available frequency bins.'


def pitch_tiles():
    """(frames per workgroup, most bins, widest blur radius) of the target kernels (tt_pitch_tile_frames(), tt_pitch_max_bins(),
    tt_pitch_max_radius()): the size the tests straddle and the capacities beyond which ``PitchBank.targets`` takes the list route."""
    lib = _hip.lib()
    return lib.tt_pitch_tile_frames(), lib.tt_pitch_max_bins(), lib.tt_pitch_max_radius()


def _bank_arrays(tracks, midi_freqs, resample_idcs):
    """
    The host arena of ``PitchBank`` (no device work): a dict of
      times float64 [R], table int64 [n, 4] = (base, K, below, above), row_off int64 [R + 1], hz float64 [V], bins int32 [V] (-1: a zero
      or out-of-range pitch), lost uint8 [R], midi float64 [V] (the scorer's numbers), outside bool [n] (``_mpe_reference_csr``'s range
      check per track), device_ok bool [n] (times non-decreasing and finite).
    """
    times, frames, table = [], [], np.zeros((len(tracks), 4), dtype=np.int64)
    device_ok = np.zeros(len(tracks), dtype=bool)
    base = 0
    for n, (t, mp) in enumerate(tracks):
        t = np.asarray(t, dtype=np.float64).ravel()
        K = len(t)
        if K != len(mp):
            raise ValueError('track %d: %d times for %d frames of pitches' % (n, K, len(mp)))
        if K == 0:
            raise ValueError('track %d holds no frame' % n)
        original = np.arange(K)
        table[n] = (base, K, original[resample_idcs[0]], original[resample_idcs[-1]])
        device_ok[n] = _is_sorted(t) and bool(np.isfinite(t).all())
        times.append(t)
        frames.extend(np.asarray(p, dtype=np.float64).ravel() for p in mp)       # lists to arrays: the one loop over the frames
        base += K
    row_off = np.zeros(base + 1, dtype=np.int64)
    np.cumsum(np.array([f.size for f in frames], dtype=np.int64), out=row_off[1:])
    hz = np.concatenate(frames) if row_off[-1] else np.empty(0)
    with np.errstate(divide='ignore', invalid='ignore'):                          # a list may hold anything; both routes drop it alike
        bins, lost_value = _note_bins(hz, midi_freqs)
        midi = frequencies_to_midi([hz])[0]
    lost_before = np.concatenate([[0], np.cumsum(lost_value, dtype=np.int64)])
    lost = (lost_before[row_off[1:]] > lost_before[row_off[:-1]]).astype(np.uint8)
    outside = np.zeros(len(tracks), dtype=bool)
    for n, (b, K) in enumerate(table[:, :2]):
        flat = hz[row_off[b]:row_off[b + K]]
        outside[n] = bool(flat.size and (flat.max() > MAX_FREQ or flat.min() < MIN_FREQ))
    return dict(times=np.concatenate(times) if times else np.empty(0), table=table, row_off=row_off, hz=hz, bins=bins, lost=lost, midi=midi,
                outside=outside, device_ok=device_ok)


class PitchBank:
    """
    The pitch annotations of a dataset, resident on the device.  ``tracks``: a sequence of ``(times, multi_pitch)`` as
    ``get_ground_truth`` returns them -- frame times (K) and a list of K arrays of pitches in Hz; ``midi_freqs``: the MIDI number of
    every bin (F); ``resample_idcs``: the reference's attribute of the same name (default ``[0, -1]``).  One arena is uploaded here,
    once; ``targets`` then forms the targets of any batch of items, and ``MultipitchEvaluator.evaluate_track`` reads the same arena as
    the scorer's reference.  The bank belongs in the process that drives the device (DataLoader workers hold no GPU context).
    A non-CUDA ``device`` raises ``RuntimeError``: there is no CPU fallback.
    """

    def __init__(self, tracks, midi_freqs, resample_idcs=None, device='cuda'):
        self.device = _cuda_device(device)
        self.midi_freqs = np.array(midi_freqs, dtype=np.float64).ravel()
        self.resample_idcs = [0, -1] if resample_idcs is None else list(resample_idcs)
        self.tracks = [(t, mp) for t, mp in tracks]                               # the lists themselves: the list route reads them
        self.host = _bank_arrays(self.tracks, self.midi_freqs, self.resample_idcs)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)  # noqa: E731
        h = self.host
        self.times_d, self.table_d, self.row_off_d = up(h['times']), up(h['table'].ravel()), up(h['row_off'])
        self.bins_d, self.lost_d, self.midi_d = up(h['bins']), up(h['lost']), up(h['midi'])
        self.device = self.times_d.device                                         # with its index, to compare with a tensor's
        self.last_lost = np.zeros(0, dtype=bool)

    def __len__(self):
        return len(self.tracks)

    def track_times(self, track_id):
        base, K = self.host['table'][track_id, :2]
        return self.host['times'][base:base + K]

    def reference_csr(self, track_id):
        """(row offsets int64 [K + 1] into the arena, the arena's float64 MIDI numbers): views of device memory, the reference that
        ``tt_mpe_match`` reads for this track."""
        base, K = self.host['table'][track_id, :2]
        return self.row_off_d[base:base + K + 1], self.midi_d

    def _on_device(self, ids, radius):
        _, max_bins, max_radius = pitch_tiles()
        return (1 <= len(self.midi_freqs) <= max_bins and radius <= max_radius and len(ids) <= 65535 and
                bool(self.host['device_ok'][ids].all()))

    def _list_route(self, ids, times, blur, dtype):
        outs, lost = [], np.zeros(len(ids), dtype=bool)
        for b, n in enumerate(ids):
            _times, _mp = self.tracks[n]
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter('always')
                lists = resample_multi_pitch(_times, _mp, times[b], self.resample_idcs)
                outs.append(multi_pitch_to_activations(lists, self.midi_freqs, blur, self.device, return_tensor=True).to(dtype))
            for w in caught:
                if issubclass(w.category, RuntimeWarning) and str(w.message) == _WARNING:
                    lost[b] = True
                else:
                    warnings.warn_explicit(w.message, w.category, w.filename, w.lineno)
        return torch.stack(outs), lost

    def targets(self, track_ids, times, n_bins_blur_decay=2.5, dtype=torch.float32, return_tensor=True):
        """
        ``multi_pitch_to_activations(resample_multi_pitch(*tracks[track_ids[b]], times[b]), midi_freqs, n_bins_blur_decay)`` of every
        item b, stacked: (B, F, T) in ``dtype`` -- ``torch.float64`` bit for bit, ``torch.float32`` its ``.float()`` -- on the device
        (``return_tensor=False``: an ndarray).  ``times``: (B, T) float64 with ``track_ids`` (B), or (T) with one track id for one
        (F, T) map.  Two small uploads (ids, times), four launches whatever B is, one small copy back: the per-item warning flags,
        kept in ``last_lost``; the reference's ``RuntimeWarning`` is emitted once if any is set.
        """
        if dtype not in (torch.float32, torch.float64):
            raise ValueError('dtype must be torch.float32 or torch.float64 (got %s)' % dtype)
        times = np.asarray(times, dtype=np.float64)
        single = times.ndim == 1
        ids = np.atleast_1d(np.asarray(track_ids)).astype(np.int64)
        times = times[None] if single else times
        if times.ndim != 2 or ids.shape != (len(times),):
            raise ValueError('times must be (B, T) with B track ids, or (T) with one (got %s and %s)' % (times.shape, ids.shape))
        if ids.size and (ids.min() < 0 or ids.max() >= len(self.tracks)):
            raise IndexError('track id outside [0, %d)' % len(self.tracks))
        B, T = times.shape
        F = len(self.midi_freqs)
        radius, w = 0, None
        if n_bins_blur_decay:
            w, radius = _gaussian_weights((2 * n_bins_blur_decay) / 5)
        if B * T * F == 0:
            out, lost = torch.zeros((B, F, T), dtype=dtype, device=self.device), np.zeros(B, dtype=bool)
        elif not self._on_device(ids, radius):
            out, lost = self._list_route(ids, times, n_bins_blur_decay, dtype)
        else:
            lib, dev = _hip.lib(), self.device
            ids_d = torch.from_numpy(ids.astype(np.int32)).to(dev)
            times_d = torch.from_numpy(np.array(times, order='C')).to(dev)         # a copy: the caller's array may be read-only
            w_d = torch.from_numpy(w).to(dev) if radius else None
            idx = torch.empty((B, T), dtype=torch.int32, device=dev)
            out = torch.empty((B, F, T), dtype=dtype, device=dev)
            flags = torch.empty(B, dtype=torch.int32, device=dev)
            scratch = torch.empty(lib.tt_pitch_scratch_bytes(B, T) // 8 + 1, dtype=torch.float64, device=dev)
            with torch.cuda.device(dev):
                st = _hip.stream_ptr()
                _hip.check(lib.tt_pitch_nearest(_hip.ptr(self.times_d), _hip.ptr(self.table_d), len(self.tracks), _hip.ptr(ids_d),
                                                _hip.ptr(times_d), B, T, _hip.ptr(idx), st), 'tt_pitch_nearest')
                _hip.check(lib.tt_pitch_targets(_hip.ptr(idx), _hip.ptr(self.table_d), len(self.tracks), _hip.ptr(ids_d), B, T,
                                                _hip.ptr(self.row_off_d), _hip.ptr(self.bins_d), _hip.ptr(self.lost_d), _hip.ptr(w_d), radius,
                                                F, int(dtype == torch.float32), _hip.ptr(scratch), _hip.ptr(out), _hip.ptr(flags), st),
                           'tt_pitch_targets')
            lost = flags.cpu().numpy().astype(bool)                                # the one copy that comes back
        self.last_lost = lost
        if lost.any():
            warnings.warn(_WARNING, RuntimeWarning)
        out = out[0] if single else out
        return out if return_tensor else out.cpu().numpy()


def pitch_to_activations(_times, _multi_pitch, times, midi_freqs, resample_idcs=(0, -1), n_bins_blur_decay=2.5, device='cuda',
                         return_tensor=False):
    """
    ``multi_pitch_to_activations(resample_multi_pitch(_times, _multi_pitch, times, resample_idcs), midi_freqs, n_bins_blur_decay)`` bit
    for bit -- the (F, T) float64 targets of a ``PitchDataset`` item (``PitchDataset.py:182-185``) -- through a ``PitchBank`` of this one
    track.  ndarray out like the reference; ``return_tensor=True``: the float64 device tensor.  Build a ``PitchBank`` once instead when
    more than one item is cut from a track: this function pays the flattening of the whole track every time.
    """
    bank = PitchBank([(_times, _multi_pitch)], midi_freqs, resample_idcs, device)
    return bank.targets(0, np.asarray(times, dtype=np.float64).ravel(), n_bins_blur_decay, torch.float64, return_tensor)
