"""
Note annotations next to the hot path: ``NoteDataset.notes_to_multi_pitch`` (reference ``timbre_trap/datasets/NoteDataset.py:93-123``)
and what its two callers do with the result -- ``multi_pitch_to_activations`` per training / validation item (``NoteDataset.py:81-84``)
and the reference lists of ``evaluate()`` (``experiments/evaluate.py:67-75``).

The reference loops over the L notes, masks all N frames per note and appends one value per (note, frame) pair.  Here the L-sized
scalars stay on the host (nearest bin, range tests, MIDI numbers: the very expressions of ``utils/targets.py`` over L values) and
everything that scales with the frames runs in HIP kernels (csrc/notes.hip, csrc/losses.hip):

  tt_note_spans                 note -> half-open frame range, the reference's float64 comparisons by binary search
  tt_note_count / tt_note_fill  frame -> the notes that hold it, in ascending note order (CSR), for the device scorer
  tt_target_activations_spans   (bin, frame range) per note -> the blurred, renormalised, clipped target map

``notes_to_multi_pitch`` is the vectorised host function with the reference's result, element for element; it is the yardstick the
device routes are tested against and the route ``times`` that are not sorted take.
"""

import warnings

import numpy as np
import torch

from .. import _hip
from .targets import _gaussian_weights, hz_to_midi, multi_pitch_to_activations

__all__ = ['notes_to_multi_pitch', 'notes_csr_device', 'notes_to_activations', 'note_tiles']


def _note_arrays(pitches, intervals, times):
    pitches = np.asarray(pitches, dtype=np.float64).ravel()
    intervals = np.ascontiguousarray(np.asarray(intervals, dtype=np.float64).reshape(-1, 2))
    times = np.ascontiguousarray(np.asarray(times, dtype=np.float64).ravel())
    if len(pitches) != len(intervals):
        raise ValueError('pitches (%d) and intervals (%d) must hold one entry per note' % (len(pitches), len(intervals)))
    return pitches, intervals, times


def _is_sorted(times):
    return bool(np.all(times[1:] >= times[:-1]))                  # a NaN time fails this and takes the mask route


def _host_spans(intervals, times):
    """(lo, hi) int64 per note for non-decreasing ``times``: frames lo <= t < hi are those with times >= onset and times < offset."""
    on, off = intervals[:, 0], intervals[:, 1]
    ok = ~(np.isnan(on) | np.isnan(off))
    lo = np.where(ok, np.searchsorted(times, np.where(ok, on, 0.0), side='left'), 0)
    hi = np.where(ok, np.searchsorted(times, np.where(ok, off, 0.0), side='left'), 0)
    return lo.astype(np.int64), hi.astype(np.int64)


def _host_pairs(intervals, times):
    """Every (frame, note) pair with the note sounding in the frame, frame-major and in note order within a frame:
    (off int64 [N + 1], note_idx int64)."""
    N, L = len(times), len(intervals)
    if _is_sorted(times):
        lo, hi = _host_spans(intervals, times)
        cnt = np.maximum(hi - lo, 0)
        note = np.repeat(np.arange(L, dtype=np.int64), cnt)
        start = np.cumsum(cnt) - cnt
        frame = lo[note] + (np.arange(int(cnt.sum()), dtype=np.int64) - start[note])
    else:
        # the reference's mask, note by note
        hits = [np.flatnonzero((times >= j) & (times < k)) for j, k in intervals]
        frame = np.concatenate(hits).astype(np.int64) if L else np.empty(0, dtype=np.int64)
        note = np.repeat(np.arange(L, dtype=np.int64), [len(h) for h in hits]) if L else np.empty(0, dtype=np.int64)
    order = np.argsort(frame, kind='stable')                      # note-major in, stable: ascending note index within a frame
    off = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(frame, minlength=N), out=off[1:])
    return off, note[order]


def notes_to_multi_pitch(pitches, intervals, times):
    """
    Notes (``pitches`` (L), ``intervals`` (L, 2) onset / offset in seconds) -> list of N float64 arrays: the pitches sounding at every
    entry of ``times``, i.e. of the notes with ``times >= onset`` and ``times < offset``, in note order -- the result of the reference's
    ``NoteDataset.notes_to_multi_pitch`` element for element (host arrays, no device work).  Sorted ``times`` cost two binary searches
    per note and one stable sort of the pairs; unsorted ``times`` fall back to one mask over the frames per note.
    """
    pitches, intervals, times = _note_arrays(pitches, intervals, times)
    off, note = _host_pairs(intervals, times)
    values = pitches[note]
    empty = np.empty(0)
    multi_pitch = np.split(values, off[1:-1]) if len(times) else []
    return [f if f.size else empty for f in multi_pitch]


def note_tiles():
    """(frames per workgroup, notes per pass) of the CSR kernels (tt_note_tile_frames(), tt_note_chunk()): the sizes the tests straddle."""
    lib = _hip.lib()
    return lib.tt_note_tile_frames(), lib.tt_note_chunk()


def _cuda_device(device):
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError('timbre_trap HIP path needs a GPU device (got %s); there is no CPU fallback' % dev)
    return dev


def _device_spans(intervals, times, dev):
    """tt_note_spans: (lo, hi) int32 device tensors for non-decreasing ``times``."""
    L, N = len(intervals), len(times)
    lo = torch.zeros(L, dtype=torch.int32, device=dev)
    hi = torch.zeros(L, dtype=torch.int32, device=dev)
    if L and N:
        t_d, iv_d = torch.from_numpy(np.array(times)).to(dev), torch.from_numpy(np.array(intervals)).to(dev)      # copies: the inputs may be read-only
        with torch.cuda.device(dev):
            _hip.check(_hip.lib().tt_note_spans(_hip.ptr(t_d), N, _hip.ptr(iv_d), L, _hip.ptr(lo), _hip.ptr(hi), _hip.stream_ptr()),
                       'tt_note_spans')
    return lo, hi


def _device_csr(lo, hi, N, extra=()):
    """
    tt_note_count -> prefix sum -> tt_note_fill on span tensors: ``(off int64 [N + 1], note_idx int32, extra values)``.  The lists hold
    up to L N entries, far more than they ever do, so their total comes back to size ``note_idx`` -- one small copy, which also carries
    the 0-dim device tensors of ``extra`` (flags the caller wants anyway) as Python ints.
    """
    dev, L = lo.device, lo.numel()
    off = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    if N == 0 or L == 0:
        back = torch.stack([e.to(torch.int64) for e in extra]).cpu().tolist() if extra else []
        return off, torch.empty(0, dtype=torch.int32, device=dev), back
    lib = _hip.lib()
    count = torch.empty(N, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = _hip.stream_ptr()
        _hip.check(lib.tt_note_count(_hip.ptr(lo), _hip.ptr(hi), L, N, _hip.ptr(count), st), 'tt_note_count')
        off[1:] = torch.cumsum(count, 0, dtype=torch.int64)
        back = torch.stack([off[-1]] + [e.to(torch.int64) for e in extra]).cpu().tolist()
        total = int(back[0])
        note_idx = torch.empty(total, dtype=torch.int32, device=dev)
        if total:
            _hip.check(lib.tt_note_fill(_hip.ptr(lo), _hip.ptr(hi), L, N, _hip.ptr(off), total, _hip.ptr(note_idx), st), 'tt_note_fill')
    return off, note_idx, back[1:]


def notes_csr_device(pitches, intervals, times, device='cuda'):
    """
    ``notes_to_multi_pitch`` as a CSR of note indices on the device: ``(off int64 [N + 1], note_idx int32)`` with the notes of frame
    ``t``, in ascending note order, at ``note_idx[off[t]:off[t + 1]]`` -- ``pitches[note_idx[...]]`` are the reference's lists.
    Sorted ``times``: tt_note_spans, tt_note_count, a prefix sum, tt_note_fill.  Unsorted ``times``: the host pairs, uploaded.
    """
    pitches, intervals, times = _note_arrays(pitches, intervals, times)
    dev = _cuda_device(device)
    if not _is_sorted(times):
        off, note = _host_pairs(intervals, times)
        return torch.from_numpy(off).to(dev), torch.from_numpy(note.astype(np.int32)).to(dev)
    lo, hi = _device_spans(intervals, times, dev)
    off, note_idx, _ = _device_csr(lo, hi, len(times))
    return off, note_idx


def _note_bins(pitches, midi_freqs):
    """Per note, with the expressions of ``multi_pitch_to_activations``: the nearest bin (-1: a zero or out-of-range pitch, dropped)
    and whether the note is non-zero and out of range (the notes the 'Could not fully represent' warning is about)."""
    lb, ub = np.min(midi_freqs), np.max(midi_freqs)
    mids = (midi_freqs[1:] + midi_freqs[:-1]) / 2.0
    nonzero = np.flatnonzero(pitches != 0)
    m = hz_to_midi(pitches[nonzero])
    inside = np.logical_and(m >= lb, m <= ub)
    bins = np.full(len(pitches), -1, dtype=np.int32)
    bins[nonzero[inside]] = np.searchsorted(mids, m[inside], side='left')
    lost = np.zeros(len(pitches), dtype=bool)
    lost[nonzero[~inside]] = True
    return bins, lost


def notes_to_activations(pitches_hz, intervals, times, midi_freqs, n_bins_blur_decay=2.5, device='cuda', return_tensor=False):
    """
    ``multi_pitch_to_activations(notes_to_multi_pitch(pitches_hz, intervals, times), midi_freqs, n_bins_blur_decay)`` bit for bit --
    the (F, T) float64 targets of a ``NoteDataset`` item -- without the per-frame lists: per note the nearest bin on the host, the
    frame range (tt_note_spans) and the map (tt_target_activations_spans) on the device.  Emits the same ``RuntimeWarning`` when a
    non-zero pitch outside the bin range sounds in at least one frame (one flag comes back for it).  ndarray out like the reference;
    ``return_tensor=True``: the float64 device tensor, no download.  A non-CUDA ``device`` raises ``RuntimeError``; ``times`` that are
    not sorted go through the host lists and ``multi_pitch_to_activations``.
    """
    pitches, intervals, times = _note_arrays(pitches_hz, intervals, times)
    midi_freqs = np.asarray(midi_freqs, dtype=np.float64)
    dev = _cuda_device(device)
    if not _is_sorted(times):
        return multi_pitch_to_activations(notes_to_multi_pitch(pitches, intervals, times), midi_freqs, n_bins_blur_decay, dev, return_tensor)
    F, T, L = len(midi_freqs), len(times), len(pitches)
    bins, lost = _note_bins(pitches, midi_freqs)
    out = torch.empty((F, T), dtype=torch.float64, device=dev)
    if F * T == 0:
        return out if return_tensor else out.cpu().numpy()
    radius, w_t, work = 0, None, None
    if (bins >= 0).any() and n_bins_blur_decay:
        w, radius = _gaussian_weights((2 * n_bins_blur_decay) / 5)
        w_t = torch.from_numpy(w).to(dev)
        work = torch.empty((F, T), dtype=torch.float64, device=dev)
    lo, hi = _device_spans(intervals, times, dev)
    b_t = torch.from_numpy(bins).to(dev) if L else None
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().tt_target_activations_spans(_hip.ptr(b_t), _hip.ptr(lo) if L else None, _hip.ptr(hi) if L else None, L,
                                                          _hip.ptr(w_t), radius, F, T, _hip.ptr(work), _hip.ptr(out), _hip.stream_ptr()),
                   'tt_target_activations_spans')
    if lost.any() and bool(((hi > lo) & torch.from_numpy(lost).to(dev)).any()):            # the one flag that comes back
        warnings.warn('Could not fully represent ground-truth with available frequency bins.', RuntimeWarning)
    return out if return_tensor else out.cpu().numpy()
