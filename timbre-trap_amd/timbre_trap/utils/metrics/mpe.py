"""
The front of csrc/mpe.hip: the scores of ``multipitch.multipitch_metrics``, bit for bit, from activations that stay on the device
(reference ``experiments/evaluate.py:100-116``).  Compaction of the activation map to per-frame bin lists, a maximum matching per
reference frame in float64, integer sums; one small copy back per track; the float64 arithmetic on the sums is the host module's.  The
reference comes as frame lists, as notes (CSR built by csrc/notes.hip) or from a ``utils.pitch.PitchBank``.
"""

import numpy as np
import torch

from ... import _hip
from .. import notes as _notes
from ..targets import midi_to_hz
from .multipitch import MAX_FREQ, MIN_FREQ, _MPE_SUMS, _max_matching, _mpe_sums, _nearest_frame_index, _scores_from_sums, frequencies_to_midi

MPE_MAX_EST = 256         # active bins per frame the matching kernel holds (= tt_mpe_max_est(), checked on first use)
MPE_MAX_REF = 64          # reference pitches per frame it holds (= tt_mpe_max_ref())


def _mpe_range_error(what):
    return ValueError('%s frequencies must lie in [%g, %g] Hz' % (what, MIN_FREQ, MAX_FREQ))


def _mpe_reference_csr(ref_freqs):
    """Ragged per-frame reference pitches (Hz) -> (offsets int64 [K + 1], flat float64 Hz), range-checked like multipitch_metrics."""
    frames = [np.asarray(f, dtype=np.float64).ravel() for f in ref_freqs]
    off = np.zeros(len(frames) + 1, dtype=np.int64)
    np.cumsum(np.array([f.size for f in frames], dtype=np.int64), out=off[1:])
    flat = np.concatenate(frames) if off[-1] else np.empty(0)
    if flat.size and (flat.max() > MAX_FREQ or flat.min() < MIN_FREQ):
        raise _mpe_range_error('reference')
    return off, flat


def _mpe_bin_tables(midi_freqs):
    """Per bin: the MIDI number the host route compares (bin -> Hz by ``activations_to_multi_pitch`` -> MIDI by
    ``frequencies_to_midi``: not bit-identical to ``midi_freqs``) and whether its frequency fails mir_eval's range check."""
    hz = midi_to_hz(np.asarray(midi_freqs, dtype=np.float64))
    return frequencies_to_midi([hz])[0], ((hz > MAX_FREQ) | (hz < MIN_FREQ)).astype(np.uint8)


def _mpe_activations(activations):
    if not isinstance(activations, torch.Tensor):
        raise RuntimeError('multipitch scoring on the device takes a GPU tensor of activations (got %s); the host function '
                           'multipitch_metrics takes frame lists' % type(activations).__name__)
    _hip.require_cuda(activations)
    x = activations.detach()
    if x.dim() == 3 and x.size(0) == 1:
        x = x[0]
    if x.dim() != 2:
        raise ValueError('activations must be (F, T) or (1, F, T) (got %s)' % (tuple(activations.shape),))
    if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError('unsupported dtype %s' % x.dtype)
    return x.to(torch.float32).contiguous()


def _mpe_estimate_args(x, est_time, midi_freqs, ref_mismatch=False):
    """``est_time`` and ``midi_freqs`` as float64 arrays, checked against the (F, T) of ``x``; ``ref_mismatch``: the list form's own check."""
    F, T = x.shape
    est_time = np.asarray(est_time, dtype=np.float64)
    midi_freqs = np.asarray(midi_freqs, dtype=np.float64)
    if ref_mismatch or len(est_time) != T:
        raise ValueError('time and frequency lists must have the same number of frames')
    if midi_freqs.shape != (F,):
        raise ValueError('midi_freqs must hold one value per bin (%d), got shape %s' % (F, midi_freqs.shape))
    return est_time, midi_freqs


def mpe_compact(activations, t=0.5, peaks_only=True, n_valid_bins=0, bin_bad=None):
    """
    The activation map as per-frame lists of active bins, on the device: ``(est_off int64 [T + 1], est_bins int32, n_est int32
    [T], bad int32 [T])`` with frame ``f``'s bins, ascending, at ``est_bins[est_off[f]:est_off[f + 1]]`` -- the non-zeros of
    ``peaks_above(x, t, n_valid_bins)`` (``peaks_only``) or of ``threshold`` of the masked map.  ``est_bins`` is allocated for the
    most bins the predicate can let through, so no count has to come back to the host in between.
    """
    x = _mpe_activations(activations)
    F, T = x.shape
    if F < 1 or T < 1:
        raise ValueError('activations hold no bin or no frame')
    lib, dev = _hip.lib(), x.device
    mode = 2 if peaks_only else 1
    fv = n_valid_bins if 0 < n_valid_bins < F else F
    per_frame = (fv + 1) // 2 if peaks_only else (fv if t > 0 else F)      # strict peaks cannot be adjacent
    n_est = torch.empty(T, dtype=torch.int32, device=dev)
    bad = torch.empty(T, dtype=torch.int32, device=dev)
    est_bins = torch.empty(max(per_frame * T, 1), dtype=torch.int32, device=dev)
    bad_t = None if bin_bad is None else torch.from_numpy(np.ascontiguousarray(bin_bad, dtype=np.uint8)).to(dev)
    with torch.cuda.device(dev):
        st = _hip.stream_ptr()
        _hip.check(lib.tt_mpe_count(_hip.ptr(x), F, T, float(t), mode, int(n_valid_bins), _hip.ptr(bad_t), _hip.ptr(n_est), _hip.ptr(bad), st),
                   'tt_mpe_count')
        est_off = torch.zeros(T + 1, dtype=torch.int64, device=dev)
        est_off[1:] = torch.cumsum(n_est, 0, dtype=torch.int64)
        _hip.check(lib.tt_mpe_fill(_hip.ptr(x), F, T, float(t), mode, int(n_valid_bins), _hip.ptr(est_off), est_bins.numel(),
                                   _hip.ptr(est_bins), st), 'tt_mpe_fill')
    return est_off, est_bins, n_est, bad


def multipitch_counts_device(ref_time, ref_freqs, est_time, activations, midi_freqs, window=0.5, t=0.5, peaks_only=True, n_valid_bins=0):
    """
    What ``multipitch_metrics(ref_time, ref_freqs, est_time, activations_to_multi_pitch(activations, midi_freqs, peaks_only, t))``
    counts per reference frame, from ``activations`` -- a CUDA fp32 / fp16 / bf16 tensor (F, T) or (1, F, T), 16-bit upcast to fp32
    -- that never leave the device: a dict of int32 device tensors ``tp``, ``tp_chroma``, ``n_ref``, ``n_est`` (one entry per
    reference frame), ``n_host_frames`` and ``sums`` (the eight integer sums the scores are formed from, int64 ndarray).

    On the host, vectorised over the ragged reference only: the reference as CSR in MIDI numbers, the estimate frame every
    reference frame reads (``resample_multipitch``'s arithmetic), the per-bin MIDI table of the host route.  On the device:
    tt_mpe_count -> prefix sum -> tt_mpe_fill -> tt_mpe_match -> integer sums, then ONE copy of ten int64 values.  A frame
    with more than MPE_MAX_REF reference pitches or more than MPE_MAX_EST active bins comes back flagged; only those frames'
    bins are downloaded and matched by ``_max_matching`` (``n_host_frames`` of them; none at evaluate()'s settings, where a frame
    holds at most 236 peaks).  ``ValueError`` as from the host function: length mismatch, reference or -- known after the copy --
    estimated frequency outside [20, 5000] Hz.  CPU tensors raise ``RuntimeError``: there is no CPU fallback.
    """
    x = _mpe_activations(activations)
    F, T = x.shape
    dev = x.device
    ref_time = np.asarray(ref_time, dtype=np.float64)
    est_time, midi_freqs = _mpe_estimate_args(x, est_time, midi_freqs, len(ref_time) != len(ref_freqs))
    ref_off, ref_hz = _mpe_reference_csr(ref_freqs)
    if len(ref_time) == 0 or T == 0 or F == 0:
        return _mpe_no_counts(len(ref_time), dev)
    ref_midi = frequencies_to_midi([ref_hz])[0]
    return _mpe_counts_from_csr(x, ref_time, est_time, midi_freqs, torch.from_numpy(ref_off).to(dev), torch.from_numpy(ref_midi).to(dev),
                                window, t, peaks_only, n_valid_bins)


def _mpe_no_counts(K, dev):
    empty = torch.zeros(K, dtype=torch.int32, device=dev)
    return dict(tp=empty, tp_chroma=empty.clone(), n_ref=empty.clone(), n_est=empty.clone(), n_host_frames=0,
                sums=np.zeros(len(_MPE_SUMS), dtype=np.int64))


def _mpe_counts_from_csr(x, ref_time, est_time, midi_freqs, ref_off_d, ref_midi_d, window, t, peaks_only, n_valid_bins):
    """
    The device leg of ``multipitch_counts_device`` from a reference that is already a CSR on the device -- ``ref_off_d`` int64
    [K + 1], ``ref_midi_d`` float64 MIDI numbers, range-checked by the caller -- and checked activations ``x`` (F, T) fp32 with
    K, T, F >= 1.  The reference pitches of frames over a capacity, and only those, are read back for the host matcher.
    """
    F, T = x.shape
    dev, K = x.device, len(ref_time)
    lib = _hip.lib()
    if (lib.tt_mpe_max_est(), lib.tt_mpe_max_ref()) != (MPE_MAX_EST, MPE_MAX_REF):
        raise RuntimeError('libttrap_hip.so was built with capacities (%d, %d), metrics says (%d, %d)'
                           % (lib.tt_mpe_max_est(), lib.tt_mpe_max_ref(), MPE_MAX_EST, MPE_MAX_REF))
    est_idx = _nearest_frame_index(est_time, ref_time, T).astype(np.int32)
    est_midi, bin_bad = _mpe_bin_tables(midi_freqs)

    est_off, est_bins, n_act, bad = mpe_compact(x, t, peaks_only, n_valid_bins, bin_bad)
    if ref_midi_d.numel() == 0:
        ref_midi_d = torch.zeros(1, dtype=torch.float64, device=dev)
    est_idx_d = torch.from_numpy(est_idx).to(dev)
    est_midi_d = torch.from_numpy(est_midi).to(dev)
    tp = torch.empty(K, dtype=torch.int32, device=dev)
    tpc = torch.zeros(K, dtype=torch.int32, device=dev)
    n_est = torch.zeros(K, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _hip.check(lib.tt_mpe_match(_hip.ptr(est_idx_d), K, T, _hip.ptr(est_off), _hip.ptr(est_bins), _hip.ptr(est_midi_d), F,
                                    _hip.ptr(ref_off_d), _hip.ptr(ref_midi_d), float(window), _hip.ptr(tp), _hip.ptr(tpc), _hip.ptr(n_est),
                                    _hip.stream_ptr()), 'tt_mpe_match')
    n_ref = (ref_off_d[1:] - ref_off_d[:-1]).to(torch.int32)
    flagged = tp < 0
    done = (~flagged).to(torch.int64)                  # flagged frames stay out of the device sums: the host adds theirs
    sums = _mpe_sums(tp * done, tpc * done, n_ref * done, n_est * done, torch)
    back = torch.stack(sums + [flagged.sum(), bad.sum(dtype=torch.int64)]).cpu().numpy()        # the one device -> host copy
    if back[-1]:
        raise _mpe_range_error('estimate')
    sums, n_host = back[:len(_MPE_SUMS)].copy(), int(back[-2])
    if n_host:
        # over a capacity of the kernel: these frames alone are matched by the host function, from their own bins and reference pitches
        js = torch.nonzero(flagged).flatten()
        fr = est_idx_d[js].to(torch.int64).clamp(max=T - 1)
        spans = torch.stack([js, est_off[fr], est_off[fr + 1], ref_off_d[js], ref_off_d[js + 1]], 1).cpu().numpy()
        got = np.zeros((n_host, 4), dtype=np.int64)
        for row, (j, lo, hi, r_lo, r_hi) in zip(got, spans):
            bins = est_bins[lo:hi].cpu().numpy() if est_idx[j] < T else np.empty(0, dtype=np.int64)
            r, e = ref_midi_d[r_lo:r_hi].cpu().numpy(), est_midi[bins]
            row[:] = (_max_matching(r, e, window, False), _max_matching(np.mod(r, 12), np.mod(e, 12), window, True), len(r), len(e))
        sums += np.array(_mpe_sums(got[:, 0], got[:, 1], got[:, 2], got[:, 3], np), dtype=np.int64)
        fix = torch.from_numpy(got.astype(np.int32)).to(dev)
        tp[js], tpc[js], n_est[js] = fix[:, 0], fix[:, 1], fix[:, 3]
    return dict(tp=tp, tp_chroma=tpc, n_ref=n_ref, n_est=n_est, n_host_frames=n_host, sums=sums)


def multipitch_metrics_device(ref_time, ref_freqs, est_time, activations, midi_freqs, window=0.5, t=0.5, peaks_only=True, n_valid_bins=0):
    """
    The fourteen scores of ``multipitch_metrics`` (same keys, same float64 values bit for bit) for estimates given as device
    activations: see ``multipitch_counts_device``.  Empty ``ref_time`` or ``est_time`` give the all-zero dictionary.
    """
    counts = multipitch_counts_device(ref_time, ref_freqs, est_time, activations, midi_freqs, window, t, peaks_only, n_valid_bins)
    return _scores_from_sums(counts['sums'])


def multipitch_counts_device_notes(ref_time, pitches_hz, intervals, est_time, activations, midi_freqs, window=0.5, t=0.5, peaks_only=True,
                                   n_valid_bins=0):
    """
    ``multipitch_counts_device(ref_time, notes_to_multi_pitch(pitches_hz, intervals, ref_time), ...)`` -- the same dictionary, bit for
    bit -- for a reference given as notes (reference ``experiments/evaluate.py:67-75`` on a ``NoteDataset``): the per-frame reference
    lists are never formed on the host.  The CSR of note indices is built on the device (csrc/notes.hip) and gathered through a
    per-note MIDI table (``frequencies_to_midi`` over the L pitches); its total and two flags come back in one small copy.
    ``ValueError`` as from the host route: ``pitches_hz`` / ``intervals`` length mismatch, a pitch outside [20, 5000] Hz of a note that
    sounds in at least one frame (a silent note's pitch is never looked at, there as here).  ``ref_time`` that are not sorted take
    the host lists.
    """
    pitches, intervals, ref_time = _notes._note_arrays(pitches_hz, intervals, ref_time)
    if not _notes._is_sorted(ref_time):
        return multipitch_counts_device(ref_time, _notes.notes_to_multi_pitch(pitches, intervals, ref_time), est_time, activations,
                                        midi_freqs, window, t, peaks_only, n_valid_bins)
    x = _mpe_activations(activations)
    F, T = x.shape
    dev = x.device
    est_time, midi_freqs = _mpe_estimate_args(x, est_time, midi_freqs)
    K = len(ref_time)
    lo, hi = _notes._device_spans(intervals, ref_time, dev)
    # _mpe_reference_csr's range check, on the notes that sound: max() > MAX_FREQ or min() < MIN_FREQ over their pitches (a NaN among
    # them makes both comparisons false)
    sounding = hi > lo
    outside = torch.from_numpy((pitches > MAX_FREQ) | (pitches < MIN_FREQ)).to(dev)
    nan = torch.from_numpy(np.isnan(pitches)).to(dev)
    ref_off_d, note_idx, (any_outside, any_nan) = _notes._device_csr(lo, hi, K, ((sounding & outside).any(), (sounding & nan).any()))
    if any_outside and not any_nan:
        raise _mpe_range_error('reference')
    if K == 0 or T == 0 or F == 0:
        return _mpe_no_counts(K, dev)
    with np.errstate(divide='ignore', invalid='ignore'):                 # a silent note may carry any pitch, 0 included
        note_midi = frequencies_to_midi([pitches])[0]
    ref_midi_d = torch.from_numpy(note_midi).to(dev)[note_idx.to(torch.int64)]
    return _mpe_counts_from_csr(x, ref_time, est_time, midi_freqs, ref_off_d, ref_midi_d, window, t, peaks_only, n_valid_bins)


def multipitch_metrics_device_notes(ref_time, pitches_hz, intervals, est_time, activations, midi_freqs, window=0.5, t=0.5, peaks_only=True,
                                    n_valid_bins=0):
    """The fourteen scores of ``multipitch_metrics_device`` for a reference given as notes: see ``multipitch_counts_device_notes``."""
    counts = multipitch_counts_device_notes(ref_time, pitches_hz, intervals, est_time, activations, midi_freqs, window, t, peaks_only,
                                            n_valid_bins)
    return _scores_from_sums(counts['sums'])


def multipitch_counts_device_track(bank, track_id, est_time, activations, midi_freqs, window=0.5, t=0.5, peaks_only=True, n_valid_bins=0):
    """
    ``multipitch_counts_device(times, multi_pitch, ...)`` -- the same dictionary, bit for bit -- for the reference ``(times,
    multi_pitch) = bank.tracks[track_id]`` of a ``utils.pitch.PitchBank`` (reference ``experiments/evaluate.py:76-78,116`` on an
    ``MPEDataset``): the ragged lists are not flattened and uploaded again per call, the matching kernel reads the bank's row offsets
    and MIDI numbers where they are.  ``ValueError`` as from the list route: estimate times / frames mismatch, a reference pitch
    outside [20, 5000] Hz (found once, when the bank was built).
    """
    x = _mpe_activations(activations)
    F, T = x.shape
    if not 0 <= int(track_id) < len(bank):
        raise IndexError('track id outside [0, %d)' % len(bank))
    if x.device != bank.device:
        raise RuntimeError('activations are on %s, the bank on %s' % (x.device, bank.device))
    est_time, midi_freqs = _mpe_estimate_args(x, est_time, midi_freqs)
    if bank.host['outside'][track_id]:
        raise _mpe_range_error('reference')
    ref_time = bank.track_times(track_id)
    if len(ref_time) == 0 or T == 0 or F == 0:
        return _mpe_no_counts(len(ref_time), x.device)
    ref_off_d, ref_midi_d = bank.reference_csr(track_id)
    return _mpe_counts_from_csr(x, ref_time, est_time, midi_freqs, ref_off_d, ref_midi_d, window, t, peaks_only, n_valid_bins)


def multipitch_metrics_device_track(bank, track_id, est_time, activations, midi_freqs, window=0.5, t=0.5, peaks_only=True, n_valid_bins=0):
    """The fourteen scores of ``multipitch_metrics_device`` for a reference kept in a ``PitchBank``: see ``multipitch_counts_device_track``."""
    counts = multipitch_counts_device_track(bank, track_id, est_time, activations, midi_freqs, window, t, peaks_only, n_valid_bins)
    return _scores_from_sums(counts['sums'])
