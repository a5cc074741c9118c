"""
Scoring next to the hot path: what reference ``experiments/evaluate.py:113-127`` computes
per track from the outputs of the path -- frame-level multi-pitch precision / recall / F1 and the reconstruction SDR.

The reference delegates both to third-party packages that are absent from this image:
  * ``mir_eval.multipitch.evaluate(ref_time, ref_freqs, est_time, est_freqs, window=0.5)`` called from
    ``timbre_trap/utils/experiments.py:376-378``;
  * ``torchmetrics.audio.SignalDistortionRatio()`` (defaults) called from ``experiments/evaluate.py:40,123``.
``multipitch_metrics`` and ``signal_distortion_ratio`` restate their published algorithms (mir_eval's multipitch module after
Poliner & Ellis 2007 / Bay et al. 2009; the filtered SDR of Scheibler 2021, "SDR -- medium rare with fast computations", as
implemented by torchmetrics / fast_bss_eval).  PARITY UNPINNED against the packages themselves (neither is installed and there
is no network); pinned instead by known-answer tests (tests/test_metrics.py) and, for the SDR, by an independent dense
least-squares derivation of the same quantity.  Host code in float64, as in the reference (NumPy lists / CPU tensors).

``multipitch_counts_device`` / ``multipitch_metrics_device`` / ``MultipitchEvaluator.evaluate_activations`` give the scores of
``multipitch_metrics`` bit for bit from activations that stay on the device (csrc/mpe.hip: compaction of the activation map to
per-frame bin lists, a maximum matching per reference frame in float64, integer sums; one small copy back per track).

``note_metrics`` / ``note_counts`` are the note-level score (precision / recall / F-measure of estimated against reference notes, with
and without the offset criterion) in the manner of ``mir_eval.transcription``, which the reference never calls and which is absent here
too: restated from the published algorithm, PARITY UNPINNED against the package, pinned by known answers and by an independent
maximum-matching routine (tests/test_notescore_restatement.py).  ``note_counts_device`` / ``note_metrics_device`` /
``MultipitchEvaluator.evaluate_events`` give the same counts, integer for integer, for estimated notes that stay on the device
(csrc/notescore.hip: onset windows by binary search, connected components by label propagation, one matching per component).

``signal_distortion_ratio_device`` / ``SignalDistortionRatio`` compute the same SDR where ``experiments/evaluate.py:51,122-127``
asks for it -- on the device, right after ``sliCQ.decode`` -- in float64 HIP kernels (csrc/sdr.hip: direct correlation sums and a
Levinson recursion instead of FFTs and a dense solve); ``signal_distortion_ratio`` stays the float64 yardstick they are tested against.
"""

import sys
from collections import namedtuple
from copy import deepcopy

import numpy as np
import torch

from .. import _hip
from .events import NoteEvents
from .targets import midi_to_hz

__all__ = ['resample_multipitch', 'frequencies_to_midi', 'match_count', 'multipitch_metrics', 'MultipitchEvaluator',
           'multipitch_counts_device', 'multipitch_metrics_device', 'multipitch_counts_device_notes',
           'multipitch_metrics_device_notes', 'multipitch_counts_device_track', 'multipitch_metrics_device_track', 'mpe_compact', 'MPE_MAX_EST', 'MPE_MAX_REF',
           'signal_distortion_ratio', 'signal_distortion_ratio_device', 'SignalDistortionRatio', 'SDR_CHUNK', 'SDR_MAX_FILTER',
           'note_counts', 'note_metrics', 'note_counts_device', 'note_metrics_device', 'NoteCounts', 'DeviceNoteCounts', 'NOTESCORE_MAX',
           'NOTESCORE_ROUNDS']

MAX_FREQ, MIN_FREQ = 5000.0, 20.0            # mir_eval.multipitch validation limits (evaluate.py:44-48 masks bins above 5 kHz)


def _nearest_frame_index(times, target_times, n):
    """Index of the frame of ``times`` (n of them, float64, non-empty) nearest to every target time; ties go to the earlier frame;
    ``n`` for targets outside [times[0], times[-1]] (an empty frame)."""
    half = times / 2.0
    mids = half[1:] + half[:-1]
    idx = np.clip(np.searchsorted(mids, target_times, side='left'), 0, n - 1)
    return np.where((target_times < times[0]) | (target_times > times[-1]), n, idx)


def resample_multipitch(times, frequencies, target_times):
    """
    Frame lists re-read at ``target_times`` by nearest neighbour (mir_eval.multipitch.resample_multipitch): ties go to the
    earlier frame; targets outside [times[0], times[-1]] get an empty frame.
    """
    target_times = np.asarray(target_times, dtype=np.float64)
    if target_times.size == 0:
        return []
    times = np.asarray(times, dtype=np.float64)
    if times.size == 0:
        return [np.array([])] * len(target_times)
    idx = _nearest_frame_index(times, target_times, len(frequencies))
    vals = list(frequencies) + [np.array([])]
    return [vals[int(i)] for i in idx]


def frequencies_to_midi(frequencies, ref_frequency=440.0):
    """Hz -> (fractional) MIDI note numbers, frame by frame."""
    return [69.0 + 12.0 * np.log2(np.asarray(f, dtype=np.float64) / ref_frequency) for f in frequencies]


def midi_to_chroma(frequencies_midi):
    """Wrap MIDI numbers into one octave (mod 12)."""
    return [np.mod(f, 12) for f in frequencies_midi]


def _max_matching(ref, est, window, chroma):
    """
    Size of a maximum matching between reference and estimated pitches of one frame, a pair being admissible when the
    pitches are at most ``window`` semitones apart (``mir_eval.util.match_events``: |ref - est| <= window, with the
    octave-wrapped distance min(d, 12 - d) in chroma mode).  Augmenting paths (Kuhn): frames hold a handful of pitches.
    """
    if len(ref) == 0 or len(est) == 0:
        return 0
    diff = np.abs(np.subtract.outer(np.asarray(ref, dtype=np.float64), np.asarray(est, dtype=np.float64)))
    if chroma:
        diff = np.mod(diff, 12)
        diff = np.minimum(diff, 12 - diff)
    adj = diff <= window
    match_est = -np.ones(len(est), dtype=np.int64)

    def augment(r, seen):
        for e in np.flatnonzero(adj[r]):
            if seen[e]:
                continue
            seen[e] = True
            if match_est[e] < 0 or augment(match_est[e], seen):
                match_est[e] = r
                return True
        return False
    count = 0
    for r in range(len(ref)):
        if augment(r, np.zeros(len(est), dtype=bool)):
            count += 1
    return count


def match_count(ref_midi, est_midi, window=0.5, chroma=False):
    """True positives per frame."""
    return np.array([_max_matching(r, e, window, chroma) for r, e in zip(ref_midi, est_midi)], dtype=np.float64)


def _prf_from_sums(tps, nr, ne, denom):
    """Precision, recall, accuracy from sum(tp), sum(n_ref), sum(n_est), sum(n_est + n_ref - tp) as float64."""
    precision = tps / ne if ne > 0 else 0.0
    recall = tps / nr if nr > 0 else 0.0
    accuracy = tps / denom if denom > 0 else 0.0
    return float(precision), float(recall), float(accuracy)


def _errors_from_sums(nr, sub, miss, fa, tot):
    """The four error scores from sum(n_ref) and the sums of their per-frame numerators, as float64."""
    if nr == 0:
        return 0.0, 0.0, 0.0, 0.0
    return float(sub / nr), float(miss / nr), float(fa / nr), float(tot / nr)


def _prf_accuracy(tp, n_ref, n_est):
    return _prf_from_sums(tp.sum(), n_ref.sum(), n_est.sum(), (n_est + n_ref - tp).sum())


def _error_scores(tp, n_ref, n_est):
    return _errors_from_sums(n_ref.sum(), (np.minimum(n_ref, n_est) - tp).sum(), np.maximum(n_ref - n_est, 0).sum(),
                             np.maximum(n_est - n_ref, 0).sum(), (np.maximum(n_ref, n_est) - tp).sum())


_SCORE_KEYS = ['Precision', 'Recall', 'Accuracy', 'Substitution Error', 'Miss Error', 'False Alarm Error', 'Total Error']


def multipitch_metrics(ref_time, ref_freqs, est_time, est_freqs, window=0.5):
    """
    The fourteen scores of ``mir_eval.multipitch.evaluate`` (same key names): estimates are re-read on the REFERENCE time base
    by nearest neighbour, every frame's pitches go to MIDI, and true positives per frame are the size of a maximum matching of
    reference and estimated pitches at most ``window`` semitones apart (octave-wrapped for the Chroma scores).
    """
    ref_time = np.asarray(ref_time, dtype=np.float64)
    est_time = np.asarray(est_time, dtype=np.float64)
    if len(ref_time) != len(ref_freqs) or len(est_time) != len(est_freqs):
        raise ValueError('time and frequency lists must have the same number of frames')
    for name, freqs in (('reference', ref_freqs), ('estimate', est_freqs)):
        for f in freqs:
            f = np.asarray(f)
            if f.size and (f.max() > MAX_FREQ or f.min() < MIN_FREQ):
                raise ValueError('%s frequencies must lie in [%g, %g] Hz' % (name, MIN_FREQ, MAX_FREQ))
    keys = _SCORE_KEYS
    out = {k: 0.0 for k in keys + ['Chroma ' + k for k in keys]}
    if len(ref_time) == 0 or len(est_time) == 0:
        return out
    est_resampled = resample_multipitch(est_time, est_freqs, ref_time)
    ref_midi, est_midi = frequencies_to_midi(ref_freqs), frequencies_to_midi(est_resampled)
    n_ref = np.array([len(f) for f in ref_midi], dtype=np.float64)
    n_est = np.array([len(f) for f in est_midi], dtype=np.float64)
    for prefix, chroma in (('', False), ('Chroma ', True)):
        r = midi_to_chroma(ref_midi) if chroma else ref_midi
        e = midi_to_chroma(est_midi) if chroma else est_midi
        tp = match_count(r, e, window, chroma)
        p, rc, a = _prf_accuracy(tp, n_ref, n_est)
        es, em, ef, et = _error_scores(tp, n_ref, n_est)
        for k, v in zip(keys, (p, rc, a, es, em, ef, et)):
            out[prefix + k] = v
    return out


class MultipitchEvaluator(object):
    """
    Result tracker with the reference's interface (``timbre_trap/utils/experiments.py:277-396``): ``evaluate`` returns the
    scores above under lower-case keys prefixed ``mpe/`` plus ``mpe/f1-score = 2 P R / (P + R + eps)``; ``append_results`` /
    ``average_results`` accumulate per-track dictionaries and give rounded means and standard deviations.
    """

    def __init__(self, tolerance=0.5):
        self.tolerance = tolerance
        self.results = None
        self.reset_results()

    def reset_results(self):
        self.results = {}

    def append_results(self, results):
        for key in results.keys():
            if key in self.results.keys():
                self.results[key] = np.append(self.results[key], results[key])
            else:
                self.results[key] = np.array([results[key]])

    def average_results(self):
        mean, std_dev = deepcopy(self.results), deepcopy(self.results)
        for key in self.results.keys():
            mean[key] = round(np.mean(mean[key]), 5)
            std_dev[key] = round(np.std(std_dev[key]), 5)
        return mean, std_dev

    @staticmethod
    def _tagged(scores):
        results = {k.lower(): v for k, v in scores.items()}
        pr, rc = results['precision'], results['recall']
        results['f1-score'] = 2 * pr * rc / (pr + rc + sys.float_info.epsilon)
        return {'mpe/' + k: v for k, v in results.items()}

    def evaluate(self, times_est, multi_pitch_est, times_ref, multi_pitch_ref):
        return self._tagged(multipitch_metrics(times_ref, multi_pitch_ref, times_est, multi_pitch_est, window=self.tolerance))

    def evaluate_activations(self, times_est, activations, midi_freqs, times_ref, multi_pitch_ref, n_valid_bins=0):
        """
        ``evaluate`` for activations that are still on the device -- the (F, T) or (1, F, T) tensor ``model.to_activations``
        returned -- instead of frame lists: the same ``mpe/...`` dictionary as ``evaluate(times_est,
        activations_to_multi_pitch(masked activations, midi_freqs, peaks_only=True), times_ref, multi_pitch_ref)``, bit for bit,
        without downloading the map (reference ``experiments/evaluate.py:100-116``).  ``n_valid_bins`` > 0 zeroes the rows from
        that bin upwards first (``evaluate.py:107-112``).
        """
        return self._tagged(multipitch_metrics_device(times_ref, multi_pitch_ref, times_est, activations, midi_freqs,
                                                      window=self.tolerance, n_valid_bins=n_valid_bins))

    def evaluate_notes(self, times_est, activations, midi_freqs, times_ref, pitches_hz, intervals, n_valid_bins=0):
        """
        ``evaluate_activations`` for a reference given as notes -- ``pitches_hz`` (L), ``intervals`` (L, 2) -- instead of frame lists:
        the dictionary of ``evaluate_activations(..., times_ref, notes_to_multi_pitch(pitches_hz, intervals, times_ref))``, bit for
        bit, with the reference lists built on the device too (reference ``experiments/evaluate.py:67-75,100-116`` on a ``NoteDataset``).
        """
        return self._tagged(multipitch_metrics_device_notes(times_ref, pitches_hz, intervals, times_est, activations, midi_freqs,
                                                            window=self.tolerance, n_valid_bins=n_valid_bins))

    def evaluate_track(self, times_est, activations, midi_freqs, bank, track_id, n_valid_bins=0):
        """
        ``evaluate_activations`` for a reference kept on the device in a ``utils.pitch.PitchBank``: the dictionary of
        ``evaluate_activations(..., *bank.tracks[track_id])``, bit for bit, without flattening and uploading the track's lists again
        (reference ``experiments/evaluate.py:76-78,100-116`` on an ``MPEDataset``).
        """
        return self._tagged(multipitch_metrics_device_track(bank, track_id, times_est, activations, midi_freqs, window=self.tolerance,
                                                            n_valid_bins=n_valid_bins))

    def evaluate_events(self, events, hop_seconds, pitches, intervals, item=0, **tolerances):
        """
        Note-level scores of the notes of batch item ``item`` of ``events`` (a ``NoteEvents`` on the device) against one track's
        annotation -- ``pitches`` (L) in MIDI numbers, ``intervals`` (L, 2) in seconds, as ``NoteDataset.get_ground_truth`` returns them
        with pitches converted to MIDI: the six scores of ``note_metrics_device`` under lower-case keys prefixed ``note/``, ready for
        ``append_results``.  ``hop_seconds``: as for ``events_to_notes``.  The pitch tolerance defaults to the evaluator's.
        """
        tolerances.setdefault('pitch_tolerance', self.tolerance)
        sel = events.item == int(item)
        est = NoteEvents(*(f[sel] for f in events))
        est = est._replace(item=torch.zeros_like(est.item))
        scores = note_metrics_device(est, [(pitches, intervals)], hop_seconds, **tolerances)[0]
        return {'note/' + k.lower(): v for k, v in scores.items()}


# ---- multi-pitch scores on the device (csrc/mpe.hip) -------------------------------------------------------------------------

MPE_MAX_EST = 256         # active bins per frame the matching kernel holds (= tt_mpe_max_est(), checked on first use)
MPE_MAX_REF = 64          # reference pitches per frame it holds (= tt_mpe_max_ref())
# the integer sums the fourteen scores are formed from, in the order of the one int64 tensor that comes back per track
_MPE_SUMS = ('tp', 'tp_chroma', 'n_ref', 'n_est', 'min', 'max', 'miss', 'false_alarm')


def _mpe_sums(tp, tpc, n_ref, n_est, xp):
    """The eight sums of _MPE_SUMS over int64 per-frame counts (``xp``: torch for device tensors, np for arrays)."""
    zero = n_ref * 0
    return [tp.sum(), tpc.sum(), n_ref.sum(), n_est.sum(), xp.minimum(n_ref, n_est).sum(), xp.maximum(n_ref, n_est).sum(),
            xp.maximum(n_ref - n_est, zero).sum(), xp.maximum(n_est - n_ref, zero).sum()]


def _scores_from_sums(sums):
    """``multipitch_metrics``' dictionary from the integer sums (exact in float64: every sum is far below 2^53)."""
    s = {k: np.float64(v) for k, v in zip(_MPE_SUMS, sums)}
    out = {}
    for prefix, tps in (('', s['tp']), ('Chroma ', s['tp_chroma'])):
        prf = _prf_from_sums(tps, s['n_ref'], s['n_est'], s['n_est'] + s['n_ref'] - tps)
        err = _errors_from_sums(s['n_ref'], s['min'] - tps, s['miss'], s['false_alarm'], s['max'] - tps)
        for k, v in zip(_SCORE_KEYS, prf + err):
            out[prefix + k] = v
    return out


def _mpe_reference_csr(ref_freqs):
    """Ragged per-frame reference pitches (Hz) -> (offsets int64 [K + 1], flat float64 Hz), range-checked like multipitch_metrics."""
    frames = [np.asarray(f, dtype=np.float64).ravel() for f in ref_freqs]
    off = np.zeros(len(frames) + 1, dtype=np.int64)
    np.cumsum(np.array([f.size for f in frames], dtype=np.int64), out=off[1:])
    flat = np.concatenate(frames) if off[-1] else np.empty(0)
    if flat.size and (flat.max() > MAX_FREQ or flat.min() < MIN_FREQ):
        raise ValueError('reference frequencies must lie in [%g, %g] Hz' % (MIN_FREQ, MAX_FREQ))
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
    est_time = np.asarray(est_time, dtype=np.float64)
    midi_freqs = np.asarray(midi_freqs, dtype=np.float64)
    if len(ref_time) != len(ref_freqs) or len(est_time) != T:
        raise ValueError('time and frequency lists must have the same number of frames')
    if midi_freqs.shape != (F,):
        raise ValueError('midi_freqs must hold one value per bin (%d), got shape %s' % (F, midi_freqs.shape))
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
        raise ValueError('estimate frequencies must lie in [%g, %g] Hz' % (MIN_FREQ, MAX_FREQ))
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
    from . import notes as _notes
    pitches, intervals, ref_time = _notes._note_arrays(pitches_hz, intervals, ref_time)
    if not _notes._is_sorted(ref_time):
        return multipitch_counts_device(ref_time, _notes.notes_to_multi_pitch(pitches, intervals, ref_time), est_time, activations,
                                        midi_freqs, window, t, peaks_only, n_valid_bins)
    x = _mpe_activations(activations)
    F, T = x.shape
    dev = x.device
    est_time = np.asarray(est_time, dtype=np.float64)
    midi_freqs = np.asarray(midi_freqs, dtype=np.float64)
    if len(est_time) != T:
        raise ValueError('time and frequency lists must have the same number of frames')
    if midi_freqs.shape != (F,):
        raise ValueError('midi_freqs must hold one value per bin (%d), got shape %s' % (F, midi_freqs.shape))
    K = len(ref_time)
    lo, hi = _notes._device_spans(intervals, ref_time, dev)
    # _mpe_reference_csr's range check, on the notes that sound: max() > MAX_FREQ or min() < MIN_FREQ over their pitches (a NaN among
    # them makes both comparisons false)
    sounding = hi > lo
    outside = torch.from_numpy((pitches > MAX_FREQ) | (pitches < MIN_FREQ)).to(dev)
    nan = torch.from_numpy(np.isnan(pitches)).to(dev)
    ref_off_d, note_idx, (any_outside, any_nan) = _notes._device_csr(lo, hi, K, ((sounding & outside).any(), (sounding & nan).any()))
    if any_outside and not any_nan:
        raise ValueError('reference frequencies must lie in [%g, %g] Hz' % (MIN_FREQ, MAX_FREQ))
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
    est_time = np.asarray(est_time, dtype=np.float64)
    midi_freqs = np.asarray(midi_freqs, dtype=np.float64)
    if not 0 <= int(track_id) < len(bank):
        raise IndexError('track id outside [0, %d)' % len(bank))
    if x.device != bank.device:
        raise RuntimeError('activations are on %s, the bank on %s' % (x.device, bank.device))
    if len(est_time) != T:
        raise ValueError('time and frequency lists must have the same number of frames')
    if midi_freqs.shape != (F,):
        raise ValueError('midi_freqs must hold one value per bin (%d), got shape %s' % (F, midi_freqs.shape))
    if bank.host['outside'][track_id]:
        raise ValueError('reference frequencies must lie in [%g, %g] Hz' % (MIN_FREQ, MAX_FREQ))
    ref_time = bank.track_times(track_id)
    if len(ref_time) == 0 or T == 0 or F == 0:
        return _mpe_no_counts(len(ref_time), x.device)
    ref_off_d, ref_midi_d = bank.reference_csr(track_id)
    return _mpe_counts_from_csr(x, ref_time, est_time, midi_freqs, ref_off_d, ref_midi_d, window, t, peaks_only, n_valid_bins)


def multipitch_metrics_device_track(bank, track_id, est_time, activations, midi_freqs, window=0.5, t=0.5, peaks_only=True, n_valid_bins=0):
    """The fourteen scores of ``multipitch_metrics_device`` for a reference kept in a ``PitchBank``: see ``multipitch_counts_device_track``."""
    counts = multipitch_counts_device_track(bank, track_id, est_time, activations, midi_freqs, window, t, peaks_only, n_valid_bins)
    return _scores_from_sums(counts['sums'])


# ---- SDR --------------------------------------------------------------------------------------------------------------

def _next_pow2(n):
    return 1 << int(np.ceil(np.log2(max(int(n), 1))))


def signal_distortion_ratio(preds, target, filter_length=512, zero_mean=False, load_diag=None):
    """
    Signal-to-distortion ratio in dB, the distortion being what is left of ``preds`` after projection onto the span of
    ``filter_length`` delayed copies of ``target`` (BSS-eval's SDR, computed the fast way):

        both signals scaled to unit norm;  r = autocorrelation of target (lags 0 .. L-1),  b = cross-correlation target -> preds;
        solve  Toeplitz(r) h = b ;   coherence = b . h ;   SDR = 10 log10(coherence / (1 - coherence)).

    ``preds`` / ``target``: arrays or tensors (..., time); float64 throughout; returns an ndarray of the leading shape (a float
    for 1-D input).  Mirrors ``torchmetrics.functional.audio.signal_distortion_ratio`` with its defaults (dense solve).
    """
    p = np.asarray(preds.detach().cpu() if hasattr(preds, 'detach') else preds, dtype=np.float64)
    t = np.asarray(target.detach().cpu() if hasattr(target, 'detach') else target, dtype=np.float64)
    if p.shape != t.shape:
        raise ValueError('preds and target must have the same shape')
    if zero_mean:
        p = p - p.mean(axis=-1, keepdims=True)
        t = t - t.mean(axis=-1, keepdims=True)
    t = t / np.maximum(np.linalg.norm(t, axis=-1, keepdims=True), 1e-6)
    p = p / np.maximum(np.linalg.norm(p, axis=-1, keepdims=True), 1e-6)
    n_fft = _next_pow2(p.shape[-1] + t.shape[-1] - 1)
    tf = np.fft.rfft(t, n=n_fft, axis=-1)
    r0 = np.fft.irfft(tf.real ** 2 + tf.imag ** 2, n=n_fft, axis=-1)[..., :filter_length]
    b = np.fft.irfft(np.conj(tf) * np.fft.rfft(p, n=n_fft, axis=-1), n=n_fft, axis=-1)[..., :filter_length]
    if load_diag is not None:
        r0 = r0.copy()
        r0[..., 0] += load_diag
    lead = r0.shape[:-1]
    r0f, bf = r0.reshape(-1, filter_length), b.reshape(-1, filter_length)
    idx = np.abs(np.subtract.outer(np.arange(filter_length), np.arange(filter_length)))
    out = np.empty(r0f.shape[0])
    for i in range(r0f.shape[0]):
        sol = np.linalg.solve(r0f[i][idx], bf[i])
        coh = float(np.dot(bf[i], sol))
        ratio = coh / (1.0 - coh)
        out[i] = 10.0 * np.log10(ratio) if ratio > 0 else -np.inf
    return float(out[0]) if not lead else out.reshape(lead)


# ---- SDR on the device (csrc/sdr.hip) ------------------------------------------------------------------------------------

SDR_CHUNK = 8192          # samples per workgroup of the correlation kernel (= tt_sdr_chunk(), checked on first use)
SDR_MAX_FILTER = 512      # largest filter_length the kernels hold in LDS


def _sdr_check(preds, target, filter_length):
    _hip.require_cuda(preds, target)
    if preds.shape != target.shape:
        raise ValueError('preds and target must have the same shape (got %s and %s)' % (tuple(preds.shape), tuple(target.shape)))
    if preds.dim() < 1 or preds.shape[-1] < 1:
        raise ValueError('preds and target must be (..., time) with at least one sample')
    if int(filter_length) != filter_length or not 1 <= filter_length <= SDR_MAX_FILTER:
        raise ValueError('filter_length must be an integer in [1, %d] (got %r)' % (SDR_MAX_FILTER, filter_length))
    for x in (preds, target):
        if x.dtype == torch.float64:
            raise ValueError('signal_distortion_ratio_device takes fp32 / fp16 / bf16 tensors; float64 input is what the host '
                             'function signal_distortion_ratio is for')
        if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError('unsupported dtype %s' % x.dtype)
    lib = _hip.lib()
    if lib.tt_sdr_chunk() != SDR_CHUNK:
        raise RuntimeError('libttrap_hip.so was built with a chunk of %d samples, metrics.SDR_CHUNK says %d' % (lib.tt_sdr_chunk(), SDR_CHUNK))
    return lib


def sdr_correlations(preds, target, filter_length=512, zero_mean=False):
    """
    The un-normalised sums the device SDR rests on: a float64 device tensor (B, 2 L + 1) holding, per clip of the flattened
    leading shape, r[0..L) (autocorrelation of ``target``), b[0..L) (cross-correlation target -> preds) and sum(preds^2),
    all linear (zeros beyond the clip's end), of the signals minus their means when ``zero_mean``.
    """
    lib = _sdr_check(preds, target, filter_length)
    L, N = int(filter_length), preds.shape[-1]
    p = preds.reshape(-1, N).float().contiguous()
    t = target.reshape(-1, N).float().contiguous()
    B = p.shape[0]
    if B < 1:
        raise ValueError('preds and target hold no clip')
    scratch = torch.empty(lib.tt_sdr_scratch_bytes(B, N, L) // 8, dtype=torch.float64, device=p.device)
    rb = torch.empty(B, 2 * L + 1, dtype=torch.float64, device=p.device)
    means = None
    with torch.cuda.device(p.device):
        st = _hip.stream_ptr()
        if zero_mean:
            means = torch.empty(B, 2, dtype=torch.float64, device=p.device)
            _hip.check(lib.tt_sdr_means(_hip.ptr(p), _hip.ptr(t), B, N, _hip.ptr(scratch), _hip.ptr(means), st), 'tt_sdr_means')
        _hip.check(lib.tt_sdr_correlate(_hip.ptr(p), _hip.ptr(t), B, N, L, _hip.ptr(means), _hip.ptr(scratch), _hip.ptr(rb), st),
                   'tt_sdr_correlate')
    return rb


def signal_distortion_ratio_device(preds, target, filter_length=512, zero_mean=False, load_diag=None):
    """
    ``signal_distortion_ratio`` for device tensors (..., N) of equal shape, computed where they are: a float64 device tensor
    of the leading shape, launched on the current stream without a host synchronisation (reference
    ``experiments/evaluate.py:51,122-127``).  fp16 / bf16 inputs are upcast to fp32; float64 raises ``ValueError`` (use the
    host function); CPU tensors raise ``RuntimeError`` -- there is no CPU fallback.  ``filter_length`` <= 512.

    Agreement with the host function: the correlations are direct float64 sums of exact products instead of FFTs, the solve
    is a Levinson recursion instead of a dense one; measured <= 5e-9 dB in float64 up to a Toeplitz condition number of 4e11.
    The one difference: an all-zero ``target`` gives a non-finite value here, where the host function raises ``LinAlgError``.
    """
    rb = sdr_correlations(preds, target, filter_length, zero_mean)
    B, L = rb.shape[0], int(filter_length)
    out = torch.empty(2, B, dtype=torch.float64, device=rb.device)
    with torch.cuda.device(rb.device):
        _hip.check(_hip.lib().tt_sdr_finish(_hip.ptr(rb), B, L, 0.0 if load_diag is None else float(load_diag), int(load_diag is not None),
                                            _hip.ptr(out[0]), _hip.ptr(out[1]), _hip.stream_ptr()), 'tt_sdr_finish')
    return out[1].reshape(preds.shape[:-1])


class SignalDistortionRatio(torch.nn.Module):
    """
    The call shape of ``torchmetrics.audio.SignalDistortionRatio`` as ``experiments/evaluate.py:51,122-127`` uses it:
    ``SignalDistortionRatio().to(device)``, then ``module(preds, target)`` -> the mean SDR over all clips of the batch as a
    0-dim tensor in ``preds``' dtype (``.item()`` is the caller's one host sync).  ``forward`` and ``update`` also add the
    batch to a running sum (float64, on the inputs' device) and count; ``compute`` is their ratio, ``reset`` clears them.
    """

    def __init__(self, filter_length=512, zero_mean=False, load_diag=None):
        super().__init__()
        self.filter_length, self.zero_mean, self.load_diag = filter_length, zero_mean, load_diag
        self.reset()

    def reset(self):
        self.sum_sdr, self.total = None, 0

    def _accumulate(self, preds, target):
        values = signal_distortion_ratio_device(preds, target, self.filter_length, self.zero_mean, self.load_diag)
        batch = values.sum()
        self.sum_sdr = batch if self.sum_sdr is None else self.sum_sdr + batch
        self.total += values.numel()
        return values

    def update(self, preds, target):
        self._accumulate(preds, target)

    def forward(self, preds, target):
        return self._accumulate(preds, target).mean().to(preds.dtype)

    def compute(self):
        if self.total == 0:
            raise RuntimeError('SignalDistortionRatio.compute() before any update()')
        return self.sum_sdr / self.total


# ---- note-level scores ------------------------------------------------------------------------------------------------------

NoteCounts = namedtuple('NoteCounts', ('n_ref', 'n_est', 'tp', 'tp_no_offset'))
NoteCounts.__doc__ = """The integers the note-level scores are formed from (``tp`` is None without the offset criterion)."""
DeviceNoteCounts = namedtuple('DeviceNoteCounts', ('n_ref', 'n_est', 'tp', 'tp_no_offset', 'n_fallback'))
DeviceNoteCounts.__doc__ = """``NoteCounts`` per batch item as int64 device tensors [B], and how many items were counted on the host."""

_NOTE_WINDOW_SLACK = 1e-4     # rnd(d) <= tol implies d <= tol + 0.5e-4: candidates are looked for this far beyond the onset tolerance


def _note_arrays(pitches, intervals, what):
    p = np.asarray(pitches, dtype=np.float64).ravel()
    iv = np.asarray(intervals, dtype=np.float64).reshape(-1, 2)
    if len(p) != len(iv):
        raise ValueError('%s pitches (%d) and intervals (%d) must hold one entry per note' % (what, len(p), len(iv)))
    return p, iv


def _note_pairs(ref_p, ref_iv, est_p, est_iv, onset_tolerance, pitch_tolerance, offset_ratio, offset_min_tolerance):
    """THE RULE.  -> (i, k, offset_ok): the onset pairs (reference i, estimate k), ascending in i, and which of them are offset pairs
    too (None without ``offset_ratio``).  Only pairs inside the widened onset window are looked at; no other can pass."""
    order = np.argsort(est_iv[:, 0], kind='stable')                       # NaN onsets last
    est_on = est_iv[order, 0]
    lo = np.searchsorted(est_on, ref_iv[:, 0] - (onset_tolerance + _NOTE_WINDOW_SLACK), side='left')
    hi = np.maximum(np.searchsorted(est_on, ref_iv[:, 0] + (onset_tolerance + _NOTE_WINDOW_SLACK), side='right'), lo)
    n = hi - lo
    i = np.repeat(np.arange(len(ref_p)), n)
    k = order[np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n) + np.repeat(lo, n)]
    with np.errstate(invalid='ignore'):                                   # inf - inf: a NaN, and a NaN makes every compare false
        onset_ok = (np.around(np.abs(ref_iv[i, 0] - est_iv[k, 0]), 4) <= onset_tolerance) & (np.abs(ref_p[i] - est_p[k]) <= pitch_tolerance)
        i, k = i[onset_ok], k[onset_ok]
        if offset_ratio is None:
            return i, k, None
        tolerance = np.maximum(offset_ratio * (ref_iv[i, 1] - ref_iv[i, 0]), offset_min_tolerance)
        return i, k, np.around(np.abs(ref_iv[i, 1] - est_iv[k, 1]), 4) <= tolerance


def _kuhn(n_ref, n_est, i, k):
    """Size of a maximum matching of the bipartite graph with edges (i[.], k[.]), ``i`` ascending: Kuhn's augmenting paths as in
    ``_max_matching``, with an explicit stack (a chain of notes may be thousands long)."""
    if len(i) == 0:
        return 0
    start = np.searchsorted(i, np.arange(n_ref + 1)).tolist()
    adj = k.tolist()
    match = [-1] * n_est
    count = 0
    for root in range(n_ref):
        if start[root] == start[root + 1]:
            continue
        seen = set()
        stack, chosen, pos = [root], [], {root: start[root]}
        while stack:
            r = stack[-1]
            at = pos[r]
            while at < start[r + 1] and adj[at] in seen:
                at += 1
            if at == start[r + 1]:                                        # r has no untried estimate left: back to its caller
                stack.pop()
                if chosen:
                    chosen.pop()
                continue
            e = adj[at]
            pos[r] = at + 1
            seen.add(e)
            chosen.append(e)
            if match[e] < 0:                                              # a free estimate: flip the path
                for rr, ee in zip(stack, chosen):
                    match[ee] = rr
                count += 1
                break
            stack.append(match[e])
            pos[match[e]] = start[match[e]]
    return count


def note_counts(ref_pitches, ref_intervals, est_pitches, est_intervals, onset_tolerance=0.05, pitch_tolerance=0.5, offset_ratio=0.2,
                offset_min_tolerance=0.05):
    """
    The integers behind ``note_metrics``: ``NoteCounts(n_ref, n_est, tp, tp_no_offset)``; ``tp`` is None when ``offset_ratio`` is None.
    """
    ref_p, ref_iv = _note_arrays(ref_pitches, ref_intervals, 'reference')
    est_p, est_iv = _note_arrays(est_pitches, est_intervals, 'estimated')
    n_ref, n_est = len(ref_p), len(est_p)
    if n_ref == 0 or n_est == 0:
        return NoteCounts(n_ref, n_est, None if offset_ratio is None else 0, 0)
    i, k, offset_ok = _note_pairs(ref_p, ref_iv, est_p, est_iv, onset_tolerance, pitch_tolerance, offset_ratio, offset_min_tolerance)
    tp = None if offset_ratio is None else _kuhn(n_ref, n_est, i[offset_ok], k[offset_ok])
    return NoteCounts(n_ref, n_est, tp, _kuhn(n_ref, n_est, i, k))


def _note_prf(tp, n_ref, n_est):
    """Precision, recall and F-measure from the integer counts, in float64."""
    tp, n_ref, n_est = np.float64(tp), np.float64(n_ref), np.float64(n_est)
    precision = tp / n_est if n_est > 0 else 0.0
    recall = tp / n_ref if n_ref > 0 else 0.0
    f_measure = 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
    return float(precision), float(recall), float(f_measure)


def _note_scores(counts):
    out = {}
    for suffix, tp in (('', counts.tp), ('_no_offset', counts.tp_no_offset)):
        if tp is not None:
            for key, v in zip(('Precision', 'Recall', 'F-measure'), _note_prf(tp, counts.n_ref, counts.n_est)):
                out[key + suffix] = v
    return out


def note_metrics(ref_pitches, ref_intervals, est_pitches, est_intervals, onset_tolerance=0.05, pitch_tolerance=0.5, offset_ratio=0.2,
                 offset_min_tolerance=0.05):
    """
    Note-level precision, recall and F-measure of estimated against reference notes, modelled on
    ``mir_eval.transcription.match_notes`` / ``precision_recall_f1_overlap`` AS RECALLED -- the package is not installed and there is
    no network, so PARITY IS UNPINNED against it; this function is the yardstick everything else in the package is compared with.

    Notes are (pitch, onset, offset) in float64: ``*_pitches`` (L) in MIDI numbers, ``*_intervals`` (L, 2) in seconds.  With
    ``rnd(x) = np.around(x, 4) = rint(x * 1e4) / 1e4``, reference note i and estimated note k are an ONSET PAIR when both

        rnd(|on_i - on_k|) <= onset_tolerance        and        |p_i - p_k| <= pitch_tolerance   (semitones)

    and additionally an OFFSET PAIR when ``rnd(|off_i - off_k|) <= max(offset_ratio * (off_i - on_i), offset_min_tolerance)``.  All
    compares are float64, and a NaN anywhere makes the compare false: such a note never matches but still counts.  ``tp_no_offset`` is
    the size of a maximum matching of the onset pairs, ``tp`` of the pairs that are both; precision = tp / n_est, recall = tp / n_ref
    (0 for a zero denominator), F-measure = 2 P R / (P + R) (0 when both are 0).

    Two deliberate differences from mir_eval.  Pitch is compared in MIDI numbers, not as 1200 |log2(f_i / f_k)| cents of Hz values: the
    device can then reproduce the verdict bit for bit, and the two forms differ only for pitches exactly at the tolerance.  The average
    overlap ratio is left out: it depends on WHICH maximum matching is chosen, and that is not unique.

    Returns ``Precision``, ``Recall``, ``F-measure`` and the same three with the suffix ``_no_offset``; ``offset_ratio=None`` returns
    only the latter.
    """
    return _note_scores(note_counts(ref_pitches, ref_intervals, est_pitches, est_intervals, onset_tolerance, pitch_tolerance, offset_ratio,
                                    offset_min_tolerance))


# ---- note-level scores on the device (csrc/notescore.hip) -------------------------------------------------------------------

NOTESCORE_MAX = 64        # references / estimates per connected component the matching kernel holds (= tt_notescore_max(), checked on first use)
NOTESCORE_ROUNDS = 32     # label-propagation rounds before an item that has not settled goes to the host


def _note_device_four(notes, what):
    if not (isinstance(notes, (tuple, list)) and len(notes) == 4 and all(isinstance(t, torch.Tensor) for t in notes)):
        raise RuntimeError('%s notes for scoring on the device are a NoteEvents or four GPU tensors (item int32, pitch, onset, offset '
                           'float64); the host function note_metrics takes arrays' % what)
    _hip.require_cuda(*notes)
    item, pitch, onset, offset = notes
    if item.dtype != torch.int32 or any(t.dtype != torch.float64 for t in (pitch, onset, offset)):
        raise ValueError('%s notes must be (item int32, pitch float64, onset float64, offset float64)' % what)
    if any(t.dim() != 1 or t.shape != item.shape or t.device != item.device for t in (item, pitch, onset, offset)):
        raise ValueError('%s notes must be four 1-d tensors of one length on one device' % what)
    return tuple(t.detach().contiguous() for t in notes)


def _note_event_times(events, hop_seconds):
    """Onset / offset seconds of a ``NoteEvents`` on the device, in the arithmetic of ``events_to_notes``."""
    if hop_seconds is None:
        raise ValueError('hop_seconds is required to place NoteEvents in time')
    _hip.require_cuda(events.item, events.onset, events.end, events.pitch)
    if isinstance(hop_seconds, (tuple, list)):
        hop_length, sample_rate = hop_seconds
        integral = isinstance(hop_length, (int, np.integer))
        hop_int, hop_mul, denom = (int(hop_length), 1.0, float(sample_rate)) if integral else (1, float(hop_length), float(sample_rate))
    else:
        hop_int, hop_mul, denom = 1, float(hop_seconds), 1.0
    n, dev = events.onset.numel(), events.onset.device
    onset = torch.empty(n, dtype=torch.float64, device=dev)
    offset = torch.empty_like(onset)
    on_f, end_f = events.onset.to(torch.int32).contiguous(), events.end.to(torch.int32).contiguous()
    if n:
        with torch.cuda.device(dev):
            _hip.check(_hip.lib().tt_notescore_times(_hip.ptr(on_f), _hip.ptr(end_f), n, hop_int, hop_mul, denom, _hip.ptr(onset),
                                                     _hip.ptr(offset), _hip.stream_ptr()), 'tt_notescore_times')
    return onset, offset


def _note_sorted(notes, n_items):
    """Notes ordered by (item, onset) -- torch's stable sort, NaN onsets last -- and the bounds of every item's run (int64 [B + 1])."""
    item, pitch, onset, offset = notes
    by_onset = torch.argsort(onset, stable=True)
    perm = by_onset[torch.argsort(item[by_onset], stable=True)]
    item = item[perm].contiguous()
    seg = torch.searchsorted(item, torch.arange(n_items + 1, dtype=torch.int32, device=item.device)).to(torch.int64)
    return (item, pitch[perm].contiguous(), onset[perm].contiguous(), offset[perm].contiguous()), seg


def _note_counts_device(est, ref, hop_seconds, n_items, onset_tolerance, pitch_tolerance, offset_ratio, offset_min_tolerance):
    """-> (DeviceNoteCounts, the same four counts as an int64 ndarray [B, 4])."""
    if isinstance(est, NoteEvents):
        est = (est.item, est.pitch) + _note_event_times(est, hop_seconds)
    est = _note_device_four(est, 'estimated')
    dev = est[0].device
    if isinstance(ref, (tuple, list)) and len(ref) == 4 and all(isinstance(t, torch.Tensor) for t in ref):
        ref = _note_device_four(ref, 'reference')
        if ref[0].device != dev:
            raise RuntimeError('estimated notes are on %s, reference notes on %s' % (dev, ref[0].device))
        if n_items is None:                                               # one value comes back
            n_items = int(torch.cat([ref[0].max().reshape(1) if ref[0].numel() else ref[0].new_zeros(1),
                                     est[0].max().reshape(1) if est[0].numel() else est[0].new_zeros(1)]).max()) + 1
    else:
        pairs = [_note_arrays(p, iv, 'reference') for p, iv in ref]
        if n_items is None:
            n_items = len(pairs)
        if len(pairs) > n_items:
            raise ValueError('%d reference note lists for %d items' % (len(pairs), n_items))
        sizes = [len(p) for p, _ in pairs]
        flat = np.empty((3, sum(sizes)))                                  # the one upload: pitch, onset, offset rows
        if sum(sizes):
            flat[0] = np.concatenate([p for p, _ in pairs])
            flat[1:] = np.concatenate([iv for _, iv in pairs]).T
        up = torch.from_numpy(flat).to(dev)
        item = torch.from_numpy(np.repeat(np.arange(len(pairs), dtype=np.int32), sizes)).to(dev)
        ref = (item, up[0], up[1], up[2])
    n_items = int(n_items)
    if n_items < 1:
        raise ValueError('n_items must be at least 1 (got %d)' % n_items)
    lib = _hip.lib()
    if lib.tt_notescore_max() != NOTESCORE_MAX:
        raise RuntimeError('libttrap_hip.so was built with a component capacity of %d, metrics.NOTESCORE_MAX says %d'
                           % (lib.tt_notescore_max(), NOTESCORE_MAX))
    ratio = 0.0 if offset_ratio is None else float(offset_ratio)
    (r_item, r_p, r_on, r_off), r_seg = _note_sorted(ref, n_items)
    (e_item, e_p, e_on, e_off), e_seg = _note_sorted(est, n_items)
    R, E, B = r_item.numel(), e_item.numel(), n_items
    if R + E >= 2 ** 31:
        raise ValueError('more than 2^31 notes')
    if R == 0 or E == 0:
        sums = torch.zeros(B, 5, dtype=torch.int64, device=dev)
        sums[:, 0], sums[:, 1] = r_seg[1:] - r_seg[:-1], e_seg[1:] - e_seg[:-1]
        host = sums.cpu().numpy()
    else:
        N = R + E
        lo, hi = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
        label, other = torch.arange(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
        changed = torch.zeros(NOTESCORE_ROUNDS, dtype=torch.int32, device=dev)
        item_mark = torch.zeros(B, dtype=torch.int32, device=dev)
        tp, tp_no = torch.empty(R, dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.int32, device=dev)
        sums = torch.empty(B, 5, dtype=torch.int64, device=dev)
        p = _hip.ptr
        with torch.cuda.device(dev):
            st = _hip.stream_ptr()
            _hip.check(lib.tt_notescore_ranges(p(r_item), p(r_on), R, p(e_item), p(e_on), E, p(r_seg), p(e_seg), B, float(onset_tolerance),
                                               p(lo), p(hi), st), 'tt_notescore_ranges')
            settled = False
            for rnd in range(NOTESCORE_ROUNDS):
                _hip.check(lib.tt_notescore_labels(p(r_item), p(r_p), p(r_on), R, p(e_item), p(e_p), p(e_on), E, p(lo), p(hi),
                                                   float(onset_tolerance), float(pitch_tolerance), p(label), p(other), p(changed[rnd:]),
                                                   p(item_mark), B, rnd + 1, st), 'tt_notescore_labels')
                label, other = other, label
                if not int(changed[rnd]):                                 # the one flag read per round
                    settled = True
                    break
            # an item whose labels still moved in the last round allowed is counted on the host
            item_flag = torch.zeros(B, dtype=torch.int32, device=dev) if settled else (item_mark == NOTESCORE_ROUNDS).to(torch.int32)
            r_lab, r_perm = torch.sort(label[:R], stable=True)
            e_lab, e_perm = torch.sort(label[R:], stable=True)
            r_perm, e_perm = r_perm.to(torch.int32), e_perm.to(torch.int32)
            _hip.check(lib.tt_notescore_match(p(label), p(r_lab), p(r_perm), p(e_lab), p(e_perm), p(r_item), p(r_p), p(r_on), p(r_off), R,
                                              p(e_p), p(e_on), p(e_off), E, float(onset_tolerance), float(pitch_tolerance), ratio,
                                              float(offset_min_tolerance), p(tp), p(tp_no), p(item_flag), B, st), 'tt_notescore_match')
            _hip.check(lib.tt_notescore_sums(p(tp), p(tp_no), R, E, p(r_seg), p(e_seg), p(item_flag), B, p(sums), st), 'tt_notescore_sums')
        host = sums.cpu().numpy()                                         # the one copy back: five integers per item
    flagged = np.flatnonzero(host[:, 4])
    if len(flagged):
        # over the kernel's capacity, or labels that did not settle: these items alone are counted by the host function from their own notes
        rs, es = r_seg.cpu().numpy(), e_seg.cpu().numpy()
        for b in flagged:
            r, e = slice(rs[b], rs[b + 1]), slice(es[b], es[b + 1])
            got = note_counts(r_p[r].cpu().numpy(), torch.stack([r_on[r], r_off[r]], 1).cpu().numpy(), e_p[e].cpu().numpy(),
                              torch.stack([e_on[e], e_off[e]], 1).cpu().numpy(), onset_tolerance, pitch_tolerance, offset_ratio,
                              offset_min_tolerance)
            host[b, 2], host[b, 3] = got.tp or 0, got.tp_no_offset
        sums = torch.from_numpy(host).to(dev)
    counts = DeviceNoteCounts(sums[:, 0], sums[:, 1], None if offset_ratio is None else sums[:, 2], sums[:, 3], len(flagged))
    return counts, host[:, :4]


def note_counts_device(est, ref, hop_seconds=None, n_items=None, onset_tolerance=0.05, pitch_tolerance=0.5, offset_ratio=0.2,
                       offset_min_tolerance=0.05):
    """
    ``note_counts`` per batch item for estimated notes that are on the device: ``DeviceNoteCounts`` of int64 device tensors [B]
    ``n_ref``, ``n_est``, ``tp`` (None when ``offset_ratio`` is None), ``tp_no_offset`` -- equal to the host function's integers -- and
    ``n_fallback``, the number of items that were counted by the host function instead.

    ``est``: a ``NoteEvents`` (then ``hop_seconds`` is required: seconds per frame or ``(hop_length, sample_rate)``, and the times are
    formed on the device in the arithmetic of ``events_to_notes``), or four device tensors ``(item int32, pitch float64 MIDI, onset
    float64 s, offset float64 s)`` in any order of notes.  ``ref``: a list over items of host ``(pitches, intervals)`` with pitches in
    MIDI numbers (uploaded once), or the same four device tensors (then ``n_items`` saves reading the largest item back).  Notes of an
    item outside [0, B) are ignored.  CPU tensors for ``est`` raise ``RuntimeError``: there is no CPU fallback.

    On the device: both lists sorted by (item, onset); per note the slice of the other list inside the onset window (binary search);
    connected components of the onset pairs by minimum-label propagation, one flag read per round; one wavefront per component for the
    two maximum matchings; integer sums per item; ONE copy of five integers per item back.  An item with a component of more than
    ``NOTESCORE_MAX`` references or estimates, or whose labels have not settled after ``NOTESCORE_ROUNDS`` rounds, is downloaded and
    counted by ``note_counts``.
    """
    return _note_counts_device(est, ref, hop_seconds, n_items, onset_tolerance, pitch_tolerance, offset_ratio, offset_min_tolerance)[0]


def note_metrics_device(est, ref, hop_seconds=None, n_items=None, onset_tolerance=0.05, pitch_tolerance=0.5, offset_ratio=0.2,
                        offset_min_tolerance=0.05):
    """The dictionary of ``note_metrics`` for every batch item (a list of B dicts), from ``note_counts_device``'s integers: the same
    float64 values, bit for bit."""
    host = _note_counts_device(est, ref, hop_seconds, n_items, onset_tolerance, pitch_tolerance, offset_ratio, offset_min_tolerance)[1]
    return [_note_scores(NoteCounts(int(n_ref), int(n_est), None if offset_ratio is None else int(tp), int(tp_no)))
            for n_ref, n_est, tp, tp_no in host]
