"""
The host yardstick for the frame-level multi-pitch scores: NumPy only, float64, as in the reference (NumPy lists).

The reference delegates them to ``mir_eval.multipitch.evaluate(ref_time, ref_freqs, est_time, est_freqs, window=0.5)``, called from
``timbre_trap/utils/experiments.py:376-378``; the package is absent from this image.  ``multipitch_metrics`` restates its published
algorithm (mir_eval's multipitch module after Poliner & Ellis 2007 / Bay et al. 2009).  PARITY UNPINNED against the package itself (it
is not installed and there is no network); pinned instead by known-answer tests (tests/test_metrics.py) and a brute-force matcher.
``_scores_from_sums`` forms the same scores from eight integer sums: the device route (``mpe.py``) counts, this module divides.
"""

import numpy as np

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


# the integer sums the fourteen scores are formed from, in the order of the one int64 tensor that comes back per track (mpe.py)
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
