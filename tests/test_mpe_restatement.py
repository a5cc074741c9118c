"""
CPU-only: a NumPy restatement of the device multi-pitch scorer (csrc/mpe.hip) -- the compaction predicate, the bit-row adjacency,
the iterative augmenting-path search with an explicit stack and a ``seen`` mask, the integer sums -- held against the host functions
``multipitch_metrics`` / ``_max_matching`` for EQUALITY on the input set of tests/test_gpu_mpe.py, plus the host-side pieces of the
device route that need no GPU (the ``est_idx`` helper against ``resample_multipitch``, the scores formed from integer sums, the
per-bin MIDI table, argument checks).

Everything here is integers and float64 comparisons, so every assertion is ``==``.

``mpe_case`` / ``edge_cases`` / ``capacity_cases`` / ``host_route`` / ``tie_case`` are shared with tests/test_gpu_mpe.py; what they
return is cached and read-only.
"""

import functools

import numpy as np
import pytest
import torch

from oracle import postprocessing as opp
from timbre_trap.utils import metrics
from timbre_trap.utils.metrics import (MPE_MAX_EST, MPE_MAX_REF, _max_matching, frequencies_to_midi, midi_to_chroma, match_count,
                                       multipitch_metrics, resample_multipitch)
from timbre_trap.utils.targets import midi_to_hz

F, FV, T = 540, 472, 300
MIDI_FREQS = 16.76557586 + np.arange(F) / 5.0
MIDI_FREQS.setflags(write=False)
THRESHOLD = 0.5
DENSITIES = (0.003, 0.05, 0.3)
COMPACT_T = (1, 63, 64, 65, 300)
OFFSETS = (0.0, 0.5, -0.5, 0.1, 0.3, 12.0, -12.0, 11.5, 6.0)
N_REF_FRAMES, N_TIES = 257, 20


# ---- inputs -------------------------------------------------------------------------------------------------------------------

def frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def activations(density, n_frames=T, seed=0):
    """fp32 (F, n_frames): a floor below the threshold everywhere, values in [0.5, 1) at a fraction ``density`` of the positions --
    also in the rows >= FV, which the scorer has to read as zero."""
    rng = np.random.default_rng([seed, n_frames, int(density * 1000)])
    x = 0.45 * rng.random((F, n_frames))
    high = rng.random((F, n_frames)) < density
    x[high] = 0.5 + 0.5 * rng.random(int(high.sum()))
    return frozen(x.astype(np.float32))


@functools.lru_cache(maxsize=None)
def edge_activations():
    """The compaction's own edge cases in 8 frames: equal neighbours (no strict peak), peaks at f = 0 and at f = FV - 1 (the row
    above the latter is masked, however large), a value exactly at the threshold, one just below, a peak in a masked row."""
    x = np.zeros((F, 8), dtype=np.float32)
    x[10:13, 0] = 0.8                                    # a plateau: no bin of it is a strict peak
    x[20, 0], x[21, 0] = 0.7, 0.7
    x[0, 1], x[1, 1] = 0.9, 0.2                          # peak at the first row
    x[FV - 1, 2], x[FV, 2] = 0.6, 0.95                   # peak at the last valid row; its upper neighbour is masked
    x[100, 3] = np.float32(THRESHOLD)                    # exactly the threshold: in
    x[200, 3] = np.nextafter(np.float32(THRESHOLD), np.float32(0))      # one ulp below: out
    x[FV + 5, 4] = 0.9                                   # only a masked row is active: an empty frame
    x[0:FV:2, 5] = 0.75                                  # the most strict peaks FV rows can hold (236)
    x[30, 6], x[31, 6], x[32, 6] = 0.6, 0.9, 0.6         # threshold mode keeps all three, peak mode the middle one
    return frozen(x)


def masked(x, fv=FV):
    y = np.array(x, dtype=np.float64)
    if 0 < fv < y.shape[0]:
        y[fv:] = 0.0
    return y


def host_mask(x, t=THRESHOLD, peaks_only=True, fv=FV):
    """(F, T) 0/1: what peaks_above / threshold of the masked map give (oracle/postprocessing.py)."""
    y = masked(x, fv)
    return opp.threshold(opp.filter_non_peaks(y) if peaks_only else y, t)


def host_frames(x, t=THRESHOLD, peaks_only=True, fv=FV):
    """activations_to_multi_pitch of the masked map: per frame the active bins' frequencies in Hz."""
    m = host_mask(x, t, peaks_only, fv)
    return [midi_to_hz(MIDI_FREQS[np.nonzero(m[:, i])[0]]) for i in range(m.shape[1])]


def est_times(n_frames=T):
    return frozen(0.0123 + np.arange(n_frames) / 341.0)


def ref_times(est_time, n=N_REF_FRAMES, n_ties=N_TIES, seed=0):
    """An unrelated grid that starts before and ends after the estimates, plus ``n_ties`` times exactly half way between two
    estimate frames (formed like resample_multipitch forms its midpoints, so that they ARE ties)."""
    rng = np.random.default_rng([seed, 77])
    grid = np.linspace(est_time[0] - 0.05, est_time[-1] + 0.05, n - n_ties)
    half = est_time / 2.0
    mids = half[1:] + half[:-1]
    ties = mids[rng.choice(len(mids), size=n_ties, replace=False)] if len(mids) >= n_ties else mids[:0]
    return frozen(np.sort(np.concatenate([grid, ties])))


@functools.lru_cache(maxsize=None)
def mpe_case(density, jitter=False, seed=0):
    """One track: activations (F, T) fp32, est_time, ref_time (257 frames), ref_freqs (0-6 pitches per frame)."""
    x = activations(density, T, seed)
    est_time = est_times()
    ref_time = ref_times(est_time, seed=seed)
    rng = np.random.default_rng([seed, int(density * 1000), int(jitter)])
    mask = host_mask(x)
    read = metrics._nearest_frame_index(est_time, ref_time, T)
    ref_freqs = []
    for i in read:
        active = np.nonzero(mask[:, i])[0] if i < T else np.empty(0, dtype=np.int64)
        n = int(rng.integers(0, 7))
        near = rng.random(n) < 0.7                                   # most pitches sit next to an estimate, the rest anywhere
        bins = np.where(near & (active.size > 0), rng.choice(active, size=n) if active.size else 0, rng.integers(0, FV, size=n))
        off = rng.normal(0.0, 0.3, size=n) if jitter else rng.choice(OFFSETS, size=n)
        ref_freqs.append(frozen(np.clip(midi_to_hz(MIDI_FREQS[bins] + off), metrics.MIN_FREQ, metrics.MAX_FREQ)))
    return dict(key=('track', density, jitter, seed), x=x, est_time=est_time, ref_time=ref_time, ref_freqs=tuple(ref_freqs), t=THRESHOLD,
                peaks_only=True, window=0.5)


CASES = tuple((d, j) for d in DENSITIES for j in (False, True))


@functools.lru_cache(maxsize=None)
def edge_cases():
    base = mpe_case(0.05)
    empty = tuple(np.empty(0) for _ in base['ref_time'])
    one = activations(0.05, 1, seed=3)
    dup = tuple(frozen(np.repeat(f[:2], 2)) for f in base['ref_freqs'])            # every pitch twice: duplicates in a frame
    cases = {
        'empty_estimates': dict(base, x=frozen(np.zeros((F, T), dtype=np.float32))),
        'empty_references': dict(base, ref_freqs=empty),
        'no_overlap': dict(base, ref_time=frozen(base['ref_time'] + 100.0)),
        'one_frame_each': dict(base, x=one, est_time=est_times(1), ref_time=frozen(est_times(1) + 0.0), ref_freqs=(base['ref_freqs'][5],)),
        'one_estimate_frame': dict(base, x=one, est_time=est_times(1)),
        'duplicates': dict(base, ref_freqs=dup),
        'window_0.25': dict(base, window=0.25),
        'window_1.0': dict(mpe_case(0.3, True), window=1.0),
    }
    return {name: dict(case, key=name) for name, case in cases.items()}


@functools.lru_cache(maxsize=None)
def capacity_cases():
    """'ref': three frames of MPE_MAX_REF + 1 pitches (one of them reads an empty estimate frame -- still over the capacity).
    'est': threshold mode on a map where every 37th frame holds more than MPE_MAX_EST bins at or above the threshold."""
    base = mpe_case(0.05)
    rng = np.random.default_rng(5)
    many = frozen(np.sort(midi_to_hz(rng.uniform(MIDI_FREQS[0] + 1, MIDI_FREQS[FV - 1] - 1, size=MPE_MAX_REF + 1))))
    refs = list(base['ref_freqs'])
    for j in (0, 100, 200):                                         # frame 0 lies before the first estimate
        refs[j] = many
    x = np.array(activations(0.05))
    for k, c in enumerate(range(3, T, 37)):
        x[:MPE_MAX_EST + 1 + 10 * k, c] = 0.6 + 0.3 * rng.random(MPE_MAX_EST + 1 + 10 * k).astype(np.float32)
    return {'ref': dict(base, key='capacity_ref', ref_freqs=tuple(refs)),
            'est': dict(base, key='capacity_est', x=frozen(x), peaks_only=False)}


@functools.lru_cache(maxsize=None)
def tie_case():
    """A reference pitch as good as exactly ``window`` away from a bin whose MIDI number, as the host route sees it (bin -> Hz ->
    MIDI), differs from ``midi_freqs`` in the last bits, chosen so that ``<= 0.5`` comes out differently for the two values; the
    map holds that one bin only (its neighbours, 0.2 semitones away, would match anyway)."""
    est_midi, _ = metrics._mpe_bin_tables(MIDI_FREQS)
    for k in np.nonzero(est_midi[:FV] != MIDI_FREQS[:FV])[0]:
        for sign in (0.5, -0.5):
            hz = midi_to_hz(MIDI_FREQS[k] + sign)
            candidates = [hz]
            for toward in (0.0, np.inf):                                   # a few representable frequencies either side
                h = hz
                for _ in range(4):
                    h = np.nextafter(h, toward)
                    candidates.append(h)
            for hz in candidates:
                r = frequencies_to_midi([np.array([hz])])[0][0]
                if metrics.MIN_FREQ <= hz <= metrics.MAX_FREQ and (abs(r - est_midi[k]) <= 0.5) != (abs(r - MIDI_FREQS[k]) <= 0.5):
                    x = np.zeros((F, 3), dtype=np.float32)
                    x[k, 1] = 0.9
                    et = est_times(3)
                    return dict(key='tie', x=frozen(x), est_time=et, ref_time=frozen(et[1:2] + 0.0), ref_freqs=(frozen(np.array([hz])),),
                                t=THRESHOLD, peaks_only=True, window=0.5, bin=int(k), midi_freqs_says=bool(abs(r - MIDI_FREQS[k]) <= 0.5))
    return None


def host_route(case):
    """The host route on one case, once: (tp, tp_chroma, n_ref, n_est per reference frame as int64, the fourteen scores)."""
    key = case['key']
    if key not in _ROUTES:
        est = host_frames(case['x'], case['t'], case['peaks_only'])
        scores = multipitch_metrics(case['ref_time'], case['ref_freqs'], case['est_time'], est, window=case['window'])
        res = resample_multipitch(case['est_time'], est, case['ref_time'])
        rm, em = frequencies_to_midi(case['ref_freqs']), frequencies_to_midi(res)
        tp = match_count(rm, em, case['window'], False).astype(np.int64)
        tpc = match_count(midi_to_chroma(rm), midi_to_chroma(em), case['window'], True).astype(np.int64)
        n_ref, n_est = np.array([len(f) for f in rm], dtype=np.int64), np.array([len(f) for f in em], dtype=np.int64)
        _ROUTES[key] = tuple(frozen(a) for a in (tp, tpc, n_ref, n_est)), scores
    return _ROUTES[key]


_ROUTES = {}


# ---- the restatement ----------------------------------------------------------------------------------------------------------

def restated_compact(x, t, peaks_only, fv):
    """k_mpe_compact: per frame the rows that pass k_peak_pick's predicate, ascending, as CSR (offsets int64, bins int32)."""
    x = np.asarray(x, dtype=np.float32)
    n_bins, n_frames = x.shape
    fv = fv if 0 < fv < n_bins else n_bins
    v = x[:fv]
    zero = np.zeros((1, n_frames), dtype=np.float32)
    up, dn = np.concatenate([zero, v[:-1]]), np.concatenate([v[1:], zero])
    peak = (v > up) & (v > dn) if peaks_only else np.ones_like(v, dtype=bool)
    active = np.zeros((n_bins, n_frames), dtype=bool)
    active[:fv] = peak & (v.astype(np.float64) >= t)
    if not peaks_only and 0.0 >= t:
        active[fv:] = True
    frames, bins = np.nonzero(active.T)                                # frame-major, bins ascending within a frame
    off = np.zeros(n_frames + 1, dtype=np.int64)
    np.cumsum(np.bincount(frames, minlength=n_frames), out=off[1:])
    return off, bins.astype(np.int32)


def restated_adjacency(r, e, window):
    """The bit rows of k_mpe_match as Python ints (bit i of row k: estimate i is admissible for reference k), plain and chroma."""
    rc, ec = np.fmod(r, 12.0), np.fmod(e, 12.0)
    plain, chroma = [], []
    for k in range(len(r)):
        d = np.fmod(np.abs(rc[k] - ec), 12.0)
        d2 = 12.0 - d
        plain.append(sum(1 << int(i) for i in np.nonzero(np.abs(r[k] - e) <= window)[0]))
        chroma.append(sum(1 << int(i) for i in np.nonzero(np.where(d < d2, d, d2) <= window)[0]))
    return plain, chroma


def restated_search(rows, n_est):
    """Kuhn's augmenting paths without recursion: a stack of (reference, chosen estimate) and a ``seen`` mask per root."""
    match = [-1] * n_est
    count = deepest = 0
    for root in range(len(rows)):
        seen, stk_r, stk_e = 0, [root], [None]
        while stk_r:
            m = rows[stk_r[-1]] & ~seen
            if not m:
                stk_r.pop()
                stk_e.pop()
                continue
            e = (m & -m).bit_length() - 1                              # lowest set bit, like __ffsll
            seen |= 1 << e
            stk_e[-1] = e
            if match[e] < 0:
                for rr, ee in zip(stk_r, stk_e):
                    match[ee] = rr
                count += 1
                break
            stk_r.append(match[e])
            stk_e.append(None)
            deepest = max(deepest, len(stk_r))
    assert deepest <= max(len(rows), 1)                                # the kernel's stack holds MPE_MAX_REF entries
    return count


def restated_counts(case):
    """The device route in NumPy: (tp, tp_chroma, n_ref, n_est) int64 per reference frame, tp = -1 where a capacity is exceeded."""
    off, bins = restated_compact(case['x'], case['t'], case['peaks_only'], FV)
    n_frames = case['x'].shape[1]
    est_midi, _ = metrics._mpe_bin_tables(MIDI_FREQS)
    idx = metrics._nearest_frame_index(case['est_time'], case['ref_time'], n_frames)
    out = np.zeros((4, len(idx)), dtype=np.int64)
    for j, i in enumerate(idx):
        r = frequencies_to_midi([np.asarray(case['ref_freqs'][j], dtype=np.float64)])[0]
        e = est_midi[bins[off[i]:off[i + 1]]] if i < n_frames else np.empty(0)
        out[2, j] = len(r)
        if len(r) > MPE_MAX_REF or len(e) > MPE_MAX_EST:
            out[0, j] = -1
            continue
        out[3, j] = len(e)
        if len(r) and len(e):
            plain, chroma = restated_adjacency(r, e, case['window'])
            out[0, j], out[1, j] = restated_search(plain, len(e)), restated_search(chroma, len(e))
    return out


def restated_sums(tp, tpc, n_ref, n_est):
    return [int(v) for v in (tp.sum(), tpc.sum(), n_ref.sum(), n_est.sum(), np.minimum(n_ref, n_est).sum(), np.maximum(n_ref, n_est).sum(),
                             np.maximum(n_ref - n_est, 0).sum(), np.maximum(n_est - n_ref, 0).sum())]


def over_capacity(case):
    """Reference frames the kernel flags: more than MPE_MAX_REF reference pitches or more than MPE_MAX_EST estimates."""
    (_, _, n_ref, _), _ = host_route(case)
    n_act = host_mask(case['x'], case['t'], case['peaks_only']).sum(axis=0).astype(np.int64)
    idx = metrics._nearest_frame_index(case['est_time'], case['ref_time'], case['x'].shape[1])
    n_est = np.concatenate([n_act, [0]])[idx]
    return int(((n_ref > MPE_MAX_REF) | (n_est > MPE_MAX_EST)).sum())


# ---- tests --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('peaks_only', (True, False))
@pytest.mark.parametrize('n_frames', COMPACT_T)
def test_compaction_restated(n_frames, peaks_only):
    x = activations(0.3, n_frames, seed=1)
    off, bins = restated_compact(x, THRESHOLD, peaks_only, FV)
    want_b, want_t = np.nonzero(host_mask(x, THRESHOLD, peaks_only))
    order = np.lexsort((want_b, want_t))
    assert np.array_equal(bins, want_b[order])
    assert np.array_equal(np.diff(off), np.bincount(want_t, minlength=n_frames))


@pytest.mark.parametrize('peaks_only', (True, False))
def test_compaction_edges_restated(peaks_only):
    x = edge_activations()
    off, bins = restated_compact(x, THRESHOLD, peaks_only, FV)
    got = [list(bins[off[i]:off[i + 1]]) for i in range(x.shape[1])]
    m = host_mask(x, THRESHOLD, peaks_only)
    assert got == [list(np.nonzero(m[:, i])[0]) for i in range(x.shape[1])]
    if peaks_only:
        assert got[0] == [] and got[1] == [0] and got[2] == [FV - 1] and got[3] == [100] and got[4] == []
        assert len(got[5]) == FV // 2 == 236 <= MPE_MAX_EST and got[6] == [31]
    else:
        assert got[0] == [10, 11, 12, 20, 21] and got[6] == [30, 31, 32]


def test_frame_index_helper_is_resample_multipitch():
    rng = np.random.default_rng(0)
    for n in (1, 2, 7, 300):
        times = est_times(n)
        frames = [np.array([float(i)]) for i in range(n)]
        half = times / 2.0
        targets = np.concatenate([rng.uniform(times[0] - 0.01, times[-1] + 0.01, 200), times, half[1:] + half[:-1],
                                  [times[0], times[-1], np.nextafter(times[0], -1), np.nextafter(times[-1], 9)]])
        idx = metrics._nearest_frame_index(times, targets, n)
        res = resample_multipitch(times, frames, targets)
        assert [list(f) for f in res] == [[float(i)] if i < n else [] for i in idx]
        assert idx[-2] == n and idx[-1] == n and idx[-4] == 0 and idx[-3] == n - 1
    c = mpe_case(0.05)
    idx = metrics._nearest_frame_index(c['est_time'], c['ref_time'], T)
    assert (idx == T).sum() > 10 and idx[0] == T and idx[-1] == T           # the reference grid overhangs both ends
    half = c['est_time'] / 2.0
    ties = np.isin(c['ref_time'], half[1:] + half[:-1])
    assert ties.sum() >= N_TIES
    assert np.array_equal(idx[ties], np.searchsorted(half[1:] + half[:-1], c['ref_time'][ties]))      # the earlier frame


@pytest.mark.parametrize('density,jitter', CASES)
def test_counts_and_scores_restated(density, jitter):
    case = mpe_case(density, jitter)
    (tp, tpc, n_ref, n_est), scores = host_route(case)
    got = restated_counts(case)
    assert np.array_equal(got[0], tp) and np.array_equal(got[1], tpc)
    assert np.array_equal(got[2], n_ref) and np.array_equal(got[3], n_est)
    assert metrics._scores_from_sums(restated_sums(*got)) == scores
    assert n_ref.max() <= 6 and tp.sum() > 0
    if density == 0.3:
        assert 90 <= n_est.max() <= MPE_MAX_EST
        assert jitter or (tpc > tp).any()                                  # octave offsets: the chroma matching finds more


@pytest.mark.parametrize('name', sorted(edge_cases()))
def test_edges_restated(name):
    case = edge_cases()[name]
    (tp, tpc, n_ref, n_est), scores = host_route(case)
    got = restated_counts(case)
    assert [list(g) for g in got] == [list(tp), list(tpc), list(n_ref), list(n_est)]
    assert metrics._scores_from_sums(restated_sums(*got)) == scores
    if name in ('empty_estimates', 'empty_references', 'no_overlap'):
        assert tp.sum() == 0
    if name == 'duplicates':
        assert (tp < n_ref).any() and tp.sum() > 0


def test_search_restated_on_dense_frames():
    """Frames up to the capacities, with long augmenting paths: the iterative search against the recursive one."""
    rng = np.random.default_rng(11)
    for n_r, n_e, spread in ((MPE_MAX_REF, MPE_MAX_EST, 20.0), (MPE_MAX_REF, 40, 6.0), (30, 30, 3.0), (MPE_MAX_REF, MPE_MAX_REF, 8.0)):
        r = np.sort(40.0 + spread * rng.random(n_r))
        e = np.sort(40.0 + spread * rng.random(n_e))
        for window in (0.25, 0.5, 1.0):
            plain, chroma = restated_adjacency(r, e, window)
            assert restated_search(plain, n_e) == _max_matching(r, e, window, False)
            assert restated_search(chroma, n_e) == _max_matching(np.mod(r, 12), np.mod(e, 12), window, True)
    # a chain in which every root displaces all earlier matches: reference k may take estimates k and k + 1 only, roots in reverse
    n = MPE_MAX_REF
    rows = [(1 << k) | (1 << (k + 1)) for k in range(n - 1, -1, -1)]
    assert restated_search(rows, n + 1) == n


def test_gpu_inputs_stay_within_capacities():
    for density, jitter in CASES:
        assert over_capacity(mpe_case(density, jitter)) == 0
    for case in edge_cases().values():
        assert over_capacity(case) == 0
    assert over_capacity(tie_case()) == 0
    caps = capacity_cases()
    assert over_capacity(caps['ref']) == 3
    assert over_capacity(caps['est']) >= 4
    got = restated_counts(caps['ref'])
    assert (got[0] == -1).sum() == 3


def test_scores_from_integer_sums_are_the_host_scores():
    for case in [mpe_case(d, j) for d, j in CASES] + list(capacity_cases().values()):
        counts, scores = host_route(case)
        assert metrics._scores_from_sums(restated_sums(*counts)) == scores
    zero = metrics._scores_from_sums([0] * 8)
    assert zero == multipitch_metrics([], [], [], []) and len(zero) == 14


def test_bin_table_is_the_host_round_trip():
    est_midi, bad = metrics._mpe_bin_tables(MIDI_FREQS)
    differs = est_midi != MIDI_FREQS
    assert 0 < differs.sum() < F and np.abs(est_midi - MIDI_FREQS).max() < 1e-13
    assert not bad[:FV].any() and bad[FV:].all()                           # 472 of 540 bins lie below 5 kHz
    tie = tie_case()
    assert tie is not None, 'no bin where the round trip decides a <= 0.5 tie differently'
    (tp, _, _, _), _ = host_route(tie)
    assert list(tp) == [0 if tie['midi_freqs_says'] else 1]                # the host route disagrees with raw midi_freqs here
    assert list(restated_counts(tie)[0]) == list(tp)


def test_device_route_refuses_what_it_cannot_take():
    from timbre_trap.utils import multipitch_counts_device, multipitch_metrics_device, MultipitchEvaluator
    c = mpe_case(0.003)
    x = torch.from_numpy(np.array(c['x']))
    for fn in (multipitch_counts_device, multipitch_metrics_device):
        with pytest.raises(RuntimeError):                                  # a CPU tensor: no fallback
            fn(c['ref_time'], c['ref_freqs'], c['est_time'], x, MIDI_FREQS)
        with pytest.raises(RuntimeError):
            fn(c['ref_time'], c['ref_freqs'], c['est_time'], np.array(c['x']), MIDI_FREQS)
    with pytest.raises(RuntimeError):
        MultipitchEvaluator().evaluate_activations(c['est_time'], x, MIDI_FREQS, c['ref_time'], c['ref_freqs'])
    assert metrics.MPE_MAX_EST >= 236 and metrics.MPE_MAX_REF == 64
