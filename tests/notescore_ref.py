"""
Case generators for the note-level score (timbre_trap.utils.note_counts and its device route), shared by
tests/test_notescore_restatement.py (CPU) and tests/test_gpu_notescore.py.  Fixed seeds; every case is
``(ref_pitches, ref_intervals, est_pitches, est_intervals)`` in float64, pitches in MIDI numbers, times in seconds.

``dense_hits`` writes the rule of ``note_metrics`` a second time, as dense matrices in plain NumPy expressions, and
``dense_counts`` hands them to scipy's maximum bipartite matching: an independent route to the same integers.
"""

import functools

import numpy as np

TOL = dict(onset_tolerance=0.05, pitch_tolerance=0.5, offset_ratio=0.2, offset_min_tolerance=0.05)

# (reference notes, track length in seconds): 20, 100 and 333 notes per second, and sizes around nothing at all
RANDOM_SIZES = ((1, 1.0), (7, 2.0), (100, 5.0), (300, 3.0), (1000, 3.0), (1500, 75.0), (1500, 15.0), (1500, 4.5))


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def random_notes(n_ref, length, seed=0, jitter=0.03, extra=0.3, missing=0.2):
    """Uniform onsets, integer reference pitches; the estimate drops ``missing`` of the notes, moves the onsets of the rest by about
    ``jitter`` seconds (normal), detunes them a little, and adds ``extra`` notes of its own; its order is shuffled."""
    rng = np.random.default_rng([seed, n_ref, 23])
    on = np.sort(rng.uniform(0.0, length, n_ref))
    dur = rng.uniform(0.05, 1.0, n_ref)
    ref_p = rng.integers(36, 96, n_ref).astype(np.float64)
    ref_iv = np.stack([on, on + dur], axis=1)
    keep = rng.random(n_ref) >= missing
    m, n_extra = int(keep.sum()), int(round(extra * n_ref))
    est_p = np.concatenate([ref_p[keep] + rng.normal(0.0, 0.25, m), rng.integers(36, 96, n_extra).astype(np.float64)])
    x_on = rng.uniform(0.0, length, n_extra)
    est_on = np.concatenate([on[keep] + rng.normal(0.0, jitter, m), x_on])
    est_off = np.concatenate([ref_iv[keep, 1] + rng.normal(0.0, 0.06, m), x_on + rng.uniform(0.05, 1.0, n_extra)])
    order = rng.permutation(len(est_p))
    return _ro(ref_p, ref_iv, est_p[order].copy(), np.stack([est_on, est_off], axis=1)[order].copy())


def random_cases():
    return {'n%d_len%g' % size: random_notes(*size) for size in RANDOM_SIZES}


def notes(rows):
    """[(pitch, onset, offset), ...] -> (pitches, intervals)."""
    a = np.array(rows, dtype=np.float64).reshape(-1, 3)
    return a[:, 0].copy(), a[:, 1:].copy()


def ladder(n):
    """A path r0 - e0 - r1 - e1 - ... - r(n-1) - e(n-1) of 2 n - 1 onset pairs, built from pitches 0.4 apart at (almost) one onset.
    By onset the references run from r(n-1) down to r0 and the estimates from e0 up, so a search that takes roots and candidates in
    onset order matches r(i) with e(i-1) for every i >= 1 and then has to flip all of it along one path of 2 n - 1 edges for r0."""
    ref = [(60.0 + 0.8 * i, 1.0 + 0.001 * (n - 1 - i), 2.0) for i in range(n)]
    est = [(60.4 + 0.8 * j, 1.0 + 0.001 * j, 2.0) for j in range(n)]
    return notes(ref) + notes(est)


def chain(n_nodes):
    """One pitch, references and estimates alternating 40 ms apart: a path of n_nodes - 1 onset pairs in one component."""
    t = 0.04 * np.arange(n_nodes)
    rows = [(60.0, x, x + 0.5) for x in t]
    return notes(rows[0::2]) + notes(rows[1::2])


def clique(n_ref, n_est):
    """Every reference pairs with every estimate by onset; by offset only with two estimates out of three."""
    ref = [(60.0, 1.0 + 0.0002 * i, 2.0 + 0.0002 * i) for i in range(n_ref)]
    est = [(60.0, 1.0 + 0.0002 * k, 2.0 + 0.0002 * k + 0.15 * (k % 3)) for k in range(n_est)]
    return notes(ref) + notes(est)


def crafted():
    """name -> (case, (tp, tp_no_offset)): small cases with the literal answer."""
    nan = float('nan')
    ref_p, ref_iv, _, _ = random_notes(100, 5.0)
    c = {}
    c['perfect_copy'] = ((ref_p, ref_iv, ref_p, ref_iv), (100, 100))
    c['no_overlap'] = ((ref_p, ref_iv, ref_p, ref_iv + 10.0), (0, 0))
    c['empty_ref'] = (notes([]) + (ref_p, ref_iv), (0, 0))
    c['empty_est'] = ((ref_p, ref_iv) + notes([]), (0, 0))
    c['both_empty'] = (notes([]) + notes([]), (0, 0))
    # an onset distance that rounds to 0.0500 hits, one that rounds to 0.0501 misses (pitches far apart keep the pairs one to one)
    c['onset_boundary'] = (notes([(40, 0.0, 1.0), (50, 0.0, 1.0), (60, 0.0, 1.0), (70, 0.0, 1.0)])
                           + notes([(40, 0.05004, 1.0), (50, 0.05006, 1.0), (60, -0.05004, 1.0), (70, -0.05006, 1.0)]), (2, 2))
    c['pitch_boundary'] = (notes([(60, 0.0, 1.0), (70, 0.0, 1.0), (80, 0.0, 1.0)])
                           + notes([(60.5, 0.0, 1.0), (69.5, 0.0, 1.0), (80.50001, 0.0, 1.0)]), (2, 2))
    # a reference of 0.25 s: 0.2 * 0.25 meets the floor of 0.05; one of 0.3 s has 0.06; one of 0.1 s keeps the floor
    c['offset_boundary'] = (notes([(40, 0.0, 0.25), (50, 0.0, 0.25), (60, 0.0, 0.3), (70, 0.0, 0.3), (80, 0.0, 0.1), (90, 0.0, 0.1)])
                            + notes([(40, 0.0, 0.30004), (50, 0.0, 0.30006), (60, 0.0, 0.355), (70, 0.0, 0.365), (80, 0.0, 0.13), (90, 0.0, 0.16)]),
                            (3, 6))
    # r1 - e1, r1 - e2, r2 - e1: matching r1 with e1 first leaves r2 alone; the answer is 2
    c['greedy_trap'] = (notes([(60.0, 0.0, 1.0), (60.8, 0.02, 1.0)]) + notes([(60.4, -0.01, 1.0), (59.6, 0.01, 1.0)]), (2, 2))
    c['path_5_edges'] = (ladder(3), (3, 3))
    c['path_9_edges'] = (ladder(5), (5, 5))
    # onset pairs: all four; offset pairs: r1 - e2 and r2 - e1 only, while a search in order matches r1 - e1, r2 - e2 by onset
    c['offset_not_a_subset'] = (notes([(60, 0.0, 1.0), (60, 0.001, 2.001)]) + notes([(60, 0.0, 2.0), (60, 0.001, 1.001)]), (2, 2))
    c['nan_pitch'] = (notes([(60, 0.0, 1.0), (62, 0.5, 1.0)]) + notes([(nan, 0.0, 1.0), (60, 0.01, 1.0), (62, 0.5, 1.0)]), (2, 2))
    c['nan_times'] = (notes([(60, 0.0, 1.0), (62, nan, 1.0), (64, 1.0, nan), (66, 2.0, 3.0)])
                      + notes([(60, nan, 1.0), (62, 0.5, 1.0), (64, 1.0, 2.0), (66, 2.0, nan), (60, 0.0, 1.0)]), (1, 3))
    c['inf_times'] = (notes([(60, np.inf, np.inf), (62, 0.0, np.inf)]) + notes([(60, np.inf, np.inf), (62, 0.0, np.inf)]), (0, 1))
    c['chain_60'] = (chain(60), (30, 30))
    c['clique_8x8'] = (clique(8, 8), (6, 8))
    return c


def dense_hits(ref_p, ref_iv, est_p, est_iv, onset_tolerance=0.05, pitch_tolerance=0.5, offset_ratio=0.2, offset_min_tolerance=0.05):
    """(onset pairs, onset-and-offset pairs) as dense boolean n_ref x n_est matrices."""
    with np.errstate(invalid='ignore'):
        onset = np.around(np.abs(np.subtract.outer(ref_iv[:, 0], est_iv[:, 0])), 4) <= onset_tolerance
        pitch = np.abs(np.subtract.outer(ref_p, est_p)) <= pitch_tolerance
        tol = np.maximum(offset_ratio * (ref_iv[:, 1] - ref_iv[:, 0]), offset_min_tolerance)
        offset = np.around(np.abs(np.subtract.outer(ref_iv[:, 1], est_iv[:, 1])), 4) <= tol[:, None]
    return onset & pitch, onset & pitch & offset


def dense_counts(case, **tolerances):
    """(tp, tp_no_offset) through scipy.sparse.csgraph.maximum_bipartite_matching."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_bipartite_matching
    if len(case[0]) == 0 or len(case[2]) == 0:
        return 0, 0
    on, both = dense_hits(*case, **tolerances)
    size = lambda hit: int((maximum_bipartite_matching(csr_matrix(hit), perm_type='column') >= 0).sum())          # noqa: E731
    return size(both), size(on)


def largest_component(case, onset_tolerance=0.05, pitch_tolerance=0.5):
    """(references, estimates) of the connected component of the onset-pair graph with the most of either."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n_ref, n_est = len(case[0]), len(case[2])
    if n_ref == 0 or n_est == 0:
        return 0, 0
    i, k = np.nonzero(dense_hits(*case, onset_tolerance=onset_tolerance, pitch_tolerance=pitch_tolerance)[0])
    n = n_ref + n_est
    _, lab = connected_components(coo_matrix((np.ones(len(i)), (i, n_ref + k)), shape=(n, n)), directed=False)
    return int(np.bincount(lab[:n_ref]).max()), int(np.bincount(lab[n_ref:], minlength=1).max())
