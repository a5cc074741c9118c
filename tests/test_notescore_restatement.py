"""
CPU-only: the note-level score of timbre_trap.utils.metrics.notescore (note_counts / note_metrics -- a restatement of
mir_eval.transcription's matching, unpinned against the package) against an independent route: the rule written a second time as
dense hit matrices (tests/notescore_ref.py: dense_hits) and scipy's maximum bipartite matching; known answers; the boundaries of the
three tolerances; and the component sizes of the generated cases, which keep tests/test_gpu_notescore.py honest about its fallback.
"""

import warnings

import numpy as np
import pytest

from timbre_trap.utils import NoteCounts, note_counts, note_metrics

from notescore_ref import RANDOM_SIZES, TOL, chain, clique, crafted, dense_counts, largest_component, notes, random_cases, random_notes

KEYS = ('Precision', 'Recall', 'F-measure')


@pytest.mark.parametrize('name', sorted(random_cases()))
def test_random_cases_against_scipy_on_dense_matrices(name):
    case = random_cases()[name]
    got = note_counts(*case)
    assert isinstance(got, NoteCounts) and (got.n_ref, got.n_est) == (len(case[0]), len(case[2]))
    assert (got.tp, got.tp_no_offset) == dense_counts(case)
    assert got.tp <= got.tp_no_offset <= min(got.n_ref, got.n_est)
    if got.n_ref >= 100:
        assert 0 < got.tp < got.tp_no_offset < got.n_ref                 # the generator leaves something to find and something to miss
    # other tolerances move both routes alike
    tol = dict(onset_tolerance=0.02, pitch_tolerance=0.25, offset_ratio=0.1, offset_min_tolerance=0.02)
    wide = note_counts(*case, **tol)
    assert (wide.tp, wide.tp_no_offset) == dense_counts(case, **tol)


@pytest.mark.parametrize('name', sorted(crafted()))
def test_crafted_cases_have_the_literal_answer(name):
    case, want = crafted()[name]
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        got = note_counts(*case)
        scores = note_metrics(*case)
    assert (got.tp, got.tp_no_offset) == want == dense_counts(case)
    assert (got.n_ref, got.n_est) == (len(case[0]), len(case[2]))
    assert sorted(scores) == sorted([k + s for k in KEYS for s in ('', '_no_offset')])
    assert all(isinstance(v, float) and 0.0 <= v <= 1.0 for v in scores.values())


def test_known_scores():
    copy, _ = crafted()['perfect_copy']
    assert set(note_metrics(*copy).values()) == {1.0}
    for name in ('no_overlap', 'empty_ref', 'empty_est', 'both_empty'):
        assert set(note_metrics(*crafted()[name][0]).values()) == {0.0}, name
    # 2 of 3 estimates, 2 of 2 references: P = 2/3, R = 1, F = 2 P R / (P + R)
    s = note_metrics(*crafted()['nan_pitch'][0])
    p = np.float64(2) / np.float64(3)
    assert (s['Precision'], s['Recall'], s['F-measure']) == (float(p), 1.0, float(2 * p * 1.0 / (p + 1.0)))
    # without the offset criterion only that family is returned, unchanged
    case = random_notes(*RANDOM_SIZES[2])
    full, no = note_metrics(*case), note_metrics(*case, offset_ratio=None)
    assert sorted(no) == sorted(k + '_no_offset' for k in KEYS) and all(no[k] == full[k] for k in no)
    assert note_counts(*case, offset_ratio=None).tp is None
    with pytest.raises(ValueError):
        note_counts(np.zeros(3), np.zeros((2, 2)), np.zeros(1), np.zeros((1, 2)))


def test_a_nan_pitch_counts_but_never_matches():
    case, _ = crafted()['nan_pitch']
    got = note_counts(*case)
    assert got == NoteCounts(2, 3, 2, 2)
    only_nan = notes([(60, 0.0, 1.0)]) + notes([(float('nan'), 0.0, 1.0)])
    assert note_counts(*only_nan) == NoteCounts(1, 1, 0, 0)


def test_chains_and_cliques():
    for n in (60, 400):
        assert note_counts(*chain(n))[2:] == (n // 2, n // 2) == dense_counts(chain(n))
    for shape in ((64, 64), (64, 65), (65, 64)):
        got = note_counts(*clique(*shape))
        assert (got.tp, got.tp_no_offset) == dense_counts(clique(*shape)) and got.tp_no_offset == 64
    # a chain far deeper than Python's recursion limit
    assert note_counts(*chain(5000))[2:] == (2500, 2500)


def test_component_sizes_stay_below_the_device_capacity():
    from timbre_trap import _hip
    cap = _hip.lib().tt_notescore_max()
    assert cap >= 64
    for name, case in random_cases().items():
        assert max(largest_component(case)) <= cap, name
    # the sizes the device tests rely on: what fits, what does not
    assert largest_component(chain(60)) == (30, 30) and largest_component(chain(400)) == (200, 200)
    assert largest_component(clique(cap, cap)) == (cap, cap) and largest_component(clique(cap, cap + 1)) == (cap, cap + 1)
    # the densest generated case is far from the capacity: the fallback is for input that is not music
    assert max(largest_component(random_notes(*RANDOM_SIZES[-1]))) <= cap // 2
    assert TOL == dict(onset_tolerance=0.05, pitch_tolerance=0.5, offset_ratio=0.2, offset_min_tolerance=0.05)
