"""
The device multi-pitch scorer (csrc/mpe.hip; timbre_trap.utils.multipitch_counts_device / multipitch_metrics_device /
MultipitchEvaluator.evaluate_activations) on the MI355X against the host route -- download, ``activations_to_multi_pitch``,
``multipitch_metrics`` -- on the inputs of tests/test_mpe_restatement.py, which computes the host route once per input.

The scorer works on small integers and float64 comparisons only: every comparison below is ``==``, never a tolerance.
F = 540 bins at ``16.76557586 + k / 5`` MIDI, 472 of them below 5 kHz; T = 300 estimate frames, 257 reference frames.
"""

import numpy as np
import pytest
import torch

from timbre_trap.utils import (MultipitchEvaluator, activations_to_multi_pitch, multipitch_counts_device, multipitch_metrics,
                               multipitch_metrics_device, peaks_above)
from timbre_trap.utils.metrics import MPE_MAX_EST, MPE_MAX_REF, mpe_compact
from timbre_trap.utils.processing import _device_pick

from test_mpe_restatement import (CASES, COMPACT_T, F, FV, MIDI_FREQS, THRESHOLD, activations, capacity_cases, edge_activations,
                                  edge_cases, host_frames, host_route, mpe_case, over_capacity, tie_case)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
COUNTS = ('tp', 'tp_chroma', 'n_ref', 'n_est')


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)             # a writable, contiguous copy (the cached inputs are read-only)


def args(case, x=None):
    return (case['ref_time'], list(case['ref_freqs']), case['est_time'], dev(case['x']) if x is None else x, MIDI_FREQS)


def kwargs(case):
    return dict(window=case['window'], t=case['t'], peaks_only=case['peaks_only'], n_valid_bins=FV)


def check_against_host(case, n_host_frames=0):
    want, scores = host_route(case)
    got = multipitch_counts_device(*args(case), **kwargs(case))
    for name, w in zip(COUNTS, want):
        g = got[name]
        assert g.is_cuda and g.dtype == torch.int32
        assert np.array_equal(g.cpu().numpy(), w), name
    assert got['n_host_frames'] == n_host_frames
    dev_scores = multipitch_metrics_device(*args(case), **kwargs(case))
    assert list(dev_scores) == list(scores) and len(scores) == 14
    assert dev_scores == scores                              # floats compared with ==: bit for bit


def check_csr(x, peaks_only):
    xd = dev(x)
    est_off, est_bins, n_est, bad = mpe_compact(xd, THRESHOLD, peaks_only, FV)
    mask = (peaks_above(xd, THRESHOLD, FV) if peaks_only else _device_pick(xd, THRESHOLD, 1, FV)).cpu().numpy()
    bins, frames = np.nonzero(mask)
    order = np.lexsort((bins, frames))
    off = est_off.cpu().numpy()
    assert off.dtype == np.int64 and off[0] == 0 and off.shape == (x.shape[1] + 1,)
    assert np.array_equal(np.diff(off), np.bincount(frames, minlength=x.shape[1]))
    assert np.array_equal(n_est.cpu().numpy(), np.diff(off))
    assert np.array_equal(est_bins[:off[-1]].cpu().numpy(), bins[order])
    assert not bad.any()                                     # no table of out-of-range bins was given
    return [list(est_bins[off[i]:off[i + 1]].cpu().numpy()) for i in range(x.shape[1])] if x.shape[1] <= 8 else None


@pytest.mark.parametrize('peaks_only', (True, False))
@pytest.mark.parametrize('n_frames', COMPACT_T)
def test_compaction(n_frames, peaks_only):
    check_csr(activations(0.3, n_frames, seed=1), peaks_only)


@pytest.mark.parametrize('peaks_only', (True, False))
def test_compaction_edges(peaks_only):
    got = check_csr(edge_activations(), peaks_only)
    if peaks_only:
        assert got[0] == [] and got[1] == [0] and got[2] == [FV - 1] and got[3] == [100] and got[4] == []
        assert got[5] == list(range(0, FV, 2)) and got[6] == [31]
    else:
        assert got[0] == [10, 11, 12, 20, 21] and got[2] == [FV - 1] and got[6] == [30, 31, 32]


@pytest.mark.parametrize('density,jitter', CASES)
def test_counts_and_scores(density, jitter):
    check_against_host(mpe_case(density, jitter))


@pytest.mark.parametrize('name', sorted(edge_cases()))
def test_edges(name):
    check_against_host(edge_cases()[name])


@pytest.mark.parametrize('which', ('ref', 'est'))
def test_over_capacity_frames_go_to_the_host(which):
    case = capacity_cases()[which]
    n = over_capacity(case)
    assert n >= 3
    if which == 'ref':
        assert max(len(f) for f in case['ref_freqs']) == MPE_MAX_REF + 1
    else:
        assert (np.array(case['x'][:FV]) >= THRESHOLD).sum(axis=0).max() > MPE_MAX_EST
    check_against_host(case, n_host_frames=n)


def test_est_midi_round_trip_decides_the_tie():
    tie = tie_case()
    (tp, _, _, _), _ = host_route(tie)
    assert list(tp) == [0 if tie['midi_freqs_says'] else 1]
    check_against_host(tie)


def test_evaluator_on_activations_is_evaluate():
    case = mpe_case(0.05)
    x = dev(case['x'])
    masked = x.clone()
    masked[FV:] = 0
    frames = activations_to_multi_pitch(masked, MIDI_FREQS, peaks_only=True)         # the host route as evaluate() ran it so far
    assert all(np.array_equal(a, b) for a, b in zip(frames, host_frames(case['x'])))
    ev = MultipitchEvaluator()
    want = ev.evaluate(case['est_time'], frames, case['ref_time'], list(case['ref_freqs']))
    got = ev.evaluate_activations(case['est_time'], x[None], MIDI_FREQS, case['ref_time'], list(case['ref_freqs']), n_valid_bins=FV)
    assert got == want and 'mpe/f1-score' in got and len(got) == 15 and got['mpe/f1-score'] > 0
    assert MultipitchEvaluator(tolerance=0.25).evaluate_activations(case['est_time'], x, MIDI_FREQS, case['ref_time'], list(case['ref_freqs']),
                                                                    n_valid_bins=FV) == \
        MultipitchEvaluator(tolerance=0.25).evaluate(case['est_time'], frames, case['ref_time'], list(case['ref_freqs']))


@pytest.mark.parametrize('dtype', (torch.float16, torch.bfloat16))
def test_16_bit_activations_are_upcast(dtype):
    case = mpe_case(0.3)
    x16 = dev(case['x']).to(dtype)
    got = multipitch_counts_device(*args(case, x16), **kwargs(case))
    want = multipitch_counts_device(*args(case, x16.float()), **kwargs(case))
    for name in COUNTS:
        assert torch.equal(got[name], want[name])
    assert np.array_equal(got['sums'], want['sums']) and got['sums'][0] > 0


def test_two_runs_are_identical():
    case = mpe_case(0.3, True)
    a = multipitch_counts_device(*args(case), **kwargs(case))
    b = multipitch_counts_device(*args(case), **kwargs(case))
    for name in COUNTS:
        assert torch.equal(a[name], b[name])
    assert np.array_equal(a['sums'], b['sums'])
    xd = dev(case['x'])
    (off1, bins1, n1, _), (off2, bins2, n2, _) = mpe_compact(xd, THRESHOLD, True, FV), mpe_compact(xd, THRESHOLD, True, FV)
    total = int(off1[-1])
    assert torch.equal(off1, off2) and torch.equal(n1, n2) and torch.equal(bins1[:total], bins2[:total]) and total > 0


def test_argument_errors():
    case = mpe_case(0.05)
    ref_time, ref_freqs, est_time, x, midi = args(case)
    kw = kwargs(case)
    with pytest.raises(RuntimeError):                                      # CPU tensor: no fallback
        multipitch_metrics_device(ref_time, ref_freqs, est_time, x.cpu(), midi, **kw)
    with pytest.raises(ValueError):                                        # reference times / frames mismatch
        multipitch_metrics_device(ref_time[:-1], ref_freqs, est_time, x, midi, **kw)
    with pytest.raises(ValueError):                                        # estimate times / frames mismatch
        multipitch_metrics_device(ref_time, ref_freqs, est_time[:-1], x, midi, **kw)
    for bad in (10.0, 6000.0):                                             # reference frequency out of [20, 5000] Hz
        with pytest.raises(ValueError):
            multipitch_metrics_device(ref_time, [np.array([bad])] + ref_freqs[1:], est_time, x, midi, **kw)
    with pytest.raises(ValueError):                                        # unmasked: peaks above 5 kHz are out of range, as on the host
        multipitch_metrics_device(ref_time, ref_freqs, est_time, x, midi, window=0.5, n_valid_bins=0)
    with pytest.raises(ValueError):
        multipitch_metrics(ref_time, ref_freqs, est_time, host_frames(case['x'], fv=0))
    with pytest.raises(ValueError):
        multipitch_metrics_device(ref_time, ref_freqs, est_time, x.double(), midi, **kw)
    zero = multipitch_metrics([], [], [], [])
    assert multipitch_metrics_device([], [], est_time, x, midi, **kw) == zero
    assert multipitch_metrics_device(ref_time, ref_freqs, [], x[:, :0], midi, **kw) == zero
    assert len(zero) == 14 and F == x.shape[0]
