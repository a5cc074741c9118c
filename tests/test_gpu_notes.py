"""
Note annotations on the MI355X (csrc/notes.hip, tt_target_activations_spans; timbre_trap.utils.notes_csr_device / notes_to_activations /
multipitch_counts_device_notes / MultipitchEvaluator.evaluate_notes) against the host route -- ``notes_to_multi_pitch``, then the existing
``multi_pitch_to_activations`` / ``evaluate_activations`` on its lists -- on the note sets of tests/test_notes_restatement.py, which pins
that host function to the reference's recorded lists, and against the reference's recorded target maps (tests/golden/notes.npz).

Nothing rounds differently on the two sides: every comparison is ``array_equal`` / ``torch.equal`` / ``==``, never a tolerance.
Sizes come from the library: N = 2 tt_note_tile_frames() + 37 frames and L = 2 tt_note_chunk() + 19 notes (two full tiles and a ragged
one for every kernel), and N = 1, L = 1.
"""

import functools
import warnings

import numpy as np
import pytest
import torch

from timbre_trap import _hip
from timbre_trap.utils import (MultipitchEvaluator, multi_pitch_to_activations, multipitch_counts_device, multipitch_counts_device_notes,
                               multipitch_metrics_device, multipitch_metrics_device_notes, note_tiles, notes, notes_csr_device,
                               notes_to_activations, notes_to_multi_pitch)
from timbre_trap.utils.metrics import MPE_MAX_REF
from timbre_trap.utils.targets import _gaussian_weights

from test_mpe_restatement import FV, MIDI_FREQS, activations, est_times
from test_notes_restatement import CROWD, CROWD_FRAMES, N_EDGE, golden_sets, lists_of, note_case, same_lists

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SHAPES = ('tiles', 'one_frame', 'one_note', 'one_each')
BLURS = (2.5, 0, 5.0)
WARNING = 'Could not fully represent'
COUNTS = ('tp', 'tp_chroma', 'n_ref', 'n_est')
T_EST = 300


def shape(name):
    tile, chunk = note_tiles()
    n, l = 2 * tile + 37, 2 * chunk + 19
    return {'tiles': (n, l), 'one_frame': (1, l), 'one_note': (n, 1), 'one_each': (1, 1)}[name]


def case_of(name, evaluable=False, crowd=False):
    return note_case(*shape(name), evaluable, crowd)


def arrays(case):
    return np.array(case['pitches']), np.array(case['intervals']), np.array(case['times'])      # writable copies of the cached inputs


def caught(fn):
    """fn() with every warning recorded: (result, whether the target code's RuntimeWarning was among them)."""
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        out = fn()
    return out, any(issubclass(x.category, RuntimeWarning) and WARNING in str(x.message) for x in w)


@functools.lru_cache(maxsize=None)
def host_targets(case_key, blur):
    """multi_pitch_to_activations of the host lists, once per case and blur: (read-only ndarray, warned)."""
    case = note_case(*case_key[1:])
    out, warned = caught(lambda: multi_pitch_to_activations(list(lists_of(case)), MIDI_FREQS, blur, DEV))
    out.setflags(write=False)
    return out, warned


def spans_through_ctypes(intervals, times):
    lib = _hip.lib()
    t_d, iv_d = torch.from_numpy(times).to(DEV), torch.from_numpy(intervals).to(DEV)
    lo = torch.full((len(intervals),), -7, dtype=torch.int32, device=DEV)
    hi = torch.full((len(intervals),), -7, dtype=torch.int32, device=DEV)
    _hip.check(lib.tt_note_spans(_hip.ptr(t_d), len(times), _hip.ptr(iv_d), len(intervals), _hip.ptr(lo), _hip.ptr(hi), _hip.stream_ptr()))
    return lo, hi


def test_tile_constants():
    tile, chunk = note_tiles()
    assert tile >= 64 and chunk >= 64 and tile % 64 == 0
    assert shape('tiles')[1] >= N_EDGE and shape('tiles')[0] > CROWD_FRAMES[1]


@pytest.mark.parametrize('name', SHAPES)
def test_spans_are_searchsorted(name):
    _, intervals, times = arrays(case_of(name))
    lo, hi = (x.cpu().numpy() for x in spans_through_ctypes(intervals, times))
    real = ~np.isnan(intervals).any(axis=1)
    assert np.array_equal(lo[real], np.searchsorted(times, intervals[real, 0], side='left'))
    assert np.array_equal(hi[real], np.searchsorted(times, intervals[real, 1], side='left'))
    assert (hi[~real] <= lo[~real]).all()                                          # a NaN bound: an empty range
    if name == 'tiles':
        assert (~real).sum() == 3 and (lo[0], hi[0], lo[1], hi[1]) == (20, 30, 41, 50) and (lo[6], hi[6]) == (0, len(times))
        assert hi[2] <= lo[2] and hi[3] <= lo[3] and hi[4] <= lo[4] and hi[5] <= lo[5]


@pytest.mark.parametrize('evaluable', (False, True))
@pytest.mark.parametrize('name', SHAPES)
def test_csr_is_the_host_lists_in_note_order(name, evaluable):
    case = case_of(name, evaluable)
    pitches, intervals, times = arrays(case)
    off, note_idx = notes_csr_device(pitches, intervals, times, DEV)
    assert off.is_cuda and off.dtype == torch.int64 and note_idx.dtype == torch.int32 and off.shape == (len(times) + 1,)
    off, note_idx = off.cpu().numpy(), note_idx.cpu().numpy()
    want = lists_of(case)
    assert off[0] == 0 and np.array_equal(np.diff(off), [len(f) for f in want]) and len(note_idx) == off[-1]
    assert same_lists([pitches[note_idx[a:b]] for a, b in zip(off[:-1], off[1:])], want)
    want_off, want_idx = notes._host_pairs(intervals, times)                       # ascending note index within a frame
    assert np.array_equal(off, want_off) and np.array_equal(note_idx, want_idx)
    if name == 'tiles':
        assert off[-1] > 3 * len(times) and (np.diff(off) > 0).all()


def test_fill_respects_its_capacity():
    _, intervals, times = arrays(case_of('tiles'))
    lib, n = _hip.lib(), len(times)
    lo, hi = spans_through_ctypes(intervals, times)
    off, full = notes_csr_device(np.zeros(len(intervals)), intervals, times, DEV)
    total = full.numel()
    cap = total // 2 + 1
    part = torch.full((total,), -7, dtype=torch.int32, device=DEV)
    _hip.check(lib.tt_note_fill(_hip.ptr(lo), _hip.ptr(hi), len(intervals), n, _hip.ptr(off), cap, _hip.ptr(part), _hip.stream_ptr()))
    assert torch.equal(part[:cap], full[:cap]) and bool((part[cap:] == -7).all())
    count = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    _hip.check(lib.tt_note_count(_hip.ptr(lo), _hip.ptr(hi), len(intervals), n, _hip.ptr(count), _hip.stream_ptr()))
    assert torch.equal(count.to(torch.int64), off[1:] - off[:-1])


@pytest.mark.parametrize('blur', BLURS)
@pytest.mark.parametrize('name', SHAPES)
def test_targets_are_the_host_route(name, blur):
    case = case_of(name)
    want, want_warned = host_targets(case['key'], blur)
    got, warned = caught(lambda: notes_to_activations(*arrays(case), MIDI_FREQS, blur, DEV))
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (len(MIDI_FREQS), len(case['times']))
    assert np.array_equal(got, want)
    assert warned == want_warned
    if name == 'tiles':
        assert warned and want.max() == 1.0 and 0 < (want > 0).sum() < want.size
        assert (want[:, 110] == 1.0).sum() >= 2                                    # the twins paint one bin, their neighbour the next


@pytest.mark.parametrize('tag', ('a', 'b'))
def test_targets_are_the_reference_maps(tag):
    sets, times, midi_freqs = golden_sets()
    s = sets[tag]
    for blur, key in ((2.5, 'act_blur'), (0, 'act_noblur')):
        got, warned = caught(lambda: notes_to_activations(np.array(s['pitches']), np.array(s['intervals']), np.array(times), midi_freqs,
                                                          blur, DEV))
        assert np.array_equal(got, s[key])
        assert warned == s['warned']                                               # fires iff the reference's did
    assert s['warned'] == (tag == 'a')


@pytest.mark.parametrize('blur', (2.5, 0))
@pytest.mark.parametrize('name', ('tiles', 'one_frame'))
def test_span_entry_is_the_pair_entry(name, blur):
    """tt_target_activations_spans against tt_target_activations on the expanded (bin, frame) pairs, through the C ABI."""
    pitches, intervals, times = arrays(case_of(name))
    lib, F, T = _hip.lib(), len(MIDI_FREQS), len(times)
    bins, _ = notes._note_bins(pitches, MIDI_FREQS)
    lo, hi = notes._host_spans(intervals, times)
    kept = np.flatnonzero((bins >= 0) & (hi > lo))
    pair_b = np.concatenate([np.full(hi[i] - lo[i], bins[i]) for i in kept]).astype(np.int32)
    pair_t = np.concatenate([np.arange(lo[i], hi[i]) for i in kept]).astype(np.int32)
    assert len(pair_b) > len(kept) or T == 1
    radius, w_d = 0, None
    if blur:
        w, radius = _gaussian_weights((2 * blur) / 5)
        w_d = torch.from_numpy(w).to(DEV)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)              # noqa: E731
    outs = []
    for spans in (False, True):
        work = torch.full((F, T), 3.0, dtype=torch.float64, device=DEV)
        out = torch.full((F, T), 3.0, dtype=torch.float64, device=DEV)
        if spans:
            b_d, lo_d, hi_d = dev(bins), dev(lo.astype(np.int32)), dev(hi.astype(np.int32))
            _hip.check(lib.tt_target_activations_spans(_hip.ptr(b_d), _hip.ptr(lo_d), _hip.ptr(hi_d), len(bins), _hip.ptr(w_d), radius, F, T,
                                                       _hip.ptr(work), _hip.ptr(out), _hip.stream_ptr()))
        else:
            b_d, t_d = dev(pair_b), dev(pair_t)
            _hip.check(lib.tt_target_activations(_hip.ptr(b_d), _hip.ptr(t_d), len(pair_b), _hip.ptr(w_d), radius, F, T, _hip.ptr(work),
                                                 _hip.ptr(out), _hip.stream_ptr()))
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and float(outs[0].max()) == 1.0 and float(outs[0].min()) == 0.0


def eval_inputs(case):
    x = torch.from_numpy(np.array(activations(0.05, T_EST))).to(DEV)
    return x, est_times(T_EST)


def check_scores(case, times=None):
    pitches, intervals, ref_time = arrays(case)
    lists = list(lists_of(case))
    n_host_frames = sum(len(f) > MPE_MAX_REF for f in lists)                       # the estimates (<= 236 peaks a frame) never exceed theirs
    if times is not None:                                                          # a re-ordered grid: the lists in its order
        lists, ref_time = [lists[i] for i in times], ref_time[times]
    x, est_time = eval_inputs(case)
    kw = dict(window=0.5, n_valid_bins=FV)
    want = multipitch_counts_device(ref_time, lists, est_time, x, MIDI_FREQS, **kw)
    got = multipitch_counts_device_notes(ref_time, pitches, intervals, est_time, x, MIDI_FREQS, **kw)
    for name in COUNTS:
        assert got[name].dtype == torch.int32 and torch.equal(got[name], want[name]), name
    assert np.array_equal(got['sums'], want['sums']) and got['n_host_frames'] == want['n_host_frames'] == n_host_frames
    scores = multipitch_metrics_device(ref_time, lists, est_time, x, MIDI_FREQS, **kw)
    assert multipitch_metrics_device_notes(ref_time, pitches, intervals, est_time, x, MIDI_FREQS, **kw) == scores and len(scores) == 14
    ev = MultipitchEvaluator()
    tagged = ev.evaluate_notes(est_time, x[None], MIDI_FREQS, ref_time, pitches, intervals, n_valid_bins=FV)
    assert tagged == ev.evaluate_activations(est_time, x[None], MIDI_FREQS, ref_time, lists, n_valid_bins=FV) and len(tagged) == 15
    return got, tagged


@pytest.mark.parametrize('name', SHAPES)
def test_evaluate_notes_is_evaluate_activations(name):
    got, tagged = check_scores(case_of(name, evaluable=True))
    if name == 'tiles':
        assert got['n_host_frames'] == 0 and got['sums'][0] > 0 and tagged['mpe/f1-score'] > 0 and int(got['n_ref'].max()) <= MPE_MAX_REF


def test_frames_over_the_capacity_go_to_the_host():
    case = case_of('tiles', evaluable=True, crowd=True)
    a, b = CROWD_FRAMES
    got, _ = check_scores(case)
    assert got['n_host_frames'] == b - a > 0 and int(got['n_ref'][a:b].min()) >= CROWD == MPE_MAX_REF + 6


def test_unsorted_times_give_the_host_route():
    case = case_of('tiles')
    pitches, intervals, times = arrays(case)
    perm = np.random.default_rng(3).permutation(len(times))
    want, want_warned = host_targets(case['key'], 2.5)
    got, warned = caught(lambda: notes_to_activations(pitches, intervals, times[perm], MIDI_FREQS, 2.5, DEV))
    assert np.array_equal(got, want[:, perm]) and warned == want_warned
    off, note_idx = (x.cpu().numpy() for x in notes_csr_device(pitches, intervals, times[perm], DEV))
    lists = lists_of(case)
    assert same_lists([pitches[note_idx[a:b]] for a, b in zip(off[:-1], off[1:])], [lists[i] for i in perm])
    check_scores(case_of('tiles', evaluable=True), times=perm)


def test_no_notes():
    n = shape('tiles')[0]
    times = np.array(note_case(n, 0)['times'])
    none, no_iv = np.empty(0), np.empty((0, 2))
    for blur in BLURS:
        got, warned = caught(lambda: notes_to_activations(none, no_iv, times, MIDI_FREQS, blur, DEV, return_tensor=True))
        assert got.is_cuda and got.shape == (len(MIDI_FREQS), n) and not bool(got.any()) and not warned
    off, note_idx = notes_csr_device(none, no_iv, times, DEV)
    assert off.shape == (n + 1,) and not bool(off.any()) and note_idx.numel() == 0
    assert all(f.size == 0 for f in notes_to_multi_pitch(none, no_iv, times))
    check_scores(note_case(n, 0, True))


def test_two_runs_are_identical():
    case = case_of('tiles', evaluable=True)
    pitches, intervals, times = arrays(case)
    a = notes_to_activations(pitches, intervals, times, MIDI_FREQS, 2.5, DEV, return_tensor=True)
    b = notes_to_activations(pitches, intervals, times, MIDI_FREQS, 2.5, DEV, return_tensor=True)
    assert a.is_cuda and a.dtype == torch.float64 and torch.equal(a, b) and float(a.max()) == 1.0
    (off1, idx1), (off2, idx2) = notes_csr_device(pitches, intervals, times, DEV), notes_csr_device(pitches, intervals, times, DEV)
    assert torch.equal(off1, off2) and torch.equal(idx1, idx2) and idx1.numel() > 0
    x, est_time = eval_inputs(case)
    c1 = multipitch_counts_device_notes(times, pitches, intervals, est_time, x, MIDI_FREQS, n_valid_bins=FV)
    c2 = multipitch_counts_device_notes(times, pitches, intervals, est_time, x, MIDI_FREQS, n_valid_bins=FV)
    assert all(torch.equal(c1[k], c2[k]) for k in COUNTS) and np.array_equal(c1['sums'], c2['sums'])


def test_argument_errors():
    case = case_of('tiles', evaluable=True)
    pitches, intervals, times = arrays(case)
    x, est_time = eval_inputs(case)
    ev = MultipitchEvaluator()
    with pytest.raises(ValueError):                                                # one interval per pitch
        notes_to_activations(pitches[:-1], intervals, times, MIDI_FREQS, device=DEV)
    with pytest.raises(ValueError):
        notes_csr_device(pitches, intervals[:-1], times, DEV)
    with pytest.raises(ValueError):
        ev.evaluate_notes(est_time, x, MIDI_FREQS, times, pitches[:-1], intervals, n_valid_bins=FV)
    with pytest.raises(ValueError):                                                # estimate times / frames mismatch
        ev.evaluate_notes(est_time[:-1], x, MIDI_FREQS, times, pitches, intervals, n_valid_bins=FV)
    with pytest.raises(RuntimeError):                                              # no CPU fallback
        notes_to_activations(pitches, intervals, times, MIDI_FREQS, device='cpu')
    with pytest.raises(RuntimeError):
        ev.evaluate_notes(est_time, x.cpu(), MIDI_FREQS, times, pitches, intervals, n_valid_bins=FV)
    # note 16 is far above 5 kHz and silent: nobody minds (the case scored above); let it sound and both routes refuse it
    assert pitches[16] > 5000.0 and intervals[16, 0] == intervals[16, 1]
    for bad in (pitches[16], 10.0):
        p, iv = pitches.copy(), intervals.copy()
        p[16], iv[16, 1] = bad, iv[16, 0] + 0.01
        with pytest.raises(ValueError):
            ev.evaluate_notes(est_time, x, MIDI_FREQS, times, p, iv, n_valid_bins=FV)
        with pytest.raises(ValueError):
            ev.evaluate_activations(est_time, x, MIDI_FREQS, times, notes_to_multi_pitch(p, iv, times), n_valid_bins=FV)
        p[16], iv[16, 1] = bad, iv[16, 0]                                          # the same pitch, silent again
        assert ev.evaluate_notes(est_time, x, MIDI_FREQS, times, p, iv, n_valid_bins=FV) == \
            ev.evaluate_activations(est_time, x, MIDI_FREQS, times, list(lists_of(case)), n_valid_bins=FV)
