"""
Pitch contours on the MI355X (csrc/contours.hip; timbre_trap.utils.note_contours / refined_pitches / refine_multi_pitch /
activations_to_multi_pitch_refined; TimbreTrap.transcribe_contours) against the NumPy reference of tests/contours_ref.py, which
tests/test_contours_restatement.py pins on the CPU.

Every result is an integer, an exact fp32 value or a float64 value formed by individually rounded operations: every comparison below is
``==`` -- integers directly, fp32 by bit pattern, ``pitch`` with NaNs equal -- never a tolerance.  The pass mask the reference is fed is
the DOWNLOADED output of ``_device_pick`` (tt_peak_pick, modes 1 and 2) on the same input, and the notes it is fed are the device's
(tests/test_gpu_events.py holds those to their own reference).  That the comparison is not one of zeros is the restatement file's
business: it checks, for every generated case used here, that at least 90 % of the voiced frames have a non-zero ``delta``.
"""

import io

import numpy as np
import pytest
import torch

from timbre_trap import _hip
from timbre_trap.utils import (NoteContours, activations_to_multi_pitch, activations_to_multi_pitch_refined, contours_to_bends, note_contours,
                               note_events, refine_multi_pitch, refined_pitches, write_midi_bends)
from timbre_trap.utils.events import _pitch_rows
from timbre_trap.utils.metrics import mpe_compact
from timbre_trap.utils.processing import _device_pick

import contours_ref as C
from cl16_ref import FILL_BIG, Arena
from test_contours_restatement import (DETUNE_BAR_CENTS, M5, RANDOM_T, THR, UNITS, crafted, detuned_notes, literal_columns, random_cases, ridge,
                                       ridge_error_cents, smooth_map)
from test_mpe_restatement import FV, MIDI_FREQS, activations

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BADARG = b'ttrap: bad argument'
FRAME_TYPES = dict(bin=torch.int32, delta=torch.float32, value=torch.float32, pitch=torch.float64, bend=torch.int32)
NOTE_TYPES = dict(n_voiced=torch.int32, bend_sum=torch.int64, bend_min=torch.int32, bend_max=torch.int32)


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)             # a writable, contiguous copy (the cached inputs are read-only)


def device_pass(x, mode, fv=0, thr=THR):
    return _device_pick(dev(x), thr, mode, fv).cpu().numpy() > 0


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(co, want, what=''):
    assert isinstance(co, NoteContours) and co.units == UNITS
    assert co.frame_off.is_cuda and co.frame_off.dtype == torch.int64 and np.array_equal(co.frame_off.cpu().numpy(), want['frame_off']), what
    for name, dtype in {**FRAME_TYPES, **NOTE_TYPES}.items():
        g = getattr(co, name)
        assert g.is_cuda and g.dtype == dtype and g.shape == want[name].shape, (what, name)
        g = g.cpu().numpy()
        if name == 'pitch':
            assert np.array_equal(g, want[name], equal_nan=True), (what, name)
        else:
            assert np.array_equal(bits(g), bits(want[name])), (what, name)


def check(x, group_off, mode, fv, gap, m, passed=None, order='pitch', what=''):
    """note_events + note_contours on the device against the reference fed with the device's pass mask and the device's notes."""
    passed = device_pass(x, mode, fv) if passed is None else passed
    kw = dict(t=THR, peaks_only=mode == 2, n_valid_bins=fv, bin_groups=group_off)
    ev = note_events(dev(x), m, max_gap=gap, order=order, **kw)
    co = note_contours(dev(x), ev, m, **kw)
    row_pitch = _pitch_rows(m, x.shape[1], 'semitone', group_off)[1]
    want = C.note_contours_ref(passed, x, group_off, m, row_pitch, UNITS, *(getattr(ev, n).cpu().numpy() for n in ('item', 'row', 'onset', 'end')),
                               f_valid=fv)
    same(co, want, what)
    assert torch.equal(co.n_voiced, ev.n_active)                                  # the voiced frames are the active ones
    return ev, co, want


# ---- random maps ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode', (1, 2))
@pytest.mark.parametrize('n_frames', RANDOM_T)
def test_random_maps(n_frames, mode):
    n = bridged = 0
    for name, c in random_cases():
        if not name.endswith('_T%d' % n_frames):
            continue
        passed = device_pass(c['x'], mode, c['fv'])
        for gap in (0, 2):
            ev, co, want = check(c['x'], c['group_off'], mode, c['fv'], gap, c['m'], passed, what=(name, gap))
            n += int(want['n_voiced'].sum())
            bridged += int((want['bin'] < 0).sum())
    assert n > 0 and (bridged > 0 or n_frames < 63)


# ---- crafted notes --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(crafted()))
def test_crafted_notes(name):
    c = crafted()[name]
    ev, co, want = check(c['x'], c['group_off'], c['mode'], c['fv'], c['gap'], c['m'])
    spans = list(zip(ev.item.tolist(), ev.row.tolist(), ev.onset.tolist(), ev.end.tolist()))
    if name == 'four_chunks':
        assert spans == [(0, 0, 5, 205)] and int(co.n_voiced[0]) == 200
    if name == 'frames_63_to_65':
        assert spans == [(0, 0, 63, 65)] and co.bin.tolist() == [3, 3]
    if name == 'neighbouring_rows_share_frames':
        assert spans == [(0, 0, 10, 40), (0, 1, 20, 60)] and set(co.bin[:30].tolist()) == {1} and set(co.bin[30:].tolist()) == {4}
    if name == 'last_item_ends_at_T':
        assert spans == [(1, 1, 63, 70)] and set(co.bin.tolist()) == {4}
    if name == 'literals_threshold':                                               # the literal answers, from the device
        names = [k for k, v in literal_columns().items() if v[2] == 0]
        assert spans == [(0, 0, 0, len(names))]
        for k, key in enumerate(names):
            _, f, _, want_delta, want_pitch = literal_columns()[key]
            if key not in ('plateau', 'larger_neighbour'):
                assert (int(co.bin[k]), np.float32(co.delta[k].item()), float(co.pitch[k])) == (f, want_delta, want_pitch), key
    if name == 'literals_peaks_bridged':
        assert int(co.n_voiced[0]) == int(ev.end[0] - ev.onset[0]) - 2 and int(torch.isnan(co.pitch).sum()) == 2
    if name == 'tie_lower_bin':
        assert co.bin.tolist() == [1, 1]


def test_onset_order_gives_the_same_contours_permuted():
    c = dict(random_cases())['groups_T130']
    by_pitch = check(c['x'], c['group_off'], 2, c['fv'], 2, c['m'])
    by_onset = check(c['x'], c['group_off'], 2, c['fv'], 2, c['m'], order='onset')
    assert by_pitch[0].onset.tolist() != by_onset[0].onset.tolist()

    def per_note(ev, co, _):
        off = co.frame_off.tolist()
        out = {}
        for i, key in enumerate(zip(ev.item.tolist(), ev.row.tolist(), ev.onset.tolist())):
            frames = tuple(getattr(co, n)[off[i]:off[i + 1]].cpu().numpy().tobytes() for n in FRAME_TYPES)
            out[key] = frames + tuple(int(getattr(co, n)[i]) for n in NOTE_TYPES)
        return out
    a, b = per_note(*by_pitch), per_note(*by_onset)
    assert a == b and len(a) == by_pitch[0].item.numel() > 10


def test_default_geometry_by_semitone_and_two_runs():
    x = np.stack([activations(0.05, 256, seed=s) for s in (0, 1)])
    kw = dict(t=THR, n_valid_bins=FV)
    ev = note_events(dev(x), MIDI_FREQS, max_gap=2, min_frames=2, **kw)
    co = note_contours(dev(x), ev, MIDI_FREQS, **kw)
    off, row_pitch = _pitch_rows(MIDI_FREQS, 540, 'semitone', None)
    want = C.note_contours_ref(device_pass(x, 2, FV), x, off, MIDI_FREQS, row_pitch, UNITS,
                               *(getattr(ev, n).cpu().numpy() for n in ('item', 'row', 'onset', 'end')), f_valid=FV)
    same(co, want)
    assert ev.item.numel() > 100 and torch.equal(co.n_voiced, ev.n_active) and int((co.bin < 0).sum()) > 0
    assert float((co.delta[co.bin >= 0] != 0).float().mean()) > 0.9
    again = note_contours(dev(x), ev, MIDI_FREQS, **kw)                            # two runs: bit-equal
    for a, b in zip(co[:-1], again[:-1]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    # other units: the bends scale, the contour stays
    coarse = note_contours(dev(x), ev, MIDI_FREQS, units_per_semitone=100, **kw)
    assert coarse.units == 100 and torch.equal(coarse.pitch.view(torch.int64), co.pitch.view(torch.int64))
    voiced = co.bin >= 0
    assert torch.equal(coarse.bend[voiced], torch.round((co.pitch[voiced] - ev.pitch.repeat_interleave(co.frame_off.diff())[voiced]) * 100).int())


# ---- per-frame lists --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('peaks_only', (False, True))
@pytest.mark.parametrize('n_frames', (1, 130))
def test_frames_against_the_reference(n_frames, peaks_only):
    x, m, fv = smooth_map(2, 17, n_frames)[0], dict(random_cases())['bins_T130']['m'], 14
    est_off, est_bins, delta, pitch = refine_multi_pitch(dev(x), m, THR, peaks_only, fv)
    off0, bins0, _, _ = mpe_compact(dev(x), THR, peaks_only, fv)
    n = int(off0[-1])
    assert torch.equal(est_off, off0) and torch.equal(est_bins, bins0[:n]) and n >= 2
    assert delta.dtype == torch.float32 and pitch.dtype == torch.float64 and delta.shape == pitch.shape == (n,)
    want_delta, want_pitch = C.refine_frames_ref(x, est_off.cpu().numpy(), est_bins.cpu().numpy(), m, fv)
    assert np.array_equal(bits(delta.cpu().numpy()), bits(want_delta)) and np.array_equal(pitch.cpu().numpy(), want_pitch)
    if n_frames == 130:
        assert float((delta != 0).float().mean()) > 0.9
    # the host lists in Hz: the same entries, frame by frame
    lists = activations_to_multi_pitch_refined(dev(x), m, peaks_only, THR, fv)
    hz = 440.0 * 2.0 ** ((want_pitch - 69.0) / 12.0)
    o = est_off.cpu().numpy()
    assert len(lists) == n_frames and all(np.array_equal(lists[t], hz[o[t]:o[t + 1]]) for t in range(n_frames))


@pytest.mark.parametrize('peaks_only', (False, True))
def test_refined_lists_at_zero_delta_are_the_unrefined_lists(peaks_only):
    rng = np.random.default_rng(3)
    x = np.zeros((540, 50), dtype=np.float32)
    for t in range(0, 50, 2):                                                      # isolated bins between zeros: every delta is 0
        x[rng.choice(np.arange(0, 540, 2), size=6, replace=False), t] = 0.9
    got = activations_to_multi_pitch_refined(dev(x), MIDI_FREQS, peaks_only, THR)
    want = activations_to_multi_pitch(dev(x), MIDI_FREQS, peaks_only, THR)
    assert len(got) == len(want) == 50 and sum(len(w) for w in want) == 150
    for g, w in zip(got, want):
        assert g.dtype == w.dtype == np.float64 and g.shape == w.shape and np.array_equal(g, w)
    assert not bool(refine_multi_pitch(dev(x), MIDI_FREQS, THR, peaks_only)[2].any())


# ---- the C ABI on a guarded arena -----------------------------------------------------------------------------------------------------

def abi_notes(x, group_off, mode, fv, m, row_pitch, ev, units=UNITS):
    lib, st = _hip.lib(), _hip.stream_ptr()
    B, F, T = x.shape
    P, L = len(group_off) - 1, len(ev[0])
    frame_off = np.concatenate([[0], np.cumsum(ev[3].astype(np.int64) - ev[2])])
    total = int(frame_off[-1])
    a = Arena(FILL_BIG, DEV)
    a.inp('x', torch.from_numpy(np.array(x)), shift=4)
    a.inp('g', torch.from_numpy(np.array(group_off, dtype=np.int32)))
    a.inp('m', torch.from_numpy(np.array(m, dtype=np.float64)), shift=8)
    a.inp('rp', torch.from_numpy(np.array(row_pitch, dtype=np.float64)))
    for k, name in enumerate(('item', 'row', 'onset', 'end')):
        a.inp(name, torch.from_numpy(np.array(ev[k], dtype=np.int32)), shift=4 * (k % 2))
    a.inp('frame_off', torch.from_numpy(frame_off), shift=8)
    for k, (name, dtype) in enumerate(FRAME_TYPES.items()):
        a.out(name, (total,), dtype, shift=8 * (k % 2))
    for k, (name, dtype) in enumerate(NOTE_TYPES.items()):
        a.out(name, (L,), dtype, shift=8 * ((k + 1) % 2))
    a.build()
    p = a.ptr
    assert lib.tt_contours_notes(p('x'), B, F, T, THR, mode, fv, p('g'), P, p('m'), p('rp'), units, p('item'), p('row'), p('onset'), p('end'), L,
                                 p('frame_off'), p('bin'), p('delta'), p('value'), p('pitch'), p('bend'), p('n_voiced'), p('bend_sum'),
                                 p('bend_min'), p('bend_max'), st) == 0
    a.verify('tt_contours_notes', finite=False)                                    # an unvoiced frame's pitch is NaN by design
    return dict(frame_off=frame_off, **{n: a.get(n).numpy() for n in list(FRAME_TYPES) + list(NOTE_TYPES)})


@pytest.mark.parametrize('mode', (1, 2))
def test_abi_notes_on_the_arena(mode):
    c = dict(random_cases())['groups_T130']
    x, g, fv, m = c['x'], c['group_off'], c['fv'], c['m']
    passed = device_pass(x, mode, fv)
    events = note_events(dev(x), m, t=THR, peaks_only=mode == 2, n_valid_bins=fv, bin_groups=g, max_gap=2)
    ev = [getattr(events, n).cpu().numpy() for n in ('item', 'row', 'onset', 'end')]
    row_pitch = _pitch_rows(m, x.shape[1], 'semitone', g)[1]
    first, second = abi_notes(x, g, mode, fv, m, row_pitch, ev), abi_notes(x, g, mode, fv, m, row_pitch, ev)
    want = C.note_contours_ref(passed, x, g, m, row_pitch, UNITS, *ev, f_valid=fv)
    for k in want:
        assert first[k].tobytes() == second[k].tobytes(), k                        # bit-identical across two calls
        if k == 'pitch':
            assert np.array_equal(first[k], want[k], equal_nan=True)
        else:
            assert np.array_equal(bits(first[k]), bits(want[k])), k
    assert (want['bin'] < 0).any() and len(ev[0]) > 10
    # the notes in another order, and a row whose pitch is NaN: its bends are 0
    perm = np.random.default_rng(0).permutation(len(ev[0]))
    shuffled = abi_notes(x, g, mode, fv, m, np.array([row_pitch[0], np.nan]), [e[perm] for e in ev])
    want2 = C.note_contours_ref(passed, x, g, m, np.array([row_pitch[0], np.nan]), UNITS, *[e[perm] for e in ev], f_valid=fv)
    for k in want2:
        assert np.array_equal(bits(shuffled[k]), bits(want2[k]), equal_nan=(k == 'pitch')), k
    assert not shuffled['bend'][np.repeat(ev[1][perm], np.diff(shuffled['frame_off'])) == 1].any()


def abi_frames(x, fv, est_off, est_bins, m, cap):
    lib, st = _hip.lib(), _hip.stream_ptr()
    a = Arena(FILL_BIG, DEV)
    a.inp('x', torch.from_numpy(np.array(x)), shift=4)
    a.inp('off', torch.from_numpy(np.array(est_off, dtype=np.int64)), shift=8)
    a.inp('bins', torch.from_numpy(np.array(est_bins, dtype=np.int32)), shift=4)
    a.inp('m', torch.from_numpy(np.array(m, dtype=np.float64)))
    a.out('delta', (cap,), torch.float32, shift=4)
    a.out('pitch', (cap,), torch.float64, shift=8)
    a.build()
    p = a.ptr
    assert lib.tt_contours_frames(p('x'), x.shape[0], x.shape[1], fv, p('off'), p('bins'), cap, p('m'), p('delta'), p('pitch'), st) == 0
    a.verify('tt_contours_frames')                                                 # every slot below the capacity written, none beyond
    return a.get('delta').numpy(), a.get('pitch').numpy()


def test_abi_frames_on_the_arena_literals_and_capacity():
    cols = literal_columns()
    names = [k for k, v in cols.items() if v[2] == 0 and k not in ('nan_neighbour', 'infinite_bin')]
    x = np.stack([cols[k][0] for k in names], axis=1)                              # (5, n): one literal column per frame, its bin listed
    delta, pitch = abi_frames(x, 0, np.arange(len(names) + 1), [cols[k][1] for k in names], M5, len(names))
    assert delta.tolist() == [cols[k][3] for k in names] and pitch.tolist() == [cols[k][4] for k in names]
    x = np.stack([cols[k][0] for k in ('nan_neighbour', 'infinite_bin', 'neighbour_at_f_valid')], axis=1)
    delta, pitch = abi_frames(x, 3, [0, 1, 2, 3], [2, 2, 2], M5, 3)
    assert delta.tolist() == [0.0, 0.0, cols['neighbour_at_f_valid'][3]] and pitch.tolist() == [60.375, 60.375, cols['neighbour_at_f_valid'][4]]
    # F = 1: no spacing
    delta, pitch = abi_frames(np.full((1, 3), 0.75, dtype=np.float32), 0, [0, 1, 2, 3], [0, 0, 0], [61.5], 3)
    assert delta.tolist() == [0.0] * 3 and pitch.tolist() == [61.5] * 3
    # the lists of mpe_compact, whole and cut short
    xm, m = smooth_map(2, 17, 130)[0], dict(random_cases())['bins_T130']['m']
    est_off, est_bins, _, _ = mpe_compact(dev(xm), THR, True, 14)
    est_off, n = est_off.cpu().numpy(), int(est_off[-1])
    est_bins = est_bins.cpu().numpy()[:n]
    want = C.refine_frames_ref(xm, est_off, est_bins, m, 14)
    for cut in (0, 7):
        delta, pitch = abi_frames(xm, 14, est_off, est_bins, m, n - cut)
        assert np.array_equal(bits(delta), bits(want[0][:n - cut])) and np.array_equal(pitch, want[1][:n - cut])
    assert n > 50


def test_abi_refusals_launch_nothing():
    lib, st = _hip.lib(), _hip.stream_ptr()
    assert lib.tt_version() >= 24
    x = smooth_map(2, 12, 65)
    B, F, T = x.shape
    a = Arena(FILL_BIG, DEV)
    a.inp('x', torch.from_numpy(np.array(x)))
    a.inp('g', torch.tensor([0, 5, 12], dtype=torch.int32))
    a.inp('m', torch.arange(12, dtype=torch.float64))
    a.inp('rp', torch.zeros(2, dtype=torch.float64))
    for name in ('item', 'row', 'onset'):
        a.inp(name, torch.zeros(4, dtype=torch.int32))
    a.inp('end', torch.full((4,), 8, dtype=torch.int32))
    a.inp('frame_off', torch.arange(0, 40, 8, dtype=torch.int64))
    a.inp('est_off', torch.arange(T + 1, dtype=torch.int64))
    a.inp('est_bins', torch.zeros(T, dtype=torch.int32))
    for name, dtype in FRAME_TYPES.items():
        a.out(name, (T,), dtype)
    for name, dtype in NOTE_TYPES.items():
        a.out(name, (4,), dtype)
    a.build()
    p = a.ptr

    def notes(B=B, F=F, T=T, mode=1, P=2, units=UNITS, n=4, **names):
        q = lambda k: p(names.get(k, k))                                           # noqa: E731
        return lib.tt_contours_notes(q('x'), B, F, T, THR, mode, 0, q('g'), P, q('m'), q('rp'), units, q('item'), q('row'), q('onset'), q('end'),
                                     n, q('frame_off'), q('bin'), q('delta'), q('value'), q('pitch'), q('bend'), q('n_voiced'), q('bend_sum'),
                                     q('bend_min'), q('bend_max'), st)

    def frames(F=F, T=T, cap=T, **names):
        q = lambda k: p(names.get(k, k))                                           # noqa: E731
        return lib.tt_contours_frames(q('x'), F, T, 0, q('est_off'), q('est_bins'), cap, q('m'), q('delta'), q('pitch'), st)

    pointers = ('x', 'g', 'm', 'rp', 'item', 'row', 'onset', 'end', 'frame_off', 'bin', 'delta', 'value', 'pitch', 'bend', 'n_voiced', 'bend_sum',
                'bend_min', 'bend_max')
    refused = [notes(B=0), notes(F=0), notes(T=0), notes(P=0), notes(mode=0), notes(mode=3), notes(units=0), notes(units=-5), notes(n=0),
               notes(n=-1)] + [notes(**{k: 'none'}) for k in pointers]
    refused += [frames(F=0), frames(T=0), frames(cap=-1)] + [frames(**{k: 'none'}) for k in ('x', 'est_off', 'est_bins', 'm', 'delta', 'pitch')]
    assert all(rc == -1 for rc in refused) and len(refused) == 37 and lib.tt_error_string(-1) == BADARG
    a.untouched('refused tt_contours_* calls')


# ---- the round trip and the public interface --------------------------------------------------------------------------------------------

def test_constant_detunings_come_back():
    x, m, semis, detune = detuned_notes()
    kw = dict(t=THR, n_valid_bins=FV)
    ev = note_events(dev(x), m, **kw)
    co = note_contours(dev(x), ev, m, **kw)
    assert ev.pitch.tolist() == semis.astype(np.float64).tolist() and torch.equal(co.n_voiced, ev.n_active)
    got = refined_pitches(ev, co)
    assert got.is_cuda and got.dtype == torch.float64
    err = np.abs(got.cpu().numpy() - (semis + detune)) * 100.0
    print('constant detunings: largest error %.3f cents' % err.max())
    assert err.max() < DETUNE_BAR_CENTS
    # a vibrato: the contour follows the centre within the same figure the reference reaches
    xr, mr, true = ridge()
    ev = note_events(dev(xr), mr)
    co = note_contours(dev(xr), ev, mr)
    assert ev.item.numel() == 1 and ridge_error_cents(co.pitch.cpu().numpy(), true) < 10.0
    assert abs(float(refined_pitches(ev, co)[0]) - true.mean()) < 0.01


def test_interface_forms_and_errors():
    c = dict(random_cases())['groups_T65']
    x, m = c['x'], c['m']
    kw = dict(t=THR, n_valid_bins=c['fv'], bin_groups=c['group_off'])
    ev = note_events(dev(x), m, max_gap=2, **kw)
    co = note_contours(dev(x), ev, m, **kw)
    one_ev = note_events(dev(x[0]), m, max_gap=2, **kw)                            # (F, T): item 0
    one = note_contours(dev(x[0]), one_ev, m, **kw)
    n0 = int((ev.item == 0).sum())
    assert one.frame_off.tolist() == co.frame_off[:n0 + 1].tolist() and torch.equal(one.bend, co.bend[:int(co.frame_off[n0])])
    for dtype in (torch.float16, torch.bfloat16):                                  # 16-bit maps are upcast
        x16 = dev(x).to(dtype)
        e16 = note_events(x16, m, max_gap=2, **kw)
        for a, b in zip(note_contours(x16, e16, m, **kw)[:-1], note_contours(x16.float(), e16, m, **kw)[:-1]):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    empty = note_contours(dev(x), note_events(torch.zeros(2, 12, 65, device=DEV), m, **kw), m, **kw)
    assert empty.frame_off.tolist() == [0] and all(f.is_cuda and f.numel() == 0 for f in empty[1:-1])
    assert [f.dtype for f in empty[:-1]] == [f.dtype for f in co[:-1]] and refined_pitches(note_events(torch.zeros(2, 12, 65, device=DEV), m), empty).numel() == 0
    with pytest.raises(RuntimeError):                                              # CPU tensor: no fallback
        note_contours(torch.from_numpy(np.array(x)), ev, m, **kw)
    with pytest.raises(ValueError):                                                # rows of another grouping
        note_contours(dev(x), ev, m, t=THR, bin_groups=np.array([0, 12]))
    with pytest.raises(ValueError):
        note_contours(dev(x), ev, m, units_per_semitone=0, **kw)
    with pytest.raises(ValueError):
        note_contours(dev(x), ev, m[:-1], **kw)
    with pytest.raises(RuntimeError):
        refine_multi_pitch(torch.from_numpy(np.array(x[0])), m)
    with pytest.raises(ValueError):
        refine_multi_pitch(dev(x[0]), m[:-1])
    # the host side: bends of one item for the writer
    frames, bends = contours_to_bends(ev, co, item=1)
    sel = (ev.item == 1).cpu().numpy()
    assert len(frames) == len(bends) == int(sel.sum()) and [len(f) for f in frames] == ev.n_active.cpu().numpy()[sel].tolist()
    assert np.array_equal(np.concatenate(bends), co.bend.cpu().numpy()[(co.bin >= 0).cpu().numpy() & np.repeat(sel, co.frame_off.diff().cpu().numpy())])


def test_transcribe_contours():
    from timbre_trap.framework import TimbreTrap
    torch.manual_seed(0)
    model = TimbreTrap(22050, 9, 60, 3, latent_size=None, model_complexity=1, skip_connections=False).cuda().eval()
    audio = torch.rand(1, 1, 66150, generator=torch.Generator().manual_seed(1)).mul(2).sub(1).cuda()
    with torch.no_grad():
        act = model.transcribe(audio)
        t = float(act.float().mean())                                              # an untrained model: a threshold its map straddles
        kw = dict(t=t, max_gap=1, min_frames=2, n_valid_bins=FV)
        ev, co = model.transcribe_contours(audio, **kw)
        want_ev = model.transcribe_notes(audio, **kw)
    assert ev.item.numel() > 0 and isinstance(co, NoteContours)
    for a, b in zip(ev, want_ev):
        assert torch.equal(a, b)
    want = note_contours(act, want_ev, model.sliCQ.midi_freqs, t=t, n_valid_bins=FV)
    for a, b in zip(co[:-1], want[:-1]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert co.units == want.units == 4096 and torch.equal(co.n_voiced, ev.n_active)
    # ... and on to a file with bends
    cqt = model.sliCQ
    times = cqt.get_times(act.shape[-1] + 1)
    frames, bends = contours_to_bends(ev, co)
    buf = io.BytesIO()
    dropped = write_midi_bends(buf, ev.pitch.cpu().numpy(), np.stack([times[ev.onset.cpu().numpy()], times[ev.end.cpu().numpy()]], 1), bends,
                               [times[f] for f in frames], ev.peak.cpu().numpy())
    assert 0 <= dropped <= ev.item.numel() and buf.getvalue()[:4] == b'MThd'
