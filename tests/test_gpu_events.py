"""
Note events on the MI355X (csrc/events.hip; timbre_trap.utils.note_events / events_to_notes / write_midi; TimbreTrap.transcribe_notes)
against the NumPy reference of tests/events_ref.py, which tests/test_events_restatement.py pins on the CPU.

Every result is an integer or an exact fp32 value of the map: every comparison below is ``==``, never a tolerance.  The pass mask the
reference is fed is the DOWNLOADED output of ``_device_pick`` (tt_peak_pick, modes 1 and 2) on the same input, so the predicate is not
derived a second time here.
"""

import io

import numpy as np
import pytest
import torch

from timbre_trap import _hip
from timbre_trap.utils import NoteEvents, events_to_notes, note_events, notes_to_activations, write_midi
from timbre_trap.utils.processing import _device_pick

from cl16_ref import FILL_BIG, Arena
from events_ref import FIELDS, note_events_ref
from test_events_restatement import (DENSITIES, F37, FV37, GAP_MIN, GROUPS37, RANDOM_T, THR, as_rows, crafted, random_map, read_midi,
                                     round_trip_case, round_trip_want)
from test_mpe_restatement import FV, MIDI_FREQS, activations

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BADARG = b'ttrap: bad argument'


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)             # a writable, contiguous copy (the cached inputs are read-only)


def device_pass(x, mode, fv=0, thr=THR):
    return _device_pick(dev(x), thr, mode, fv).cpu().numpy() > 0


def same(ev, want, what=''):
    assert isinstance(ev, NoteEvents)
    for name, w in zip(FIELDS, want):
        g = getattr(ev, name)
        assert g.is_cuda and g.dtype == (torch.float32 if name == 'peak' else torch.int32), (what, name)
        assert np.array_equal(g.cpu().numpy(), w), (what, name)
    assert ev.pitch.dtype == torch.float64 and ev.pitch.shape == ev.row.shape


def check(x, group_off, mode, fv, gap, minf, passed=None, what=''):
    passed = device_pass(x, mode, fv) if passed is None else passed
    ev = note_events(dev(x), np.arange(x.shape[1], dtype=np.float64), t=THR, peaks_only=mode == 2, n_valid_bins=fv, bin_groups=group_off,
                     max_gap=gap, min_frames=minf)
    want = note_events_ref(passed, x, group_off, gap, minf)
    same(ev, want, what)
    return ev, want


# ---- random maps ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode', (1, 2))
@pytest.mark.parametrize('n_frames', RANDOM_T)
def test_random_maps(n_frames, mode):
    n = 0
    for density in DENSITIES:
        x = random_map(density, n_frames)
        passed = device_pass(x, mode, FV37)
        for gap, minf in GAP_MIN:
            _, want = check(x, GROUPS37, mode, FV37, gap, minf, passed, (density, gap, minf))
            n += len(want[0])
    assert n > 0


# ---- crafted rows ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(crafted()))
def test_crafted_rows(name):
    c = crafted()[name]
    ev, want = check(c['x'], c['group_off'], c['mode'], c['fv'], c['gap'], c['minf'])
    assert as_rows(want) == c['want']                                              # ... and both are the literal answer
    if 'peaks' in c:
        assert list(ev.peak.cpu().numpy()) == c['peaks']


def test_alternating_row_fills_the_capacity_bound():
    c = crafted()['alternating']
    ev, _ = check(c['x'], c['group_off'], 1, 0, 0, 1)
    T = c['x'].shape[2]
    assert ev.item.numel() == -(-T // 2) == 65


# ---- the default geometry ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('resolution', ('semitone', 'bin'))
def test_both_groupings_at_540_bins(resolution):
    x = np.stack([activations(0.05, 300, seed=s) for s in (0, 1)])
    passed = device_pass(x, 2, FV)
    ev = note_events(dev(x), MIDI_FREQS, n_valid_bins=FV, resolution=resolution, max_gap=2, min_frames=2)
    semi = np.floor(MIDI_FREQS + 0.5).astype(np.int64)
    if resolution == 'semitone':
        off = np.concatenate([np.searchsorted(semi, np.arange(semi[0], semi[-1] + 1)), [540]]).astype(np.int32)
        pitch = np.arange(semi[0], semi[-1] + 1).astype(np.float64)
    else:
        off, pitch = np.arange(541, dtype=np.int32), MIDI_FREQS
    want = note_events_ref(passed, x, off, 2, 2)
    same(ev, want)
    assert len(want[0]) > 100 and np.array_equal(ev.pitch.cpu().numpy(), pitch[want[1]])


def test_more_words_than_a_grid_dimension_holds():
    """B P W = 25 x 540 x 5 = 67 500 > 65 535 words: the launches are linear in one grid dimension."""
    rng = np.random.default_rng(11)
    x = (0.45 * rng.random((25, 540, 300))).astype(np.float32)
    hit = rng.random(x.shape) < 0.004
    x[hit] = 0.9
    x[24, 539, 290:] = 0.8                                                         # the very last row of the very last item
    ev = note_events(dev(x), MIDI_FREQS, peaks_only=False, resolution='bin', max_gap=3)
    want = note_events_ref(device_pass(x, 1), x, np.arange(541, dtype=np.int32), 3, 1)
    same(ev, want)
    assert as_rows(want)[-1] == (24, 539, 290, 300, 10) and len(want[0]) > 10000


# ---- the C ABI on a guarded arena -----------------------------------------------------------------------------------------------------

def abi_run(x, group_off, mode, fv, gap, minf, capacity_cut=0):
    """The four entry points with every operand and output a window of a guarded arena (one arena per stage: the outputs of one stage are
    the bit-unchanged inputs of the next).  -> dict of host arrays."""
    lib, st = _hip.lib(), _hip.stream_ptr()
    B, F, T = x.shape
    P, W = len(group_off) - 1, (T + 63) // 64
    xt, gt = torch.from_numpy(np.array(x)), torch.from_numpy(np.array(group_off, dtype=np.int32))
    a = Arena(FILL_BIG, DEV)
    a.inp('x', xt, shift=4)
    a.inp('g', gt, shift=4)
    a.out('mask', (B * P * W,), torch.int64)
    a.build()
    assert lib.tt_events_mask(a.ptr('x'), B, F, T, THR, mode, fv, a.ptr('g'), P, a.ptr('mask'), st) == 0
    a.verify('tt_events_mask')
    mask = a.get('mask')

    a = Arena(FILL_BIG, DEV)
    a.inp('mask', mask)
    a.out('n_on', (B * P * W,), torch.int32, shift=4)
    a.out('n_end', (B * P * W,), torch.int32)
    a.build()
    assert lib.tt_events_count(a.ptr('mask'), B, P, T, gap, a.ptr('n_on'), a.ptr('n_end'), st) == 0
    a.verify('tt_events_count')
    n_on, n_end = a.get('n_on'), a.get('n_end')
    per_row = lambda n: n.view(B * P, W).sum(1)                                    # noqa: E731
    assert torch.equal(per_row(n_on), per_row(n_end))
    on_off, end_off = torch.cumsum(n_on, 0, dtype=torch.int64) - n_on, torch.cumsum(n_end, 0, dtype=torch.int64) - n_end
    total = int(n_on.sum())
    out = dict(mask=mask, n_on=n_on, n_end=n_end, total=total)
    cap = total - capacity_cut
    if cap <= 0:
        return out

    a = Arena(FILL_BIG, DEV)
    a.inp('mask', mask)
    a.inp('on_off', on_off)
    a.inp('end_off', end_off)
    for k, name in enumerate(('item', 'row', 'onset', 'end')):
        a.out(name, (cap,), torch.int32, shift=4 * (k % 2))
    a.build()
    assert lib.tt_events_fill(a.ptr('mask'), B, P, T, gap, a.ptr('on_off'), a.ptr('end_off'), cap, a.ptr('item'), a.ptr('row'),
                              a.ptr('onset'), a.ptr('end'), st) == 0
    a.verify('tt_events_fill')                                                     # every slot below the capacity written, none beyond
    out.update({n: a.get(n) for n in ('item', 'row', 'onset', 'end')})
    if capacity_cut:
        return out

    b = Arena(FILL_BIG, DEV)
    b.inp('x', xt)
    b.inp('g', gt)
    b.inp('mask', mask)
    for name in ('item', 'row', 'onset', 'end'):
        b.inp(name, out[name], shift=4)
    b.out('n_active', (total,), torch.int32)
    b.out('peak', (total,), torch.float32, shift=4)
    b.out('keep', (total,), torch.int32)
    b.build()
    assert lib.tt_events_finish(b.ptr('x'), B, F, T, THR, mode, fv, b.ptr('g'), P, b.ptr('mask'), b.ptr('item'), b.ptr('row'), b.ptr('onset'),
                                b.ptr('end'), total, minf, b.ptr('n_active'), b.ptr('peak'), b.ptr('keep'), st) == 0
    b.verify('tt_events_finish', finite=bool(np.isfinite(x).all()))
    out.update({n: b.get(n) for n in ('n_active', 'peak', 'keep')})
    return out


@pytest.mark.parametrize('mode,gap,minf', ((1, 0, 1), (2, 5, 3), (1, 63, 64)))
def test_abi_on_the_arena(mode, gap, minf):
    x = random_map(0.3, 129)
    first, second = abi_run(x, GROUPS37, mode, FV37, gap, minf), abi_run(x, GROUPS37, mode, FV37, gap, minf)
    assert first.keys() == second.keys() and first['total'] > 0
    for k in first:                                                                # bit-identical across two calls
        assert first[k] == second[k] if k == 'total' else torch.equal(first[k].view(torch.uint8), second[k].view(torch.uint8)), k
    keep = first['keep'].bool()
    got = tuple(first[n][keep].numpy() for n in FIELDS)
    want = note_events_ref(device_pass(x, mode, FV37), x, GROUPS37, gap, minf)
    for name, g, w in zip(FIELDS, got, want):
        assert np.array_equal(g, w), name
    assert torch.equal(first['keep'], (first['end'] - first['onset'] >= minf).int())
    # tail bits beyond T are zero in every row's last word (T = 129: bit 0 alone may be set)
    assert not bool((first['mask'].view(-1, 3)[:, 2] & ~1).any())


def test_abi_crafted_and_capacity():
    for name in ('nan_inf_threshold', 'neighbouring_rows_T64', 'gap_63', 'gap_64', 'alternating'):
        c = crafted()[name]
        r = abi_run(c['x'], c['group_off'], c['mode'], c['fv'], c['gap'], c['minf'])
        keep = r['keep'].bool()
        assert [tuple(int(r[n][i]) for n in FIELDS[:5]) for i in range(r['total']) if keep[i]] == c['want'], name
    c = crafted()['alternating']
    full = abi_run(c['x'], c['group_off'], 1, 0, 0, 1)
    cut = abi_run(c['x'], c['group_off'], 1, 0, 0, 1, capacity_cut=7)              # nothing at or beyond the capacity: the arena's guards
    for n in ('item', 'row', 'onset', 'end'):
        assert torch.equal(cut[n], full[n][:full['total'] - 7])


def test_abi_refusals_launch_nothing():
    lib, st = _hip.lib(), _hip.stream_ptr()
    assert lib.tt_version() >= 21
    x = random_map(0.3, 65)
    B, F, T = x.shape
    P, W = len(GROUPS37) - 1, 2
    a = Arena(FILL_BIG, DEV)
    a.inp('x', torch.from_numpy(np.array(x)))
    a.inp('g', torch.from_numpy(GROUPS37.copy()))
    for name in ('off_a', 'off_b'):
        a.inp(name, torch.zeros(B * P * W, dtype=torch.int64))
    a.out('mask', (B * P * W,), torch.int64)
    for name in ('n_on', 'n_end', 'item', 'row', 'onset', 'end', 'n_active', 'keep'):
        a.out(name, (B * P * W,), torch.int32)
    a.out('peak', (B * P * W,), torch.float32)
    a.build()
    p = a.ptr

    def mask(B=B, F=F, T=T, mode=1, P=P, x='x', g='g', m='mask'):
        return lib.tt_events_mask(p(x), B, F, T, THR, mode, 0, p(g), P, p(m), st)

    def count(B=B, P=P, T=T, gap=0, m='mask', a_='n_on', b_='n_end'):
        return lib.tt_events_count(p(m), B, P, T, gap, p(a_), p(b_), st)

    def fill(B=B, P=P, T=T, gap=0, cap=4, m='mask', oa='off_a', ob='off_b', i='item', r='row', o='onset', e='end'):
        return lib.tt_events_fill(p(m), B, P, T, gap, p(oa), p(ob), cap, p(i), p(r), p(o), p(e), st)

    def finish(B=B, F=F, T=T, mode=1, P=P, n=4, minf=1, x='x', g='g', m='mask', i='item', r='row', o='onset', e='end', na='n_active',
               pk='peak', k='keep'):
        return lib.tt_events_finish(p(x), B, F, T, THR, mode, 0, p(g), P, p(m), p(i), p(r), p(o), p(e), n, minf, p(na), p(pk), p(k), st)

    refused = [mask(B=0), mask(F=0), mask(T=0), mask(P=0), mask(mode=0), mask(mode=3), mask(x='none'), mask(g='none'), mask(m='none'),
               count(B=0), count(P=0), count(T=0), count(gap=-1), count(gap=64), count(m='none'), count(a_='none'), count(b_='none'),
               fill(B=0), fill(P=0), fill(T=0), fill(gap=-1), fill(gap=64), fill(cap=-1), fill(m='none'), fill(oa='none'), fill(ob='none'),
               fill(i='none'), fill(r='none'), fill(o='none'), fill(e='none'),
               finish(B=0), finish(F=0), finish(T=0), finish(P=0), finish(mode=0), finish(n=0), finish(minf=0), finish(x='none'),
               finish(g='none'), finish(m='none'), finish(i='none'), finish(r='none'), finish(o='none'), finish(e='none'), finish(na='none'),
               finish(pk='none'), finish(k='none')]
    assert all(rc == -1 for rc in refused) and lib.tt_error_string(-1) == BADARG
    a.untouched('refused tt_events_* calls')


# ---- the round trip with the device code that goes the other way -----------------------------------------------------------------------

def test_round_trip_through_notes_to_activations():
    case = round_trip_case()
    target = notes_to_activations(case['pitches'], case['intervals'], case['times'], MIDI_FREQS, return_tensor=True)
    assert target.dtype == torch.float64 and target.shape == (540, 300)
    ev = note_events(target.float(), MIDI_FREQS, resolution='semitone', t=0.5, peaks_only=True)
    got = list(zip(ev.row.tolist(), ev.onset.tolist(), ev.end.tolist()))
    assert got == round_trip_want(case) and len(got) == 40                          # no note lost, none split
    assert np.array_equal(ev.pitch.cpu().numpy(), np.sort(case['midi']).astype(np.float64))
    assert torch.equal(ev.n_active, ev.end - ev.onset) and bool((ev.peak == 1).all()) and not bool(ev.item.any())
    # back to the annotation's shape: onsets and offsets are the times of the spans' frames
    pitches, intervals = events_to_notes(ev, case['times'][1])
    assert pitches.dtype == np.float64 and intervals.shape == (40, 2)
    want = np.array(round_trip_want(case))
    assert np.array_equal(intervals, want[:, 1:] * case['times'][1])
    assert np.array_equal(events_to_notes(ev, (1.0, 341.0))[1], want[:, 1:] * 1.0 / 341.0)
    assert events_to_notes(ev, 0.01, item=1)[0].shape == (0,) and events_to_notes(ev, 0.01, item=1)[1].shape == (0, 2)


# ---- the public interface ---------------------------------------------------------------------------------------------------------------

def test_interface_forms_and_errors():
    x = random_map(0.3, 129)
    midi = np.arange(F37, dtype=np.float64)
    kw = dict(bin_groups=GROUPS37, max_gap=2, min_frames=2)
    ev = note_events(dev(x), midi, **kw)
    one = note_events(dev(x[1]), midi, **kw)                                       # (F, T): item 0
    sel = ev.item == 1
    assert one.item.numel() == int(sel.sum()) > 0 and not bool(one.item.any())
    for name in FIELDS[1:] + ('pitch',):
        assert torch.equal(getattr(one, name), getattr(ev, name)[sel])
    # 16-bit maps are upcast
    for dtype in (torch.float16, torch.bfloat16):
        x16 = dev(x).to(dtype)
        for a, b in zip(note_events(x16, midi, **kw), note_events(x16.float(), midi, **kw)):
            assert torch.equal(a, b)
    # order='onset': a permutation of order='pitch', per item by (onset, row)
    by_onset = note_events(dev(x), midi, order='onset', **kw)
    key = lambda e: list(zip(*(getattr(e, n).tolist() for n in NoteEvents._fields)))          # noqa: E731
    assert sorted(key(by_onset)) == sorted(key(ev)) and key(by_onset) != key(ev)
    triples = list(zip(by_onset.item.tolist(), by_onset.onset.tolist(), by_onset.row.tolist()))
    assert triples == sorted(triples)
    # two runs are identical
    for a, b in zip(note_events(dev(x), midi, **kw), ev):
        assert torch.equal(a, b)
    # nothing to find, nothing to read: empty tensors of the right types
    for empty in (note_events(torch.zeros(2, F37, 70, device=DEV), midi), note_events(torch.zeros(2, F37, 0, device=DEV), midi),
                  note_events(torch.zeros(0, F37, 9, device=DEV), midi), note_events(dev(x), midi, bin_groups=np.array([4])),
                  note_events(dev(x), midi, max_gap=63, min_frames=10 ** 6)):
        assert all(f.is_cuda and f.numel() == 0 for f in empty)
        assert [f.dtype for f in empty] == [torch.int32] * 5 + [torch.float32, torch.float64]
    with pytest.raises(RuntimeError):                                              # CPU tensor: no fallback
        note_events(torch.from_numpy(np.array(x)), midi)
    with pytest.raises(RuntimeError):
        note_events(np.array(x), midi)
    for bad in (dict(max_gap=-1), dict(max_gap=64), dict(min_frames=0), dict(order='time'), dict(resolution='octave'),
                dict(bin_groups=np.array([5, 3])), dict(bin_groups=np.array([0, F37 + 1]))):
        with pytest.raises(ValueError):
            note_events(dev(x), midi, **bad)
    with pytest.raises(ValueError):
        note_events(dev(x).double(), midi)
    with pytest.raises(ValueError):
        note_events(dev(x), midi[:-1])


def test_transcribe_notes_and_midi_file(tmp_path):
    from timbre_trap.framework import TimbreTrap
    torch.manual_seed(0)
    model = TimbreTrap(22050, 9, 60, 3, latent_size=None, model_complexity=1, skip_connections=False).cuda().eval()
    audio = torch.rand(1, 1, 66150, generator=torch.Generator().manual_seed(1)).mul(2).sub(1).cuda()
    with torch.no_grad():
        act = model.transcribe(audio)
        t = float(act.float().mean())                                              # an untrained model: a threshold its map straddles
        kw = dict(t=t, max_gap=1, min_frames=2, n_valid_bins=FV)
        ev = model.transcribe_notes(audio, **kw)
    want = note_events(act, model.sliCQ.midi_freqs, **kw)
    assert ev.item.numel() > 0
    for a, b in zip(ev, want):
        assert torch.equal(a, b)
    same(ev, note_events_ref(device_pass(act.cpu().numpy(), 2, FV, t), act.cpu().numpy(), _semitone_offsets(model.sliCQ.midi_freqs), 1, 2))
    by_onset = model.transcribe_notes(audio, order='onset', **kw)
    pairs = list(zip(by_onset.onset.tolist(), by_onset.row.tolist()))
    assert pairs == sorted(pairs) and sorted(by_onset.row.tolist()) == sorted(ev.row.tolist())
    # to the annotation's arrays, to a MIDI file, and back through the reader: the same ticks
    cqt = model.sliCQ
    pitches, intervals = events_to_notes(by_onset, (cqt.hop_length, cqt.sample_rate))
    assert np.array_equal(intervals[:, 0], cqt.get_times(act.shape[-1] + 1)[by_onset.onset.cpu().numpy()])
    assert np.array_equal(intervals[:, 1], cqt.get_times(act.shape[-1] + 1)[by_onset.end.cpu().numpy()])
    path = tmp_path / 'clip.mid'
    data = write_midi(str(path), pitches, intervals, by_onset.peak.cpu().numpy())
    tpb, tempo, events = read_midi(path.read_bytes())
    assert path.read_bytes() == data == write_midi(io.BytesIO(), pitches, intervals, by_onset.peak.cpu().numpy())
    ticks = np.rint(intervals * 480 * 120 / 60.0).astype(np.int64)                     # the writer's expression at its defaults
    assert (tpb, tempo) == (480, 500000) and len(events) == 2 * len(pitches)
    assert sorted(e[0] for e in events if e[1] == 'on') == sorted(ticks[:, 0].tolist())
    assert sorted(e[0] for e in events if e[1] == 'off') == sorted(ticks[:, 1].tolist())
    assert sorted(e[2] for e in events if e[1] == 'on') == sorted(int(p) for p in np.clip(np.rint(pitches), 0, 127))


def _semitone_offsets(midi_freqs):
    semi = np.floor(np.asarray(midi_freqs, dtype=np.float64) + 0.5).astype(np.int64)
    return np.concatenate([np.searchsorted(semi, np.arange(semi[0], semi[-1] + 1)), [len(semi)]]).astype(np.int32)
