"""
Note-level scoring on the MI355X (csrc/notescore.hip; timbre_trap.utils.note_counts_device / note_metrics_device;
MultipitchEvaluator.evaluate_events) against the host yardstick ``note_counts``, which tests/test_notescore_restatement.py pins on
the CPU.  Every result is an integer: every comparison below is ``==``, never a tolerance.
"""

import numpy as np
import pytest
import torch

from timbre_trap import _hip
from timbre_trap.utils import (DeviceNoteCounts, MultipitchEvaluator, events_to_notes, note_counts, note_counts_device,
                               note_events, note_metrics, note_metrics_device, notes_to_activations)
from timbre_trap.utils import metrics

from cl16_ref import FILL_BIG, Arena
from notescore_ref import chain, clique, crafted, random_cases, random_notes
from test_events_restatement import round_trip_case
from test_mpe_restatement import MIDI_FREQS

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BADARG = b'ttrap: bad argument'


def four(cases):
    """Cases (one per item) -> the two device forms (item int32, pitch, onset, offset float64): (est, ref)."""
    out = []
    for side in (2, 0):
        item = np.concatenate([np.full(len(c[side]), b, dtype=np.int32) for b, c in enumerate(cases)])
        p = np.concatenate([c[side] for c in cases])
        iv = np.concatenate([c[side + 1] for c in cases])
        out.append(tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (item, p, iv[:, 0], iv[:, 1])))
    return out


def host(cases, **tol):
    return [note_counts(*c, **tol) for c in cases]


def same(got, want, n_fallback=0):
    assert isinstance(got, DeviceNoteCounts) and got.n_fallback == n_fallback
    for name in ('n_ref', 'n_est', 'tp', 'tp_no_offset'):
        g = getattr(got, name)
        assert g.is_cuda and g.dtype == torch.int64 and g.shape == (len(want),), name
        assert g.tolist() == [getattr(w, name) for w in want], name


def score(cases, n_fallback=0, **tol):
    est, ref = four(cases)
    got = note_counts_device(est, ref, n_items=len(cases), **tol)
    same(got, host(cases, **tol), n_fallback)
    # the reference as host lists, uploaded by the front: the same integers
    again = note_counts_device(est, [(c[0], c[1]) for c in cases], **tol)
    same(again, host(cases, **tol), n_fallback)
    return got


# ---- random cases ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(random_cases()))
def test_random_cases_one_item(name):
    case = random_cases()[name]
    got = score([case])
    if len(case[0]) >= 100:
        assert 0 < int(got.tp[0]) < int(got.tp_no_offset[0]) < len(case[0])
    score([case], onset_tolerance=0.02, pitch_tolerance=0.25, offset_ratio=0.1, offset_min_tolerance=0.02)


@pytest.mark.parametrize('name', ('n300_len3', 'n1500_len4.5'))
def test_three_items_sharing_times_and_pitches(name):
    """The items hold the same notes, thinned differently: a pair across items would change the counts."""
    ref_p, ref_iv, est_p, est_iv = random_cases()[name]
    cases = [(ref_p, ref_iv, est_p, est_iv), (ref_p, ref_iv, est_p[::2], est_iv[::2]), (ref_p[::2], ref_iv[::2], est_p, est_iv)]
    got = score(cases)
    assert len(set(got.tp_no_offset.tolist())) == 3
    # an item without estimates between two that have them, and one without references
    none = np.empty(0), np.empty((0, 2))
    score([cases[0], (ref_p, ref_iv) + none, cases[1], none + (est_p, est_iv)])


# ---- crafted cases --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(crafted()))
def test_crafted_cases(name):
    case, want = crafted()[name]
    got = score([case])
    assert (int(got.tp[0]), int(got.tp_no_offset[0])) == want
    est, ref = four([case])
    assert note_metrics_device(est, ref, n_items=1) == [note_metrics(*case)]


def test_all_crafted_cases_as_one_batch():
    cases = [c for _, (c, _) in sorted(crafted().items())]
    got = score(cases)
    assert list(zip(got.tp.tolist(), got.tp_no_offset.tolist())) == [w for _, (_, w) in sorted(crafted().items())]
    est, ref = four(cases)
    assert note_metrics_device(est, ref, n_items=len(cases)) == [note_metrics(*c) for c in cases]
    no = note_counts_device(est, ref, n_items=len(cases), offset_ratio=None)
    assert no.tp is None and torch.equal(no.tp_no_offset, got.tp_no_offset)
    keys = sorted(note_metrics(*cases[0], offset_ratio=None))
    assert all(sorted(d) == keys for d in note_metrics_device(est, ref, n_items=len(cases), offset_ratio=None))


# ---- components at and beyond the capacity --------------------------------------------------------------------------------------------

def test_chain_on_the_device_and_by_the_fallback():
    got = score([chain(60)])
    assert (int(got.tp[0]), int(got.tp_no_offset[0])) == (30, 30)
    got = score([chain(400)], n_fallback=1)
    assert (int(got.tp[0]), int(got.tp_no_offset[0])) == (200, 200)
    # the long chain between two items that stay on the device: only it goes to the host
    score([random_notes(300, 3.0), chain(400), chain(60)], n_fallback=1)


def test_clique_at_and_over_the_capacity():
    cap = _hip.lib().tt_notescore_max()
    assert cap == metrics.NOTESCORE_MAX >= 64
    got = score([clique(cap, cap)])
    assert int(got.tp_no_offset[0]) == cap and 0 < int(got.tp[0]) < cap
    score([clique(cap, cap + 1)], n_fallback=1)
    score([clique(cap + 1, cap)], n_fallback=1)


def test_labels_that_do_not_settle_go_to_the_host(monkeypatch):
    """The chain of 60 needs five rounds; allowed two, its item is counted by the host function; the item beside it, whose components
    are pairs, has settled by then and is not."""
    monkeypatch.setattr(metrics.notescore, 'NOTESCORE_ROUNDS', 2)             # the module whose global _note_counts_device reads
    score([chain(60), crafted()['pitch_boundary'][0]], n_fallback=1)


# ---- NoteEvents -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('hop', ('seconds', 'int_pair', 'float_pair'))
def test_round_trip_and_both_orders_of_note_events(hop):
    case = round_trip_case()
    hop = {'seconds': case['times'][1], 'int_pair': (1, 341.0), 'float_pair': (1.0, 341.0)}[hop]
    target = notes_to_activations(case['pitches'], case['intervals'], case['times'], MIDI_FREQS, return_tensor=True).float()
    maps = torch.stack([target, torch.roll(target, 7, dims=1)])                     # item 1: every note 7 frames late
    ref = [(case['midi'].astype(np.float64), case['intervals'])] * 2
    results = []
    for order in ('pitch', 'onset'):
        ev = note_events(maps, MIDI_FREQS, order=order)
        got = note_counts_device(ev, ref, hop_seconds=hop)
        want = [note_counts(ref[b][0], ref[b][1], *events_to_notes(ev, hop, item=b)) for b in (0, 1)]
        same(got, want)
        results.append(got)
    for a, b in zip(results[0][:4], results[1][:4]):
        assert torch.equal(a, b)
    # frames are 2.9 ms and the annotation sits within half a frame of them: item 0 comes back whole
    assert results[0].n_ref.tolist() == [40, 40] and int(results[0].tp_no_offset[0]) == 40 and int(results[0].tp[0]) == 40
    ev = note_events(maps, MIDI_FREQS)
    tracker = MultipitchEvaluator()
    for b in (0, 1):
        scores = tracker.evaluate_events(ev, hop, *ref[b], item=b)
        want = note_metrics(ref[b][0], ref[b][1], *events_to_notes(ev, hop, item=b))
        assert scores == {'note/' + k.lower(): v for k, v in want.items()} and len(scores) == 6
        tracker.append_results(scores)
    assert tracker.results['note/recall_no_offset'][0] == 1.0 and len(tracker.average_results()[0]) == 6


# ---- the interface --------------------------------------------------------------------------------------------------------------------

def test_two_runs_are_bit_equal_and_input_order_does_not_matter():
    cases = [random_notes(1500, 4.5), random_notes(1000, 3.0)]
    est, ref = four(cases)
    a, b = note_counts_device(est, ref), note_counts_device(est, ref, n_items=2)
    g = torch.Generator().manual_seed(3)
    pe, pr = torch.randperm(est[0].numel(), generator=g).to(DEV), torch.randperm(ref[0].numel(), generator=g).to(DEV)
    c = note_counts_device(tuple(t[pe] for t in est), tuple(t[pr] for t in ref), n_items=2)
    for x, y, z in zip(a[:4], b[:4], c[:4]):
        assert torch.equal(x, y) and torch.equal(x, z)
    same(a, host(cases))


def test_interface_errors():
    est, ref = four([random_notes(100, 5.0)])
    with pytest.raises(RuntimeError):                                              # CPU tensors: no fallback
        note_counts_device(tuple(t.cpu() for t in est), ref)
    with pytest.raises(RuntimeError):
        note_counts_device(tuple(t.cpu().numpy() for t in est), ref)
    with pytest.raises(ValueError):
        note_counts_device((est[0].long(),) + est[1:], ref)
    with pytest.raises(ValueError):
        note_counts_device((est[0], est[1].float()) + est[2:], ref)
    with pytest.raises(ValueError):
        note_counts_device((est[0][:-1],) + est[1:], ref)
    with pytest.raises(ValueError):
        note_counts_device(est, ref, n_items=0)
    ev = note_events(torch.zeros(1, 540, 8, device=DEV), MIDI_FREQS)
    with pytest.raises(ValueError):                                                # NoteEvents need a hop
        note_counts_device(ev, ref)
    got = note_counts_device(ev, ref, hop_seconds=0.01)                            # no estimate at all
    assert got.n_est.tolist() == [0] and got.tp.tolist() == [0] and got.n_ref.tolist() == [100]


# ---- the C ABI on a guarded arena -----------------------------------------------------------------------------------------------------

def sorted_four(p, iv):
    order = np.argsort(iv[:, 0], kind='stable')
    return [torch.zeros(len(p), dtype=torch.int32)] + [torch.from_numpy(np.ascontiguousarray(a[order])) for a in (p, iv[:, 0], iv[:, 1])]


def abi_counts(case, rounds=16):
    """The five entry points, every operand and result a window of a guarded arena.  One item.  -> (n_ref, n_est, tp, tp_no, flag)."""
    lib, st = _hip.lib(), _hip.stream_ptr()
    r, e = sorted_four(case[0], case[1]), sorted_four(case[2], case[3])
    R, E = len(case[0]), len(case[2])
    N = R + E
    seg_r, seg_e = torch.tensor([0, R]), torch.tensor([0, E])

    def arena(**extra):
        a = Arena(FILL_BIG, DEV)
        for side, t in (('r', r), ('e', e)):
            for k, name in enumerate(('item', 'p', 'on', 'off')):
                a.inp(side + name, t[k], shift=8 * (k % 2))
        a.inp('seg_r', seg_r)
        a.inp('seg_e', seg_e)
        for name, t in extra.items():
            a.inp(name, t)
        return a

    a = arena()
    a.out('lo', (N,), torch.int32, shift=4)
    a.out('hi', (N,), torch.int32)
    a.build()
    p = a.ptr
    assert lib.tt_notescore_ranges(p('ritem'), p('ron'), R, p('eitem'), p('eon'), E, p('seg_r'), p('seg_e'), 1, 0.05, p('lo'), p('hi'), st) == 0
    a.verify('tt_notescore_ranges')
    lo, hi = a.get('lo'), a.get('hi')
    assert bool((lo >= 0).all()) and bool((hi >= lo).all()) and int(hi[:R].max()) <= E and int(hi[R:].max()) <= R

    label = torch.arange(N, dtype=torch.int32)
    for rnd in range(rounds):
        a = arena(lo=lo, hi=hi, label=label)
        a.out('next', (N,), torch.int32, shift=4)
        a.acc('changed', torch.zeros(1, dtype=torch.int32))
        a.acc('mark', torch.zeros(1, dtype=torch.int32))
        a.build()
        p = a.ptr
        assert lib.tt_notescore_labels(p('ritem'), p('rp'), p('ron'), R, p('eitem'), p('ep'), p('eon'), E, p('lo'), p('hi'), 0.05, 0.5,
                                       p('label'), p('next'), p('changed'), p('mark'), 1, rnd + 1, st) == 0
        a.verify('tt_notescore_labels')
        nxt = a.get('next')
        assert bool((nxt <= label).all()) and bool((nxt >= 0).all())
        moved = not torch.equal(nxt, label)
        assert int(a.get('changed')) == int(moved) and int(a.get('mark')) == (rnd + 1 if moved else 0)
        label = nxt
        if not moved:
            break
    else:
        raise AssertionError('labels did not settle in %d rounds' % rounds)

    r_lab, r_perm = torch.sort(label[:R], stable=True)
    e_lab, e_perm = torch.sort(label[R:], stable=True)
    a = arena(label=label, r_lab=r_lab, r_perm=r_perm.int(), e_lab=e_lab, e_perm=e_perm.int())
    a.out('tp', (R,), torch.int32)
    a.out('tp_no', (R,), torch.int32, shift=4)
    a.acc('flag', torch.zeros(1, dtype=torch.int32))
    a.build()
    p = a.ptr
    assert lib.tt_notescore_match(p('label'), p('r_lab'), p('r_perm'), p('e_lab'), p('e_perm'), p('ritem'), p('rp'), p('ron'), p('roff'), R,
                                  p('ep'), p('eon'), p('eoff'), E, 0.05, 0.5, 0.2, 0.05, p('tp'), p('tp_no'), p('flag'), 1, st) == 0
    a.verify('tt_notescore_match')
    tp, tp_no, flag = a.get('tp'), a.get('tp_no'), a.get('flag')
    roots = label[:R] == torch.arange(R, dtype=torch.int32)
    assert not bool(tp[~roots].any()) and not bool(tp_no[~roots].any())

    a = Arena(FILL_BIG, DEV)
    for name, t in (('tp', tp), ('tp_no', tp_no), ('seg_r', seg_r), ('seg_e', seg_e), ('flag', flag)):
        a.inp(name, t)
    a.out('sums', (1, 5), torch.int64)
    a.build()
    p = a.ptr
    assert lib.tt_notescore_sums(p('tp'), p('tp_no'), R, E, p('seg_r'), p('seg_e'), p('flag'), 1, p('sums'), st) == 0
    a.verify('tt_notescore_sums')
    return tuple(a.get('sums')[0].tolist())


@pytest.mark.parametrize('name', ('n100_len5', 'n1000_len3'))
def test_abi_on_the_arena(name):
    case = random_cases()[name]
    want = note_counts(*case)
    assert abi_counts(case) == tuple(want) + (0,)


def test_abi_on_the_arena_crafted():
    for name in ('path_9_edges', 'nan_times', 'inf_times', 'chain_60', 'offset_not_a_subset'):
        case, want = crafted()[name]
        assert abi_counts(case)[2:] == want + (0,), name
    cap = _hip.lib().tt_notescore_max()
    assert abi_counts(clique(cap, cap + 1)) == (cap, cap + 1, 0, 0, 1)              # over the capacity: flagged, nothing counted


def test_abi_times():
    lib, st = _hip.lib(), _hip.stream_ptr()
    frames = torch.tensor([0, 1, 7, 300, 2 ** 31 - 1], dtype=torch.int32)
    a = Arena(FILL_BIG, DEV)
    a.inp('on', frames)
    a.inp('end', frames.flip(0).contiguous(), shift=4)
    a.out('t0', (5,), torch.float64)
    a.out('t1', (5,), torch.float64, shift=8)
    a.build()
    assert lib.tt_notescore_times(a.ptr('on'), a.ptr('end'), 5, 256, 1.0, 22050.0, a.ptr('t0'), a.ptr('t1'), st) == 0
    a.verify('tt_notescore_times')
    want = frames.numpy().astype(np.int64) * 256 / 22050.0                          # the expression of events_to_notes
    assert np.array_equal(a.get('t0').numpy(), want) and np.array_equal(a.get('t1').numpy(), want[::-1])


def test_abi_refusals_launch_nothing():
    lib, st = _hip.lib(), _hip.stream_ptr()
    assert lib.tt_version() >= 23
    n = 8
    a = Arena(FILL_BIG, DEV)
    for name in ('i0', 'i1', 'i2', 'i3', 'i4'):
        a.inp(name, torch.zeros(n, dtype=torch.int32))
    for name in ('d0', 'd1', 'd2'):
        a.inp(name, torch.zeros(n, dtype=torch.float64))
    a.inp('seg', torch.tensor([0, n]))
    for name in ('o0', 'o1', 'o2'):
        a.out(name, (n,), torch.int32)
    a.out('od0', (n,), torch.float64)
    a.out('od1', (n,), torch.float64)
    a.out('sums', (1, 5), torch.int64)
    a.build()
    p = a.ptr
    big = 2 ** 31

    def times(on='i0', end='i1', n=n, t0='od0', t1='od1'):
        return lib.tt_notescore_times(p(on), p(end), n, 1, 0.01, 1.0, p(t0), p(t1), st)

    def ranges(ri='i0', ro='d0', R=n, ei='i1', eo='d1', E=n, sr='seg', se='seg', B=1, lo='o0', hi='o1'):
        return lib.tt_notescore_ranges(p(ri), p(ro), R, p(ei), p(eo), E, p(sr), p(se), B, 0.05, p(lo), p(hi), st)

    def labels(ri='i0', rp='d0', ro='d1', R=n, ei='i1', ep='d0', eo='d1', E=n, lo='i2', hi='i3', li='i4', out='o0', ch='o1', mk='o2', B=1):
        return lib.tt_notescore_labels(p(ri), p(rp), p(ro), R, p(ei), p(ep), p(eo), E, p(lo), p(hi), 0.05, 0.5, p(li), p(out), p(ch), p(mk), B,
                                       1, st)

    def match(lab='i0', rl='i1', rp_='i2', el='i3', ep_='i4', ri='i0', rp='d0', ro='d1', rf='d2', R=n, ep='d0', eo='d1', ef='d2', E=n, tp='o0',
              tn='o1', fl='o2', B=1):
        return lib.tt_notescore_match(p(lab), p(rl), p(rp_), p(el), p(ep_), p(ri), p(rp), p(ro), p(rf), R, p(ep), p(eo), p(ef), E, 0.05, 0.5,
                                      0.2, 0.05, p(tp), p(tn), p(fl), B, st)

    def sums(tp='i0', tn='i1', R=n, E=n, sr='seg', se='seg', fl='i2', B=1, out='sums'):
        return lib.tt_notescore_sums(p(tp), p(tn), R, E, p(sr), p(se), p(fl), B, p(out), st)

    refused = [times(on='none'), times(end='none'), times(n=0), times(n=big), times(t0='none'), times(t1='none'),
               ranges(ri='none'), ranges(ro='none'), ranges(R=0), ranges(ei='none'), ranges(eo='none'), ranges(E=0), ranges(R=big - n),
               ranges(sr='none'), ranges(se='none'), ranges(B=0), ranges(lo='none'), ranges(hi='none'),
               labels(ri='none'), labels(rp='none'), labels(ro='none'), labels(R=0), labels(ei='none'), labels(ep='none'), labels(eo='none'),
               labels(E=0), labels(E=big), labels(lo='none'), labels(hi='none'), labels(li='none'), labels(out='none'), labels(out='i4'),
               labels(ch='none'), labels(mk='none'), labels(B=0),
               match(lab='none'), match(rl='none'), match(rp_='none'), match(el='none'), match(ep_='none'), match(ri='none'), match(rp='none'),
               match(ro='none'), match(rf='none'), match(R=0), match(ep='none'), match(eo='none'), match(ef='none'), match(E=0),
               match(R=big), match(tp='none'), match(tn='none'), match(fl='none'), match(B=0),
               sums(tp='none'), sums(tn='none'), sums(R=0), sums(E=0), sums(sr='none'), sums(se='none'), sums(fl='none'), sums(B=0),
               sums(out='none')]
    assert all(rc == -1 for rc in refused) and lib.tt_error_string(-1) == BADARG
    a.untouched('refused tt_notescore_* calls')
