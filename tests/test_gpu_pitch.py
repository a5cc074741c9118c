"""
Frame-level pitch annotations on the MI355X (csrc/pitch.hip; timbre_trap.utils.PitchBank / pitch_to_activations /
multipitch_counts_device_track / MultipitchEvaluator.evaluate_track) against the host route -- ``resample_multi_pitch``, then the existing
``multi_pitch_to_activations`` / ``evaluate_activations`` on its lists -- and against the reference's recorded target maps
(tests/golden/pitch.npz; tests/test_pitch_restatement.py pins the host side to them without a GPU).

Nothing rounds differently on the two sides: every comparison is ``array_equal`` / ``torch.equal`` / ``==``, never a tolerance.
Sizes come from the library: T = 2 tt_pitch_tile_frames() + 37 frames (two full tiles and a ragged one) and T = 1; F = 540 and F = 1;
one bin or one blur radius more than the kernels hold takes the list route.
"""

import functools
import types

import numpy as np
import pytest
import torch

from timbre_trap import _hip
from timbre_trap.utils import (MultipitchEvaluator, PitchBank, multi_pitch_to_activations, multipitch_counts_device,
                               multipitch_counts_device_track, multipitch_metrics_device, multipitch_metrics_device_track, pitch_tiles,
                               pitch_to_activations, slice_times)
from timbre_trap.utils.slicing import nearest_indices
from timbre_trap.utils.targets import _gaussian_weights

from test_mpe_restatement import FV, MIDI_FREQS, activations, est_times
from test_pitch_restatement import READ_LOST, UNREAD_LOST, caught, expanded_pairs, golden_tracks, lists_route, second_track

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BLURS = (2.5, 0, 5.0)
DTYPES = (torch.float64, torch.float32)
IDCS = [3, -2]
T_EST = 300


def n_frames():
    return 2 * pitch_tiles()[0] + 37


def fixture_track(tag='a'):
    sets, _, _ = golden_tracks()
    return sets[tag]['source_times'], sets[tag]['lists']


@functools.lru_cache(maxsize=None)
def bank_of_two():
    """Track 0: the fixture's variant a; track 1: the short one.  Real 540-bin grid, resample_idcs [3, -2]."""
    _, _, midi_freqs = golden_tracks()
    return PitchBank([fixture_track('a'), second_track()], midi_freqs, IDCS, DEV)


@functools.lru_cache(maxsize=None)
def batch_items(T):
    """Four items of T frames from two tracks: (track ids, times (4, T)) --
    0: track 0, the fixture's own first T targets (the -inf padding, the midpoints, the frame with the lost pitch: it warns);
    1: track 0 on a regular grid over the later part of the track (reads neither lost frame);
    2: track 1 over its silent frames only (nothing painted);
    3: track 1, shorter than the item, padded by slice_times with -inf in front and +inf behind."""
    _, times, _ = golden_tracks()
    src = fixture_track()[0]
    t2 = second_track()[0]
    grid = types.SimpleNamespace(hop_length=128, sample_rate=22050)                # 5.8 ms a frame, like the second track
    padded, _ = slice_times(np.array(t2), T, -7 * 128 / 22050, cqt=grid, sample_rate=22050) if T > len(t2) else (np.array(t2[:T]), 0)
    rows = [np.resize(times, T), np.linspace(src[130], src[-1] + 0.02, T), np.linspace(t2[4], t2[18], T), padded]
    out = np.stack(rows)
    out.setflags(write=False)
    return np.array([0, 0, 1, 1]), out


@functools.lru_cache(maxsize=None)
def host_item(T, b, blur):
    """The host route on item b of batch_items(T), once: (read-only float64 ndarray, warned)."""
    ids, times = batch_items(T)
    bank = bank_of_two()
    tr = bank.tracks[ids[b]]
    out, warned = caught(lambda: multi_pitch_to_activations(lists_route(tr, times[b], IDCS), bank.midi_freqs, blur, DEV))
    out.setflags(write=False)
    return out, warned


def host_batch(T, blur):
    items = [host_item(T, b, blur) for b in range(4)]
    return np.stack([m for m, _ in items]), [w for _, w in items]


def test_constants_and_scratch():
    tile, max_bins, max_radius = pitch_tiles()
    lib = _hip.lib()
    assert tile >= 64 and tile % 64 == 0 and max_bins >= 540 and max_radius >= _gaussian_weights(2.0)[1] == 8
    assert lib.tt_pitch_scratch_bytes(0, 5) == 0 and lib.tt_pitch_scratch_bytes(4, n_frames()) >= 4 * 3 * 12
    assert lib.tt_version() >= 14


def test_nearest_is_the_host_rule():
    """tt_pitch_nearest through the C ABI into a sentinel-filled buffer, against nearest_indices: the fixture's targets (midpoints,
    duplicates, -inf / +inf padding, outside the span), a NaN, a track of one frame, the short track."""
    _, times, midi_freqs = golden_tracks()
    one = (np.array([0.5]), [np.array([440.0])])
    bank = PitchBank([fixture_track('a'), one, second_track()], midi_freqs, None, DEV)
    T = len(times)
    tgt = np.stack([times, times, times, times])
    tgt[1, 100] = np.nan
    tgt[2] = np.linspace(0.4, 0.6, T)
    tgt[2, 7], tgt[2, 8], tgt[2, 9] = 0.5, np.nan, -np.inf
    tgt[3] = np.linspace(0.2, 0.6, T)
    track = np.array([0, 0, 1, 2], dtype=np.int32)
    lib = _hip.lib()
    idx = torch.full((4 * T + 8,), -7, dtype=torch.int32, device=DEV)
    tgt_d, track_d = torch.from_numpy(tgt).to(DEV), torch.from_numpy(track).to(DEV)
    _hip.check(lib.tt_pitch_nearest(_hip.ptr(bank.times_d), _hip.ptr(bank.table_d), len(bank), _hip.ptr(track_d), _hip.ptr(tgt_d), 4, T,
                                    _hip.ptr(idx), _hip.stream_ptr()))
    got = idx.cpu().numpy()
    assert (got[4 * T:] == -7).all()
    got = got[:4 * T].reshape(4, T)
    for b, n in enumerate(track):
        src = bank.track_times(n)
        below, above = bank.host['table'][n, 2:]
        assert np.array_equal(got[b], nearest_indices(src, tgt[b], below, above)), b
    sets, _, _ = golden_tracks()
    assert np.array_equal(got[0], sets['b']['idx'])                                # [0, -1]: what the reference's interp1d returned
    assert got[1, 100] == 199 and (got[2] == 0).all()
    # a track id that names no track reads nothing
    bad = torch.tensor([7], dtype=torch.int32, device=DEV)
    _hip.check(lib.tt_pitch_nearest(_hip.ptr(bank.times_d), _hip.ptr(bank.table_d), len(bank), _hip.ptr(bad), _hip.ptr(tgt_d), 1, T,
                                    _hip.ptr(idx), _hip.stream_ptr()))
    assert bool((idx[:T] == -1).all()) and np.array_equal(idx[T:2 * T].cpu().numpy(), got[1])


@pytest.mark.parametrize('blur', (2.5, 0))
def test_targets_entry_is_the_pair_entry(blur):
    """tt_pitch_targets through the C ABI against tt_target_activations on every item's expanded (bin, frame) pairs."""
    T = n_frames()
    ids, times = batch_items(T)
    bank = bank_of_two()
    lib, F, B = _hip.lib(), len(bank.midi_freqs), len(ids)
    radius, w_d = 0, None
    if blur:
        w, radius = _gaussian_weights((2 * blur) / 5)
        w_d = torch.from_numpy(w).to(DEV)
    idx = np.stack([nearest_indices(bank.track_times(n), times[b], *bank.host['table'][n, 2:]) for b, n in enumerate(ids)]).astype(np.int32)
    idx_d, ids_d = torch.from_numpy(idx).to(DEV), torch.from_numpy(ids.astype(np.int32)).to(DEV)
    want, want_flags = [], []
    for b, n in enumerate(ids):
        bins, frames, lost = expanded_pairs(bank.host, n, idx[b])
        work = torch.full((F, T), 3.0, dtype=torch.float64, device=DEV)
        out = torch.full((F, T), 3.0, dtype=torch.float64, device=DEV)
        r = radius if len(bins) else 0
        b_d, f_d = (torch.from_numpy(bins).to(DEV), torch.from_numpy(frames).to(DEV)) if len(bins) else (None, None)
        _hip.check(lib.tt_target_activations(_hip.ptr(b_d), _hip.ptr(f_d), len(bins), _hip.ptr(w_d), r, F, T, _hip.ptr(work), _hip.ptr(out),
                                             _hip.stream_ptr()))
        want.append(out)
        want_flags.append(int(lost))
    want = torch.stack(want)
    assert want_flags == [1, 0, 0, 0] and not bool(want[2].any()) and float(want.max()) == 1.0
    for dtype in DTYPES:
        out = torch.full((B * F * T + 16,), 3.0, dtype=dtype, device=DEV)
        flags = torch.full((B + 2,), -7, dtype=torch.int32, device=DEV)
        scratch = torch.empty(lib.tt_pitch_scratch_bytes(B, T) // 8 + 1, dtype=torch.float64, device=DEV)
        _hip.check(lib.tt_pitch_targets(_hip.ptr(idx_d), _hip.ptr(bank.table_d), len(bank), _hip.ptr(ids_d), B, T, _hip.ptr(bank.row_off_d),
                                        _hip.ptr(bank.bins_d), _hip.ptr(bank.lost_d), _hip.ptr(w_d), radius, F, int(dtype == torch.float32),
                                        _hip.ptr(scratch), _hip.ptr(out), _hip.ptr(flags), _hip.stream_ptr()))
        assert bool((out[B * F * T:] == 3.0).all()) and flags.tolist() == want_flags + [-7, -7]
        assert torch.equal(out[:B * F * T].view(B, F, T), want.to(dtype))
    # over a capacity: refused before anything is launched
    _, max_bins, max_radius = pitch_tiles()
    for f, r in ((max_bins + 1, radius), (F, max_radius + 1)):
        assert lib.tt_pitch_targets(_hip.ptr(idx_d), _hip.ptr(bank.table_d), len(bank), _hip.ptr(ids_d), B, T, _hip.ptr(bank.row_off_d),
                                    _hip.ptr(bank.bins_d), _hip.ptr(bank.lost_d), _hip.ptr(w_d), r, f, 0, _hip.ptr(scratch), _hip.ptr(out),
                                    _hip.ptr(flags), _hip.stream_ptr()) == -1


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('tag', ('a', 'b'))
def test_targets_are_the_reference_maps(tag, dtype):
    sets, times, midi_freqs = golden_tracks()
    s = sets[tag]
    bank = PitchBank([fixture_track(tag)], midi_freqs, s['idcs'], DEV)
    for blur, key in ((2.5, 'act_blur'), (0, 'act_noblur')):
        got, warned = caught(lambda: bank.targets(0, np.array(times), blur, dtype))
        assert got.is_cuda and got.dtype == dtype and got.shape == (540, 300)
        assert torch.equal(got.cpu(), torch.from_numpy(np.array(s[key])).to(dtype))
        assert warned == s['warned'] == bool(bank.last_lost[0]) and bank.last_lost.shape == (1,)
        if dtype == torch.float64:
            one, warned = caught(lambda: pitch_to_activations(s['source_times'], list(s['lists']), np.array(times), midi_freqs, s['idcs'],
                                                              blur, DEV))
            assert isinstance(one, np.ndarray) and one.dtype == np.float64 and np.array_equal(one, s[key]) and warned == s['warned']
    # a wider blur than the fixture records: the host route is the yardstick
    want, want_warned = caught(lambda: multi_pitch_to_activations(lists_route((s['source_times'], s['lists']), times, s['idcs']), midi_freqs,
                                                                  5.0, DEV))
    got, warned = caught(lambda: bank.targets(0, np.array(times), 5.0, dtype))
    assert torch.equal(got.cpu(), torch.from_numpy(want).to(dtype)) and warned == want_warned == s['warned']
    one, warned = caught(lambda: pitch_to_activations(s['source_times'], list(s['lists']), np.array(times), midi_freqs, s['idcs'], 5.0, DEV,
                                                      return_tensor=True))
    assert one.is_cuda and one.dtype == torch.float64 and np.array_equal(one.cpu().numpy(), want) and warned == s['warned']
    assert s['warned'] == (tag == 'a')                                             # b still holds the lost pitch nobody reads
    assert bank.host['lost'][UNREAD_LOST] == 1 and bool(bank.host['lost'][READ_LOST]) == (tag == 'a')


@pytest.mark.parametrize('blur', BLURS)
@pytest.mark.parametrize('T', ('tiles', 'one'))
def test_a_batch_is_the_host_route_item_by_item(T, blur):
    T = n_frames() if T == 'tiles' else 1
    ids, times = batch_items(T)
    bank = bank_of_two()
    want, want_warned = host_batch(T, blur)
    for dtype in DTYPES:
        got, warned = caught(lambda: bank.targets(ids, np.array(times), blur, dtype))
        assert got.is_cuda and got.dtype == dtype and got.shape == (4, 540, T)
        assert torch.equal(got.cpu(), torch.from_numpy(want).to(dtype))
        assert bank.last_lost.tolist() == want_warned and warned == any(want_warned)
        for b in range(4):                                                         # an item does not depend on its neighbours
            single, warned = caught(lambda: bank.targets(int(ids[b]), np.array(times[b]), blur, dtype))
            assert single.shape == (540, T) and torch.equal(single, got[b]) and warned == want_warned[b]
    if T > 1:
        assert want_warned == [True, False, False, False]
        assert not want[2].any() and want[0].max() == want[1].max() == want[3].max() == 1.0
        assert np.isneginf(times[3][:7]).all() and np.isposinf(times[3][-1])       # the padded item reads frames 3 and K - 2 there
        back, _ = caught(lambda: bank.targets(ids, np.array(times), blur, torch.float64, return_tensor=False))
        assert isinstance(back, np.ndarray) and np.array_equal(back, want)


def test_one_bin():
    """F = 1: the only bin is MIDI 69; 440 Hz paints it, 441 Hz is lost, 0 is dropped."""
    midi = np.array([69.0])
    track = (np.arange(6) * 0.01, [np.array([440.0]), np.empty(0), np.array([0.0]), np.array([441.0]), np.array([440.0, 440.0]), np.empty(0)])
    T = n_frames()
    times = np.stack([np.linspace(-0.01, 0.07, T), np.linspace(0.006, 0.024, T)])
    bank = PitchBank([track], midi, None, DEV)
    for blur in BLURS:
        for b, flag in ((0, True), (1, False)):
            want, warned = caught(lambda: multi_pitch_to_activations(lists_route(track, times[b], [0, -1]), midi, blur, DEV))
            assert warned == flag
            got, warned = caught(lambda: bank.targets([0, 0], times, blur, torch.float64))
            assert warned and got.shape == (2, 1, T) and np.array_equal(got[b].cpu().numpy(), want) and bank.last_lost.tolist() == [True, False]
    assert want.sum() == 0 and float(got[0].sum()) > 0


def test_over_a_capacity_takes_the_list_route():
    _, max_bins, max_radius = pitch_tiles()
    t2 = second_track()
    T = 70
    times = np.stack([np.linspace(t2[0][15], t2[0][-1] + 0.01, T), np.linspace(t2[0][0] - 0.01, t2[0][30], T)])
    wide = MIDI_FREQS[0] + np.arange(max_bins + 1) * 0.1                          # one bin more than the mask holds
    blur_wide = 5.0 * (max_radius + 1) / 8.0                                       # sigma = (radius + 1) / 4: one more than the window holds
    assert _gaussian_weights((2 * blur_wide) / 5)[1] == max_radius + 1
    for midi, blur in ((wide, 2.5), (MIDI_FREQS, blur_wide)):
        bank = PitchBank([t2], midi, None, DEV)
        assert not bank._on_device(np.array([0, 0]), _gaussian_weights((2 * blur) / 5)[1])
        for dtype in DTYPES:
            got = bank.targets([0, 0], times, blur, dtype)
            assert got.is_cuda and got.dtype == dtype and got.shape == (2, len(midi), T)
            for b in range(2):
                want = multi_pitch_to_activations(lists_route(t2, times[b], [0, -1]), midi, blur, DEV, return_tensor=True)
                assert torch.equal(got[b], want.to(dtype))
    # a track whose times are not sorted never reaches the kernels either; its neighbour in the bank still does
    perm = np.random.default_rng(5).permutation(len(t2[0]))
    shuffled = (t2[0][perm], [t2[1][i] for i in perm])
    bank = PitchBank([shuffled, t2], MIDI_FREQS, None, DEV)
    assert bank.host['device_ok'].tolist() == [False, True] and bank._on_device(np.array([1]), 4) and not bank._on_device(np.array([0, 1]), 4)
    got = bank.targets([0, 1], times, 2.5, torch.float64)
    for b, tr in enumerate((shuffled, t2)):
        want = multi_pitch_to_activations(lists_route(tr, times[b], [0, -1]), MIDI_FREQS, 2.5, DEV, return_tensor=True)
        assert torch.equal(got[b], want)


def test_two_runs_are_identical_and_arguments_are_checked():
    T = n_frames()
    ids, times = batch_items(T)
    bank = bank_of_two()
    with pytest.warns(RuntimeWarning):
        a = bank.targets(ids, np.array(times))
    with pytest.warns(RuntimeWarning):
        b = bank.targets(ids, np.array(times))
    assert a.dtype == torch.float32 and torch.equal(a, b) and float(a.max()) == 1.0
    empty = bank.targets(np.zeros(0, dtype=np.int64), np.zeros((0, T)))
    assert empty.shape == (0, 540, T) and bank.last_lost.shape == (0,)
    assert bank.targets(ids, np.zeros((4, 0))).shape == (4, 540, 0)
    with pytest.raises(IndexError):
        bank.targets([0, 2, 0, 0], np.array(times))
    with pytest.raises(ValueError):
        bank.targets([0, 1], np.array(times))
    with pytest.raises(ValueError):
        bank.targets(ids, np.array(times), dtype=torch.float16)


def evaluable(lists):
    """The fixture track as the scorer accepts it: zeros dropped, pitches moved into [20, 5000] Hz."""
    return [np.clip(f[f != 0], 20.0, 5000.0) for f in lists]


def test_evaluate_track_is_evaluate_activations():
    src, lists = fixture_track('a')
    t2 = second_track()
    _, _, midi_freqs = golden_tracks()
    good = evaluable(lists)
    bank = PitchBank([(src, list(lists)), (src, good), t2], midi_freqs, None, DEV)
    x = torch.from_numpy(np.array(activations(0.05, T_EST))).to(DEV)
    est_time = est_times(T_EST)
    kw = dict(window=0.5, n_valid_bins=FV)
    ev = MultipitchEvaluator()
    for n, (ref_time, ref) in ((1, (src, good)), (2, t2)):
        want = multipitch_counts_device(ref_time, list(ref), est_time, x, MIDI_FREQS, **kw)
        got = multipitch_counts_device_track(bank, n, est_time, x, MIDI_FREQS, **kw)
        for name in ('tp', 'tp_chroma', 'n_ref', 'n_est'):
            assert got[name].dtype == torch.int32 and torch.equal(got[name], want[name]), name
        assert np.array_equal(got['sums'], want['sums']) and got['n_host_frames'] == want['n_host_frames'] == 0
        scores = multipitch_metrics_device(ref_time, list(ref), est_time, x, MIDI_FREQS, **kw)
        assert multipitch_metrics_device_track(bank, n, est_time, x, MIDI_FREQS, **kw) == scores and len(scores) == 14
        tagged = ev.evaluate_track(est_time, x[None], MIDI_FREQS, bank, n, n_valid_bins=FV)
        assert tagged == ev.evaluate_activations(est_time, x[None], MIDI_FREQS, ref_time, list(ref), n_valid_bins=FV) and len(tagged) == 15
        if n == 1:
            assert got['sums'][0] > 0 and int(got['n_ref'].sum()) == sum(len(f) for f in good) and tagged['mpe/f1-score'] > 0
    # the fixture as recorded holds zeros and pitches above 5 kHz: both routes refuse it
    with pytest.raises(ValueError):
        ev.evaluate_activations(est_time, x, MIDI_FREQS, src, list(lists), n_valid_bins=FV)
    with pytest.raises(ValueError):
        ev.evaluate_track(est_time, x, MIDI_FREQS, bank, 0, n_valid_bins=FV)
    with pytest.raises(ValueError):                                                # estimate times / frames mismatch
        ev.evaluate_track(est_time[:-1], x, MIDI_FREQS, bank, 1, n_valid_bins=FV)
    with pytest.raises(IndexError):
        ev.evaluate_track(est_time, x, MIDI_FREQS, bank, 3, n_valid_bins=FV)
    with pytest.raises(RuntimeError):                                              # no CPU fallback
        ev.evaluate_track(est_time, x.cpu(), MIDI_FREQS, bank, 1, n_valid_bins=FV)
