"""
CPU-only: the host side of the device route for frame-level pitch annotations (timbre_trap/utils/pitch.py) against what the reference's
``PitchDataset.resample_multi_pitch`` + ``multi_pitch_to_activations`` returned (tests/golden/pitch.npz, recorded by
tests/golden/make_golden_pitch.py): the bank's flat arrays, expanded through ``nearest_indices``, give the recorded maps through
oracle/targets.py's blur; the nearest rule equals SciPy's on the fixture's grid; and a restatement of csrc/pitch.hip's arithmetic in
integers -- a bitmask per frame, a window of 2 r + 1 bits per position, zero pairs skipped, one minimum per tile of frames -- gives the
same maps, bit for bit.

Everything here is float64 comparisons and integers, so every assertion is ``==`` / ``array_equal``.

``golden_tracks`` / ``second_track`` / ``lists_route`` / ``expanded_pairs`` are shared with tests/test_gpu_pitch.py; what they return is
cached and read-only.
"""

import functools
import os
import warnings

import numpy as np
import pytest
import scipy.interpolate

from oracle import targets as otg
from timbre_trap.utils import pitch, resample_multi_pitch
from timbre_trap.utils.slicing import nearest_indices
from timbre_trap.utils.targets import midi_to_hz

from test_mpe_restatement import MIDI_FREQS, frozen

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pitch.npz')
WARNING = 'Could not fully represent'
READ_LOST, UNREAD_LOST = 37, 121              # make_golden_pitch.py: source frames that hold a pitch outside the bin range
TILE = 64                                     # frames per tile of the restatement (the library's own figure is asserted on the GPU)


# ---- inputs -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def golden_tracks():
    """tests/golden/pitch.npz as {'a' | 'b': dict(source_times, lists, idcs, idx, act_blur, act_noblur, warned)}, times, midi_freqs."""
    g = np.load(GOLDEN)
    sets = {}
    for tag in ('a', 'b'):
        keep = np.ones(len(g['values']), dtype=bool) if tag == 'a' else g['in_b']
        lists = [f[k] for f, k in zip(np.split(g['values'], np.cumsum(g['counts'])[:-1]), np.split(keep, np.cumsum(g['counts'])[:-1]))]
        sets[tag] = dict(source_times=frozen(g['source_times']), lists=tuple(frozen(f) for f in lists),
                         idcs=[int(i) for i in g['idcs_%s' % tag]], idx=frozen(g['idx_%s' % tag]), act_blur=frozen(g['act_%s_blur' % tag]),
                         act_noblur=frozen(g['act_%s_noblur' % tag]), warned=bool(g['warned_%s' % tag]))
    return sets, frozen(g['times']), frozen(g['midi_freqs'])


@functools.lru_cache(maxsize=None)
def second_track(n_frames=50, n_silent=20):
    """A short track on a regular 5.8 ms grid: ``n_silent`` empty frames, then one to three pitches per frame, all inside the bin range."""
    times = frozen(0.25 + 0.0058 * np.arange(n_frames))
    lists = [np.empty(0)] * n_silent
    for k in range(n_silent, n_frames):
        lists.append(midi_to_hz(MIDI_FREQS[[(53 * k + 97 * j) % 470 for j in range(1 + k % 3)]] + 0.04 * (k % 3 - 1)))
    return times, tuple(frozen(f) for f in lists)


def caught(fn):
    """fn() with every warning recorded: (result, whether the target code's RuntimeWarning was among them)."""
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        out = fn()
    return out, any(issubclass(x.category, RuntimeWarning) and WARNING in str(x.message) for x in w)


def lists_route(track, times, idcs):
    """The lists every item's frames read on the host route."""
    return resample_multi_pitch(track[0], list(track[1]), times, idcs)


def expanded_pairs(host, track_id, idx):
    """The (bin, frame) pairs of one item from the bank's host arena: frame t reads arena row base + idx[t]; dropped values carry -1.
    Returns (bins int32, frames int32, whether a row that is read holds a lost pitch)."""
    base = host['table'][track_id, 0]
    rows = base + np.asarray(idx, dtype=np.int64)
    lo, hi = host['row_off'][rows], host['row_off'][rows + 1]
    frames = np.repeat(np.arange(len(rows)), hi - lo)
    values = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)]).astype(np.int64) if len(frames) else np.empty(0, dtype=np.int64)
    bins = host['bins'][values]
    kept = bins >= 0
    return bins[kept].astype(np.int32), frames[kept].astype(np.int32), bool(host['lost'][rows].any())


def map_from_pairs(bins, frames, F, T, blur):
    """multi_pitch_to_activations from the pairs on: paint, oracle blur, division by the smallest painted value, clip."""
    act = np.zeros((F, T))
    if len(bins):
        act[bins, frames] = 1
        if blur:
            w, r = otg.gaussian_weights((2 * blur) / 5)
            act = otg.blur_rows(act, w, r)
            act = np.clip(act / np.min(act[bins, frames]), 0.0, 1.0)
    return act


# ---- csrc/pitch.hip in integers -------------------------------------------------------------------------------------------------

def restated_window(words, wi, o, r):
    """pitch_window: bit k = mask bit 32 (wi - 1) + o + k of the three words around word ``wi``, cut to 2 r + 1 bits."""
    word = lambda w: int(words[w]) if 0 <= w < len(words) else 0                   # noqa: E731
    wi, o, r = int(wi), int(o), int(r)
    lo = word(wi - 1) | (word(wi) << 32)
    return ((lo >> o) | ((word(wi + 1) << (64 - o)) & (2 ** 64 - 1))) & ((1 << (2 * r + 1)) - 1)


def restated_blur(u, w, r):
    """pitch_blur: the centre first, then the pairs from the outside in; a pair without a one is skipped."""
    u, r = int(u), int(r)
    acc = np.float64((u >> r) & 1) * w[r]
    for j in range(-r, 0):
        pair = ((u >> (r + j)) & 1) + ((u >> (r - j)) & 1)
        if pair:
            acc = acc + np.float64(pair) * w[r + j]
    return acc


def restated_kernels(host, track_id, idx, F, blur, dtype=np.float64, tile=TILE):
    """k_pitch_min / k_pitch_reduce / k_pitch_write on one item: (map, flag)."""
    T = len(idx)
    r, w = 0, None
    if blur:
        w, r = otg.gaussian_weights((2 * blur) / 5)
    base, K = host['table'][track_id, :2]
    n_words = -(-F // 32)
    masks, rows = np.zeros((T, n_words), dtype=np.uint32), np.full(T, -1, dtype=np.int64)
    for t in range(T):
        if 0 <= idx[t] < K:
            rows[t] = base + idx[t]
            for f in host['bins'][host['row_off'][rows[t]]:host['row_off'][rows[t] + 1]].tolist():
                if 0 <= f < F:
                    masks[t, f >> 5] |= np.uint32(1 << (f & 31))
    partials = []
    for t0 in range(0, T, tile):                                                   # one minimum per tile, then the minimum of those
        m = 1.0e300
        for t in range(t0, min(T, t0 + tile)):
            if rows[t] >= 0 and r:
                for f in host['bins'][host['row_off'][rows[t]]:host['row_off'][rows[t] + 1]].tolist():
                    if 0 <= f < F:
                        m = min(m, restated_blur(restated_window(masks[t], f >> 5, 32 + (f & 31) - r, r), w, r))
        partials.append(m)
    mn = min(partials)
    out = np.zeros((F, T), dtype=np.float64)
    for t in range(T):
        for wi in range(n_words):
            if not any(int(masks[t, k]) for k in (wi - 1, wi, wi + 1) if 0 <= k < n_words):
                continue
            for k in range(min(32, F - 32 * wi)):
                if r == 0:
                    out[32 * wi + k, t] = (int(masks[t, wi]) >> k) & 1
                else:
                    u = restated_window(masks[t], wi, 32 + k - r, r)
                    if u:
                        out[32 * wi + k, t] = min(max(restated_blur(u, w, r) / mn, 0.0), 1.0)
    return out.astype(dtype), bool(host['lost'][rows[rows >= 0]].any())


# ---- tests --------------------------------------------------------------------------------------------------------------------

def test_fixture_covers_the_corner_cases():
    sets, times, midi_freqs = golden_tracks()
    a, b = sets['a'], sets['b']
    assert np.array_equal(midi_freqs, MIDI_FREQS) is False and len(midi_freqs) == 540         # the real grid, not the tests' round one
    src = a['source_times']
    assert len(src) == 200 and len(times) == 300 and (np.diff(src) >= 0).all() and src[49] == src[50]
    assert np.isneginf(times[:15]).all() and np.isposinf(times[-25:]).all() and not (np.diff(times[15:-25]) >= 0).all()
    assert a['idcs'] == [3, -2] and b['idcs'] == [0, -1]
    assert (a['idx'][:15] == 3).all() and (a['idx'][-25:] == 198).all() and (b['idx'][:15] == 0).all() and (b['idx'][-25:] == 199).all()
    for s in (a, b):
        assert READ_LOST in s['idx'] and UNREAD_LOST not in s['idx']
    assert a['warned'] and not b['warned']
    assert len(a['lists'][READ_LOST]) == 2 and len(b['lists'][READ_LOST]) == 1 and len(b['lists'][UNREAD_LOST]) == 2
    assert (a['lists'][30] == 0).sum() == 2 and sum(len(f) == 0 for f in a['lists']) >= 40
    mids = src / 2.0
    mids = mids[1:] + mids[:-1]
    assert sum(int(t in mids) for t in times) >= 6                                 # exact midpoints are among the targets
    assert a['act_blur'].max() == 1.0 and a['act_noblur'][0].any() and a['act_noblur'][-1].any()        # both edge bins are painted


@pytest.mark.parametrize('tag', ('a', 'b'))
def test_nearest_rule_is_scipy_on_the_fixture(tag):
    sets, times, _ = golden_tracks()
    s = sets[tag]
    src = s['source_times']
    original = np.arange(len(src))
    below, above = original[s['idcs'][0]], original[s['idcs'][-1]]
    got = nearest_indices(src, times, below, above)
    assert np.array_equal(got, s['idx'])                                           # what the reference's interp1d returned
    again = scipy.interpolate.interp1d(x=src, y=original, kind='nearest', bounds_error=False, fill_value=(below, above),
                                       assume_sorted=True)(times).astype('uint')
    assert np.array_equal(got, again)
    k = 48                                                                         # an exact midpoint goes to the earlier frame
    mid = src[k] / 2.0 + src[k + 1] / 2.0
    assert list(nearest_indices(src, [np.nextafter(mid, -np.inf), mid, np.nextafter(mid, np.inf)], below, above)) == [k, k, k + 1]
    # K = 1 has no midpoints; a NaN target sorts after every midpoint and fails both comparisons
    assert list(nearest_indices(src[:1], [src[0] - 1.0, src[0], src[0] + 1.0, np.nan], 0, 0)) == [0, 0, 0, 0]
    assert list(nearest_indices(src, [np.nan], below, above)) == [len(src) - 1]


@pytest.mark.parametrize('tag', ('a', 'b'))
def test_bank_arrays_give_the_reference_maps(tag):
    sets, times, midi_freqs = golden_tracks()
    s = sets[tag]
    host = pitch._bank_arrays([(s['source_times'], list(s['lists']))], midi_freqs, s['idcs'])
    K, F, T = len(s['lists']), len(midi_freqs), len(times)
    assert host['table'].tolist() == [[0, K, np.arange(K)[s['idcs'][0]], np.arange(K)[s['idcs'][-1]]]]
    assert host['row_off'][-1] == sum(len(f) for f in s['lists']) == len(host['bins']) == len(host['midi'])
    assert host['device_ok'].all() and host['outside'].all()                       # sorted and finite; pitches far above 5 kHz
    assert np.flatnonzero(host['lost']).tolist() == ([READ_LOST, UNREAD_LOST] if tag == 'a' else [UNREAD_LOST])
    below, above = host['table'][0, 2:]
    idx = nearest_indices(s['source_times'], times, below, above)
    bins, frames, lost = expanded_pairs(host, 0, idx)
    assert lost == s['warned']                                                     # a lost pitch in a frame nobody reads does not warn
    for blur, key in ((2.5, 'act_blur'), (0, 'act_noblur')):
        assert np.array_equal(map_from_pairs(bins, frames, F, T, blur), s[key])
    # two pitches in one bin paint once: the pairs hold a duplicate
    pairs = set(zip(bins.tolist(), frames.tolist()))
    assert len(pairs) < len(bins)
    # the scorer's arrays are those of the list route
    from timbre_trap.utils.metrics import frequencies_to_midi
    with np.errstate(divide='ignore'):
        assert np.array_equal(host['midi'], frequencies_to_midi([np.concatenate(s['lists'])])[0])


@pytest.mark.parametrize('blur', (2.5, 0, 5.0))
@pytest.mark.parametrize('tag', ('a', 'b'))
def test_restated_kernels_give_the_maps(tag, blur):
    sets, times, midi_freqs = golden_tracks()
    s = sets[tag]
    host = pitch._bank_arrays([(s['source_times'], list(s['lists']))], midi_freqs, s['idcs'])
    bins, frames, _ = expanded_pairs(host, 0, s['idx'])
    want = s['act_blur'] if blur == 2.5 else s['act_noblur'] if blur == 0 else map_from_pairs(bins, frames, 540, 300, blur)
    got, flag = restated_kernels(host, 0, s['idx'], 540, blur)
    assert np.array_equal(got, want) and flag == s['warned']
    if blur == 2.5:
        got32, _ = restated_kernels(host, 0, s['idx'], 540, blur, np.float32)
        assert got32.dtype == np.float32 and np.array_equal(got32, want.astype(np.float32))


def test_bank_arrays_of_several_tracks_and_odd_input():
    sets, times, midi_freqs = golden_tracks()
    a = sets['a']
    t2, l2 = second_track()
    host = pitch._bank_arrays([(a['source_times'], list(a['lists'])), (t2, list(l2)), ([1.0], [[440.0, 0]])], midi_freqs, [0, -1])
    assert host['table'].tolist() == [[0, 200, 0, 199], [200, 50, 0, 49], [250, 1, 0, 0]]
    assert host['outside'].tolist() == [True, False, True]                         # a zero is outside the scorer's range too
    assert len(host['times']) == 251 and len(host['row_off']) == 252 and host['lost'][200:].sum() == 0
    one = pitch._bank_arrays([(t2, list(l2))], midi_freqs, [0, -1])
    b0, b1 = host['row_off'][200], host['row_off'][250]
    assert np.array_equal(host['bins'][b0:b1], one['bins']) and np.array_equal(host['row_off'][200:251] - b0, one['row_off'])
    # unsorted or non-finite source times never reach the device route
    odd = pitch._bank_arrays([(t2[::-1], list(l2)), (np.where(np.arange(50) == 49, np.inf, t2), list(l2)), (t2, list(l2))], midi_freqs, [0, -1])
    assert odd['device_ok'].tolist() == [False, False, True]
    with pytest.raises(ValueError):
        pitch._bank_arrays([(t2[:-1], list(l2))], midi_freqs, [0, -1])
    with pytest.raises(ValueError):
        pitch._bank_arrays([([], [])], midi_freqs, [0, -1])


def test_device_route_refuses_the_cpu_and_the_stand_in_has_the_method():
    from timbre_trap import datasets
    from timbre_trap.utils import PitchBank, pitch_to_activations
    t2, l2 = second_track()
    with pytest.raises(RuntimeError):                                              # no CPU fallback
        PitchBank([(t2, list(l2))], MIDI_FREQS, device='cpu')
    with pytest.raises(RuntimeError):
        pitch_to_activations(t2, list(l2), t2, MIDI_FREQS, device='cpu')
    assert hasattr(datasets.PitchDataset, 'multi_pitch_to_activations')
    if datasets.REFERENCE_DATASETS is None:
        assert datasets.PitchDataset.pitch_to_activations is pitch_to_activations
