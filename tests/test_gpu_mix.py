"""
Random stem mixtures on the MI355X (csrc/mix.hip; timbre_trap.utils.AudioBank / StemMixer / mix_targets) against the explicit
sequential loop over the stems -- the kernels' contract, see tests/test_mix_restatement.py for why it is the loop and not
``torch.sum`` -- and against what the reference's ``StemMixingDataset`` recorded (tests/golden/mix.npz).

Nothing rounds differently on the two sides: every comparison is ``torch.equal`` / ``np.array_equal``, never a tolerance (the sign of a
zero is not part of the contract, and neither comparison sees it).  Sizes come from the library: N and F T straddle tt_mix_tile() /
tt_mix_targets_tile(); the arena's track bases and the stems' starts take every residue mod 4, so both load paths run at every
alignment, and the output sits at two alignments inside a guard buffer.
"""

import functools

import numpy as np
import pytest
import torch

from timbre_trap import _hip
from timbre_trap.utils import AudioBank, StemMixer, StemSource, mix_targets, mix_tiles, slice_audio

from test_mix_restatement import fixture_cqt, fixture_mixer, golden_mix, sequential_sum

pytestmark = pytest.mark.gpu

DEV = 'cuda'
STEM_COUNTS = (0, 1, 2, 5, 7)


def tile():
    return mix_tiles()[0]


@functools.lru_cache(maxsize=None)
def small_bank():
    """Six closed-form tracks whose bases in the arena take every residue mod 4; one is a single sample long, one 7 samples."""
    t = tile()
    lengths = [3 * t + 1, 2 * t + 5, 1, t + 4, 4 * t + 1, 7]
    tracks = []
    for k, n in enumerate(lengths):
        i = torch.arange(n, dtype=torch.float64)
        tracks.append((0.6 * torch.sin(0.05 * i + k) + 0.3 * torch.sin(0.31 * i + 0.7 * k) + 1e-3 * (k + 1)).float().reshape(1, n))
    bank = AudioBank(tracks, DEV)
    assert set((bank.table[:, 0] % 4).tolist()) == {0, 1, 2, 3}
    return tracks, bank


def host_excerpt(track, start, n):
    """Output sample i = track[start + i] inside the track, +0 elsewhere."""
    out = torch.zeros(n, dtype=track.dtype)
    flat = track.reshape(-1)
    lo, hi = max(0, -start), min(n, len(flat) - start)
    if hi > lo:
        out[lo:hi] = flat[start + lo:start + hi]
    return out


def host_mix(tracks, stem_track, stem_start, item_off, item_split, n):
    """The yardstick: per item the audio-only group and the annotated group, each added stem after stem from zero; their sum when both
    hold a stem (the ``+=`` of BaseDataset.py:320), the one that does otherwise, zeros for an item without stems."""
    rows = []
    for b in range(len(item_off) - 1):
        s0, s1 = item_off[b], item_off[b + 1]
        cut = [host_excerpt(tracks[stem_track[s]], int(stem_start[s]), n) for s in range(s0, s1)]
        groups = [sequential_sum(torch.stack(c)) for c in (cut[:item_split[b]], cut[item_split[b]:]) if c]
        rows.append(torch.zeros(n) if not groups else (groups[0] if len(groups) == 1 else groups[0] + groups[1]))
    return torch.stack(rows) if rows else torch.zeros((0, n))


def stems_for(lengths, n):
    """(track, start) pairs for excerpts of n samples: per track the slice cases (first, last = ending exactly at the track's end, every
    residue mod 4, the middle) or the padding cases (pad_left in {0, 1, pad_total - 1, pad_total}), then starts that leave one sample,
    or none, of the track inside the excerpt."""
    out = []
    for t, length in enumerate(lengths):
        if length >= n:
            starts = {0, length - n, (length - n) // 2} | {r for r in range(4) if r <= length - n} | {length - n - r for r in range(4) if r <= length - n}
        else:
            pad_total = n - length
            starts = {-p for p in (0, 1, pad_total - 1, pad_total) if p >= 0}
        starts |= {length - 1, 1 - n, length, -n}
        out += [(t, s) for s in sorted(starts)]
    return out


def items_for(stems):
    """The stems dealt to items of 0, 1, 2, 5, 7, 0, ... stems; splits cycle through all audio-only, all annotated, both groups."""
    track, start, off, split = [], [], [0], []
    k = 0
    while len(track) < len(stems):
        n = min(STEM_COUNTS[k % len(STEM_COUNTS)], len(stems) - len(track))
        for t, s in stems[len(track):len(track) + n]:
            track.append(t)
            start.append(s)
        off.append(len(track))
        split.append((n, 0, n // 2)[(k // len(STEM_COUNTS)) % 3])
        k += 1
    for n in STEM_COUNTS:                                                          # every count once more with both groups
        for j in range(n):
            t, s = stems[(7 * j + n) % len(stems)]
            track.append(t)
            start.append(s)
        off.append(len(track))
        split.append(n // 2)
    return (np.array(track, dtype=np.int32), np.array(start, dtype=np.int64), np.array(off, dtype=np.int32), np.array(split, dtype=np.int32))


def call_mix_audio(bank, track, start, off, split, n, guard):
    """tt_mix_audio through the C ABI into the middle of a NaN-filled buffer: (the B x n result, whether the guards are untouched)."""
    B = len(off) - 1
    buf = torch.full((2 * guard + B * n,), float('nan'), dtype=torch.float32, device=DEV)
    up = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    track_d, start_d, off_d, split_d = up(track), up(start), up(off), up(split)
    y = buf[guard:guard + B * n]
    rc = _hip.lib().tt_mix_audio(_hip.ptr(bank.arena), _hip.ptr(bank.table_d), len(bank), _hip.ptr(track_d), _hip.ptr(start_d),
                                 _hip.ptr(off_d), _hip.ptr(split_d), B, n, _hip.ptr(y), _hip.stream_ptr())
    assert rc == 0
    got = buf.cpu()
    untouched = bool(torch.isnan(got[:guard]).all()) and bool(torch.isnan(got[guard + B * n:]).all())
    return got[guard:guard + B * n].reshape(B, n), untouched


@pytest.mark.parametrize('which', ['one', 'tile-1', 'tile', 'tile+1', '2tile+3'])
def test_mix_audio_is_the_sequential_loop(which):
    n = {'one': 1, 'tile-1': tile() - 1, 'tile': tile(), 'tile+1': tile() + 1, '2tile+3': 2 * tile() + 3}[which]
    tracks, bank = small_bank()
    lengths = bank.table[:, 1].tolist()
    stems = stems_for(lengths, n)
    track, start, off, split = items_for(stems)
    # what the cases are meant to cover, checked on the tables themselves
    counts, interior = np.diff(off), [(bank.table[t, 0] + s) % 4 for t, s in stems if s >= 0 and s + n <= lengths[t]]
    assert set(STEM_COUNTS) <= set(counts.tolist())
    assert any(sp == 0 and c for sp, c in zip(split, counts)) and any(sp == c and c for sp, c in zip(split, counts))
    assert any(0 < sp < c for sp, c in zip(split, counts))
    assert set(interior) == {0, 1, 2, 3}
    assert any(s + n == lengths[t] and s > 0 for t, s in stems) and (2, 0) in stems
    want = host_mix(tracks, track, start, off, split, n)
    for guard in (64, 67):                                                         # two alignments of the output
        got, untouched = call_mix_audio(bank, track, start, off, split, n, guard)
        assert untouched, guard
        assert not torch.isnan(got).any() and torch.equal(got, want), guard
    # the front: same tables, same values, (B, 1, N)
    assert torch.equal(bank.mix(track, start, off, split, n).cpu()[:, 0], want)


def test_mix_audio_two_runs_are_identical():
    tracks, bank = small_bank()
    n = 2 * tile() + 3
    tables = items_for(stems_for(bank.table[:, 1].tolist(), n))
    a, _ = call_mix_audio(bank, *tables, n, 64)
    b, _ = call_mix_audio(bank, *tables, n, 64)
    assert torch.equal(a, b)


def test_mix_audio_beyond_two_to_the_31():
    """A track whose base in the arena lies beyond 2^31 elements: offsets are 64-bit.  The arena is allocated, not filled."""
    t = tile()
    base, length, n = (1 << 31) + 5, 2 * t + 2, t + 3
    try:
        arena = torch.empty(base + length, dtype=torch.float32, device=DEV)
    except RuntimeError as e:                                                      # pragma: no cover
        pytest.fail('could not allocate the 8.6 GB arena: %r' % e)
    track = torch.sin(0.37 * torch.arange(length, dtype=torch.float64)).float()
    arena[base:].copy_(track)
    arena[:8].zero_()
    table = torch.tensor([0, 8, base, length], dtype=torch.int64, device=DEV)
    stem_track = np.array([1, 1, 0], dtype=np.int32)
    stem_start = np.array([3, length - n, 0], dtype=np.int64)
    off, split = np.array([0, 2, 3], dtype=np.int32), np.array([1, 0], dtype=np.int32)
    up = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    tables = [up(a) for a in (stem_track, stem_start, off, split)]
    y = torch.full((2, n), float('nan'), dtype=torch.float32, device=DEV)
    rc = _hip.lib().tt_mix_audio(_hip.ptr(arena), _hip.ptr(table), 2, *[_hip.ptr(a) for a in tables], 2, n, _hip.ptr(y), _hip.stream_ptr())
    assert rc == 0
    want = host_mix([torch.zeros(8), track], stem_track, stem_start, off, split, n)
    assert torch.equal(y.cpu(), want)
    del arena
    torch.cuda.empty_cache()


def host_targets(maps, off, dtype):
    rows = []
    for b in range(len(off) - 1):
        group = maps[off[b]:off[b + 1]]
        acc = sequential_sum(group) if len(group) else torch.zeros(maps.shape[1:], dtype=torch.float64)
        rows.append(torch.clamp(acc, 0, 1).to(dtype))
    return torch.stack(rows)


@pytest.mark.parametrize('F', [1, 3])
@pytest.mark.parametrize('which', ['1', '2', '3', 'tile-1', 'tile', 'tile+1'])
def test_mix_targets_is_the_sequential_loop(F, which):
    edge = mix_tiles()[1]
    T = {'1': 1, '2': 2, '3': 3, 'tile-1': edge - 1, 'tile': edge, 'tile+1': edge + 1}[which]
    off = np.array([0, 1, 1, 3, 8, 10], dtype=np.int32)                           # items of 1, 0, 2, 5, 2 maps
    gen = torch.Generator().manual_seed(100 * F + T)
    maps = torch.rand(10, F, T, generator=gen, dtype=torch.float64) * 0.6          # two maps and more: sums above 1
    maps[0, 0, 0] = -0.25                                                          # a negative entry (item 0: one map)
    maps[1, 0, 0], maps[2, 0, 0] = 0.75, 0.5                                       # a sum above 1 whatever the draws (item 2)
    maps[8, F - 1, T - 1], maps[9, F - 1, T - 1] = -0.5, 0.125                     # a negative sum (item 4)
    maps[4, F - 1, T // 2] = float('nan')                                          # a NaN (item 3)
    maps_d = maps.to(DEV)
    off_d = torch.from_numpy(off).to(DEV)
    B = len(off) - 1
    for dtype in (torch.float64, torch.float32):
        want = host_targets(maps, off, dtype)
        assert (want == 1).any() and (want[0] == 0).any() and want[1].abs().sum() == 0 and torch.isnan(want[3]).sum() == 1
        for guard in (16, 19):
            buf = torch.full((2 * guard + B * F * T,), -7.0, dtype=dtype, device=DEV)
            out = buf[guard:guard + B * F * T]
            rc = _hip.lib().tt_mix_targets(_hip.ptr(maps_d), _hip.ptr(off_d), B, F, T, int(dtype == torch.float32), _hip.ptr(out),
                                           _hip.stream_ptr())
            assert rc == 0
            got = buf.cpu().numpy()
            assert (got[:guard] == -7).all() and (got[guard + B * F * T:] == -7).all(), (dtype, guard)
            assert np.array_equal(got[guard:guard + B * F * T].reshape(B, F, T), want.numpy(), equal_nan=True), (dtype, guard)
        assert np.array_equal(mix_targets(maps_d, off, dtype).cpu().numpy(), want.numpy(), equal_nan=True)
    # maps that do not begin on a 16-byte boundary, and no map at all
    shifted = torch.empty(10 * F * T + 1, dtype=torch.float64, device=DEV)[1:].reshape(10, F, T).copy_(maps_d)
    assert np.array_equal(mix_targets(shifted, off, torch.float64).cpu().numpy(), host_targets(maps, off, torch.float64).numpy(), equal_nan=True)
    none = mix_targets(maps_d[:0], np.zeros(3, dtype=np.int32), torch.float32)
    assert none.shape == (2, F, T) and float(none.abs().sum()) == 0


@functools.lru_cache(maxsize=None)
def fixture_batch(dtype, budget=None):
    kw = {} if budget is None else {'map_budget_bytes': budget}
    data = fixture_mixer(DEV, **kw).batch(range(12), dtype=dtype)
    return data


def test_fixture_audio_and_times():
    g = golden_mix()
    data = fixture_batch(torch.float64)
    assert data['track'] == [str(i) for i in range(12)]
    assert data['audio'].shape == (12, 1, g['audio'].shape[1]) and data['audio'].dtype == torch.float32 and data['audio'].is_cuda
    assert torch.equal(data['audio'].cpu()[:, 0], torch.from_numpy(g['audio'].copy()))
    assert np.array_equal(data['times'], g['times'], equal_nan=True) and data['times'].dtype == np.float64
    assert np.array_equal(data['annotated'], g['has_gt'])


def test_fixture_ground_truth():
    g = golden_mix()
    d64, d32 = fixture_batch(torch.float64), fixture_batch(torch.float32)
    assert d64['ground_truth'].dtype == torch.float64 and d64['ground_truth'].is_cuda and d64['ground-truth'] is d64['ground_truth']
    assert np.array_equal(d64['ground_truth'].cpu().numpy(), g['ground_truth'])
    assert d32['ground_truth'].dtype == torch.float32
    assert torch.equal(d32['ground_truth'].cpu(), torch.from_numpy(g['ground_truth'].copy()).float())
    assert torch.equal(d32['audio'], d64['audio'])


def test_fixture_one_item_per_chunk():
    """A budget below one map: every chunk is one item.  Same tensors."""
    g = golden_mix()
    mixer = fixture_mixer(DEV, map_budget_bytes=1)
    assert [b1 - b0 for b0, b1 in mixer.upload()._chunks(np.arange(13))] == [1] * 12
    small = mixer.batch(range(12), dtype=torch.float64)
    whole = fixture_batch(torch.float64)
    assert torch.equal(small['ground_truth'], whole['ground_truth']) and torch.equal(small['audio'], whole['audio'])
    assert np.array_equal(small['times'], whole['times'], equal_nan=True)
    assert np.array_equal(small['ground_truth'].cpu().numpy(), g['ground_truth'])


def test_fixture_in_two_batches_and_twice():
    """The draws continue from batch to batch; two mixers built alike give identical tensors."""
    whole = fixture_batch(torch.float32)
    mixer = fixture_mixer(DEV)
    first, second = mixer.batch(range(5)), mixer.batch(range(5, 12))
    assert torch.equal(torch.cat([first['audio'], second['audio']]), whole['audio'])
    assert torch.equal(torch.cat([first['ground_truth'], second['ground_truth']]), whole['ground_truth'])
    assert second['track'] == [str(i) for i in range(5, 12)]
    again = fixture_mixer(DEV).batch(range(12))
    assert torch.equal(again['audio'], whole['audio']) and torch.equal(again['ground_truth'], whole['ground_truth'])


def test_audio_only_sources_give_audio_only():
    g = golden_mix()
    mixer = StemMixer([StemSource(g['tracks'][:2], None, seed=1), StemSource(g['tracks'][2:4], None, seed=2)], fixture_cqt(), 0.2, 3,
                      n_min=1, n_max=3, device=DEV)
    data = mixer.batch(range(3))
    assert sorted(data) == ['audio', 'track'] and data['audio'].shape == (3, 1, 4410)


def test_excerpts_are_slice_audio():
    g = golden_mix()
    tracks = g['tracks']
    bank = AudioBank([t if k % 2 else t[0] for k, t in enumerate(tracks)], DEV)   # (1, N) and (N) alike
    n = 4410
    ids, starts = [], []
    for k, t in enumerate(tracks):
        length = t.shape[-1]
        for s in ((0, min(1, length - n), (length - n) // 2, length - n) if length >= n else (0, -1, -(n - length) // 2, -(n - length - 1))):
            ids.append(k)
            starts.append(s)
    got = bank.excerpts(ids, starts, n).cpu()
    assert got.shape == (len(ids), 1, n)
    for b, (k, s) in enumerate(zip(ids, starts)):
        want, _ = slice_audio(tracks[k], n, s, sample_rate=22050)
        assert torch.equal(got[b], want), (k, s)


def test_argument_checks():
    tracks, bank = small_bank()
    with pytest.raises(RuntimeError):
        AudioBank(tracks, 'cpu')
    with pytest.raises(RuntimeError):
        fixture_mixer('cpu')
    with pytest.raises(IndexError):
        bank.excerpts([0, len(bank)], [0, 0], 16)
    with pytest.raises(IndexError):
        bank.mix([-1], [0], [0, 1], [0], 16)
    with pytest.raises(ValueError):
        bank.mix([0, 1], [0, 0], [0, 1], [0], 16)                                  # item_off does not reach the last stem
    with pytest.raises(ValueError):
        bank.mix([0], [0], [0, 1], [2], 16)                                        # a split beyond the item
    with pytest.raises(ValueError):
        StemMixer([StemSource(tracks, None)], fixture_cqt(), 0.2, 4, n_min=3, n_max=2, device=DEV)
    with pytest.raises(RuntimeError):
        mix_targets(torch.zeros(1, 2, 2, dtype=torch.float64), [0, 1])
    with pytest.raises(ValueError):
        mix_targets(torch.zeros(1, 2, 2, device=DEV), [0, 1])                      # float32 maps
    lib = _hip.lib()
    assert lib.tt_version() >= 18 and lib.tt_mix_tile() % 256 == 0
    y = torch.zeros(4, device=DEV)
    assert lib.tt_mix_audio(_hip.ptr(bank.arena), _hip.ptr(bank.table_d), len(bank), None, None, None, None, 1, -1, _hip.ptr(y),
                            _hip.stream_ptr()) != 0
    assert lib.tt_mix_audio(_hip.ptr(bank.arena), _hip.ptr(bank.table_d), len(bank), None, None, None, None, 1, 4, _hip.ptr(y),
                            _hip.stream_ptr()) != 0
    assert lib.tt_mix_targets(None, None, 1, -1, 4, 0, _hip.ptr(y), _hip.stream_ptr()) != 0
