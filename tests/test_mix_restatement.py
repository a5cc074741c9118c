"""
CPU-only: the host side of the stem mixer (timbre_trap.utils.mixing) against what the reference's ``StemMixingDataset`` recorded in
tests/golden/mix.npz, and the summation order the device kernels are held to.

``StemMixer.plan`` must make the reference's draws: the number of stems, the shuffled choice, one offset per stem from its own source's
generator with ``slice_audio``'s bounds, item after item -- whether it is asked item by item or once for all items.

Summation order.  The reference sums stems with ``torch.sum(dim=0)`` on the CPU.  The kernels (csrc/mix.hip) add the stems one after the
other from zero.  ``test_torch_sum_is_the_sequential_loop`` pins how far the two are the same values, in float32 and float64, at the
training length (66150 samples) and at the fixture's (4410):
  2, 3, 4 stems   every element;
  5 stems         every element of a row but its scalar tail.  torch's CPU sum walks a row in chunks of four vector registers and
                  finishes the rest of the row -- fewer than 64 elements -- with four interleaved accumulators over the stems; with a
                  fifth stem that is (((x0 + x4) + x1) + x2) + x3, not the loop.  Measured on torch 2.10 (AVX2 build, 32 floats or 16
                  doubles a chunk) with uniform random stems: 4 of 66150 and 14 of 4410 float32 elements, all in the tail, differ from the
                  loop by one unit in the last place; float64 likewise.  With 6 and more stems the tail regroups further.
A mixture holds 5 stems of ONE group (all annotated or all audio-only) only at ``n_mix = 5`` with every stem drawn from the same kind of
dataset; its last few samples may then differ from the reference's by a last-place unit.  Where the tail begins depends on the host's
vector width, so it cannot be a contract: THE EXPLICIT LOOP -- not ``torch.sum`` -- is the kernels' contract and the yardstick of
tests/test_gpu_mix.py.  The sign of a zero is not part of the contract: comparisons are ``torch.equal`` / ``np.array_equal``.
"""

import functools
import math
import os

import numpy as np
import pytest
import torch

from timbre_trap.utils import StemMixer, StemSource, slice_audio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class GridCQT:
    """The frame / time arithmetic of the transform (reference cqtwrapper.py:235-308) for the fixture's grid; no tables, no device."""

    def __init__(self, sample_rate, block_length, max_window_length, midi_freqs):
        self.sample_rate, self.block_length, self.max_window_length = sample_rate, block_length, max_window_length
        self.hop_length = block_length / max_window_length
        self.midi_freqs = midi_freqs

    def get_expected_samples(self, t):
        return int(max(0, t) * self.sample_rate)

    def get_expected_frames(self, num_samples):
        return math.ceil((num_samples / self.block_length) * self.max_window_length)

    def get_times(self, n_frames):
        return np.arange(n_frames) * self.hop_length / self.sample_rate

    def get_midi_freqs(self):
        return self.midi_freqs


@functools.lru_cache(maxsize=None)
def golden_mix():
    """The fixture, read once: a dict of read-only arrays plus ``tracks`` (1 x N float32 tensors per global index), ``annotations``
    ((times, list of arrays) per annotated track, in global order) and ``drawn_off``."""
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'mix.npz'))
    g = {k: z[k] for k in z.files}
    for a in g.values():
        a.setflags(write=False)
    bounds = np.concatenate([[0], np.cumsum(g['track_lengths'])])
    flat = torch.from_numpy(g['track_audio'].copy())
    g['tracks'] = [flat[a:b].reshape(1, -1) for a, b in zip(bounds[:-1], bounds[1:])]
    frames = np.concatenate([[0], np.cumsum(g['ann_frames'])])
    values = np.concatenate([[0], np.cumsum(g['ann_counts'])])
    g['annotations'] = []
    for a, b in zip(frames[:-1], frames[1:]):
        lists = [g['ann_values'][values[k]:values[k + 1]] for k in range(a, b)]
        g['annotations'].append((g['ann_times'][a:b], lists))
    g['drawn_off'] = np.concatenate([[0], np.cumsum(g['n_mix'])])
    return g


def fixture_cqt():
    g = golden_mix()
    return GridCQT(int(g['sample_rate']), int(g['block_length']), int(g['max_window_length']), g['midi_freqs'])


def fixture_mixer(device='cuda', **kw):
    """A fresh mixer over the fixture's three datasets (fresh generators: the draws start over)."""
    g = golden_mix()
    first = g['dataset_first']
    sources = []
    for k, seed in enumerate(g['seeds']):
        audio = g['tracks'][first[k]:first[k + 1]]
        ann = None if k == 0 else g['annotations'][first[k] - first[1]:first[k + 1] - first[1]]
        sources.append(StemSource(audio, ann, seed=int(seed)))
    return StemMixer(sources, fixture_cqt(), float(g['n_secs']), len(g['n_mix']), n_min=int(g['n_min']), n_max=int(g['n_max']),
                     seed=int(g['mix_seed']), device=device, **kw)


def sequential_sum(x):
    """The kernels' contract: x[0] + x[1] + ... added one after the other from zero."""
    acc = torch.zeros_like(x[0])
    for row in x:
        acc = acc + row
    return acc


def check_plan(p, items):
    g = golden_mix()
    first_annotated = g['dataset_first'][1]
    assert np.array_equal(p['n_mix'], g['n_mix'][items])
    assert np.array_equal(p['item_off'], np.concatenate([[0], np.cumsum(g['n_mix'][items])]))
    assert p['stem_track'].dtype == np.int32 and p['stem_start'].dtype == np.int64 and p['item_off'].dtype == np.int32
    for k, i in enumerate(items):
        a, b = g['drawn_off'][i], g['drawn_off'][i + 1]
        idx, start = g['drawn_index'][a:b], g['drawn_start'][a:b]
        assert p['drawn'][k] == list(zip(idx.tolist(), start.tolist())), i
        # group order: audio-only first, annotated second, each in drawn order (separate_ground_truth)
        ann = idx >= first_annotated
        want_idx, want_start = np.concatenate([idx[~ann], idx[ann]]), np.concatenate([start[~ann], start[ann]])
        s0, s1 = p['item_off'][k], p['item_off'][k + 1]
        assert np.array_equal(p['stem_track'][s0:s1], want_idx) and np.array_equal(p['stem_start'][s0:s1], want_start), i
        assert p['item_split'][k] == (~ann).sum()
        q0, q1 = p['pitch_off'][k], p['pitch_off'][k + 1]
        assert q1 - q0 == ann.sum() and np.array_equal(p['pitch_track'][q0:q1], idx[ann] - first_annotated)
        if ann.any():
            assert np.array_equal(p['pitch_times'][q0], g['times'][i]) and g['has_gt'][i]
        else:
            assert not g['has_gt'][i] and np.isnan(g['times'][i]).all()


def test_fixture_covers_the_cases():
    g = golden_mix()
    n_samples = int(float(g['n_secs']) * int(g['sample_rate']))
    lengths = g['track_lengths']
    assert len(lengths) == 7 and (lengths < n_samples).sum() == 2 and 1 in lengths and n_samples in lengths
    assert g['n_mix'].min() == 1 and g['n_mix'].max() == 5 and len(g['n_mix']) == 12
    assert g['has_gt'].any() and not g['has_gt'].all() and (g['drawn_start'] < 0).any()
    assert g['ground_truth'].max() == 1.0 and g['ground_truth'].min() == 0.0


def test_plan_item_by_item():
    mixer = fixture_mixer()
    assert len(mixer) == 12 and mixer.audio_bank is None                           # plan() needs no device
    for i in range(12):
        check_plan(mixer.plan([i]), [i])


def test_plan_all_at_once():
    mixer = fixture_mixer()
    check_plan(mixer.plan(range(12)), list(range(12)))
    assert mixer.audio_bank is None


def test_plan_reproduces_the_recorded_audio_on_the_host():
    """The plan's tables, cut with the host ``slice_audio`` and added with the sequential loop, give the reference's audio: the tables
    mean what the kernels take them to mean."""
    g = golden_mix()
    p = fixture_mixer().plan(range(12))
    n_samples = g['audio'].shape[1]
    for b in range(12):
        s0, s1, split = p['item_off'][b], p['item_off'][b + 1], p['item_split'][b]
        cut = [slice_audio(g['tracks'][p['stem_track'][s]], n_samples, int(p['stem_start'][s]), sample_rate=22050)[0][0] for s in range(s0, s1)]
        groups = [sequential_sum(torch.stack(c)) for c in (cut[:split], cut[split:]) if c]
        mix = groups[0] if len(groups) == 1 else groups[0] + groups[1]
        assert torch.equal(mix, torch.from_numpy(g['audio'][b].copy())), b


TAIL_CHUNK = 64          # torch's CPU sum: four vector registers of at most 16 floats (AVX-512) a chunk; what is left of a row is its tail


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('length', [66150, 4410])
def test_torch_sum_is_the_sequential_loop(dtype, length):
    """``torch.sum(x, dim=0)`` on the CPU against the explicit loop, as values: 2 to 4 stems everywhere, 5 stems everywhere but the
    row's scalar tail (docstring above), for the audio's shape (n, 1, N) and the maps' (n, F, T)."""
    gen = torch.Generator().manual_seed(length)
    for n in (2, 3, 4, 5):
        x = (torch.rand(n, 1, length, generator=gen, dtype=torch.float64) * 2 - 1).to(dtype)
        m = torch.rand(n, 7, length // 10, generator=gen, dtype=torch.float64).to(dtype)
        for t in (x, m):
            got, want = torch.sum(t, dim=0).reshape(-1), sequential_sum(t).reshape(-1)
            body = len(got) if n < 5 else len(got) // TAIL_CHUNK * TAIL_CHUNK
            differ = (got != want).nonzero().reshape(-1)
            print('%s n=%d %s: %d of %d elements differ, first at %s' % (dtype, n, tuple(t.shape), len(differ), len(got),
                                                                      int(differ[0]) if len(differ) else None))
            assert torch.equal(got[:body], want[:body]), n
            # and never by more than the rounding of one addition
            assert torch.allclose(got, want, rtol=0, atol=float(torch.finfo(dtype).eps) * n)


def test_argument_checks_without_a_device():
    with pytest.raises(RuntimeError):
        fixture_mixer(device='cpu')
    g = golden_mix()
    src = StemSource(g['tracks'][:2], None, seed=0)
    with pytest.raises(ValueError):
        StemMixer([src], fixture_cqt(), 0.2, 4, n_min=3, n_max=2)
    with pytest.raises(ValueError):
        StemSource(g['tracks'][:2], g['annotations'][:1])
