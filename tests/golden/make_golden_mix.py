"""
Generates tests/golden/mix.npz by importing the REFERENCE (read-only at /root/reference) in this container and recording what its
``StemMixingDataset`` returns for 12 consecutive items over three in-memory datasets -- one ``AudioDataset`` (2 tracks) and two
``MPEDataset``s (3 and 2 tracks) with seeds of their own -- at ``n_secs = 0.2`` (4410 samples, 69 frames), ``n_min = 1``,
``n_max = 5``.  Run once here:

    python tests/golden/make_golden_mix.py

Only inputs and recorded outputs travel; third-party modules the reference imports and this image lacks are stubbed for import only
(``make_golden.install_stubs`` plus empty ``mir_eval`` / ``jams`` / ``mido``).  The datasets below subclass the reference's base classes
with closed-form tracks held in memory (``get_audio`` / ``get_ground_truth`` overridden, ``base_dir`` an existing temporary directory so
that nothing is fetched); everything that draws, cuts, sums and clamps is the reference's own code.

Seven tracks: lengths 6000 and 1 (audio only), 5200, 4410 (exactly one excerpt: its only slice ends at the track's end) and 3000
(annotated, seed 5), 4800 and 7000 (annotated, seed 11); the tracks of 1 and 3000 samples are shorter than the excerpt and are zero
padded.  Every annotated track holds bin 270 in every fifth annotation frame, so mixtures of two annotated stems sum above 1 there.

Recorded per item: the audio, the float64 ground truth (zeros and ``has_gt`` False where the mixture holds no annotated stem), the
times, and the plan -- the stems in the order drawn (global index into the ``ComboDataset`` space, excerpt start in samples, negative
= zero padding in front), captured by wrapping ``slice_audio``.
"""

import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import stub_cqt  # noqa: E402
from make_golden import install_stubs  # noqa: E402

SAMPLE_RATE, N_SECS, N_ITEMS = 22050, 0.2, 12
N_MIN, N_MAX, MIX_SEED = 1, 5, 10
LENGTHS = ((6000, 1), (5200, 4410, 3000), (4800, 7000))       # per dataset; the first dataset has no annotations
SEEDS = (3, 5, 11)
ANNOTATION_STEP, COMMON_BIN = 0.01, 270


def hz(m):
    return 440.0 * (2.0 ** ((np.asarray(m, dtype=np.float64) - 69.0) / 12.0))


def closed_form_tracks():
    """Per global track index: (1 x N) float32 audio; closed-form, every track its own phase."""
    n_tracks = sum(len(d) for d in LENGTHS)
    longest = max(max(d) for d in LENGTHS)
    bank = stub_cqt.closed_form_audio(n_tracks, longest)
    flat = [n for d in LENGTHS for n in d]
    return [bank[g, :, :n].clone() for g, n in enumerate(flat)]


def closed_form_annotations(g, n_samples, midi_freqs):
    """(times (K), list of K arrays in Hz) for global track g: a 10 ms grid over the track, 0 to 2 pitches a frame plus the common bin."""
    K = int(np.ceil(n_samples / SAMPLE_RATE / ANNOTATION_STEP)) + 1
    times = ANNOTATION_STEP * np.arange(K)
    mp = []
    for k in range(K):
        bins = [(37 * k + 111 * j + 53 * g) % 500 + 10 for j in range((k + g) % 3)]
        values = [float(hz(midi_freqs[b] + 0.03 * ((k + j) % 5 - 2))) for j, b in enumerate(bins)]
        if k % 5 == 0:
            values.append(float(hz(midi_freqs[COMMON_BIN])))
        mp.append(np.array(values, dtype=np.float64))
    return times, mp


def main():
    install_stubs()
    for name in ('mir_eval', 'jams', 'mido'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, '/root/reference')
    from timbre_trap.datasets import AudioDataset, MPEDataset, StemMixingDataset
    from timbre_trap.framework import CQT
    cqt = CQT(n_octaves=9, bins_per_octave=60, sample_rate=SAMPLE_RATE, secs_per_block=3)
    midi_freqs = np.asarray(cqt.get_midi_freqs(), dtype=np.float64)
    audio = closed_form_tracks()
    first = np.concatenate([[0], np.cumsum([len(d) for d in LENGTHS])])
    drawn = []                                   # (global index, start) in the order the reference cuts the stems

    class InMemory:
        """What both in-memory datasets share: track names are global indices, audio comes from the list above."""

        @staticmethod
        def available_splits():
            return ['all']

        def get_tracks(self, split):
            return [str(g) for g in range(first[self.k], first[self.k + 1])]

        def get_audio(self, track):
            self.current = int(track)
            return audio[int(track)].clone()

        def slice_audio(self, audio, n_samples=None, offset_s=None):
            out, offset_t = super().slice_audio(audio, n_samples, offset_s)
            drawn.append((self.current, int(round(offset_t * self.sample_rate))))
            return out, offset_t

    class MemoryAudio(InMemory, AudioDataset):
        k = 0

    class MemoryMPE(InMemory, MPEDataset):
        def get_ground_truth(self, track):
            return closed_form_annotations(int(track), audio[int(track)].size(-1), midi_freqs)

    class MemoryMPE1(MemoryMPE):
        k = 1

    class MemoryMPE2(MemoryMPE):
        k = 2

    with tempfile.TemporaryDirectory() as base_dir:
        datasets = [MemoryAudio(sample_rate=SAMPLE_RATE, base_dir=base_dir, n_secs=N_SECS, seed=SEEDS[0]),
                    MemoryMPE1(sample_rate=SAMPLE_RATE, cqt=cqt, base_dir=base_dir, n_secs=N_SECS, seed=SEEDS[1]),
                    MemoryMPE2(sample_rate=SAMPLE_RATE, cqt=cqt, base_dir=base_dir, n_secs=N_SECS, seed=SEEDS[2])]
        mixer = StemMixingDataset(datasets, tracks_per_epoch=N_ITEMS, n_min=N_MIN, n_max=N_MAX, seed=MIX_SEED)
        assert len(mixer) == N_ITEMS
        n_samples = int(N_SECS * SAMPLE_RATE)
        n_frames = cqt.get_expected_frames(cqt.get_expected_samples(N_SECS))
        out_audio = np.zeros((N_ITEMS, n_samples), dtype=np.float32)
        out_gt = np.zeros((N_ITEMS, len(midi_freqs), n_frames), dtype=np.float64)
        out_times = np.full((N_ITEMS, n_frames), np.nan)
        has_gt = np.zeros(N_ITEMS, dtype=bool)
        drawn_off = [0]
        for i in range(N_ITEMS):
            data = mixer[i]
            assert data['track'] == str(i) and tuple(data['audio'].shape) == (1, n_samples) and data['audio'].dtype == torch.float32
            out_audio[i] = data['audio'][0].numpy()
            if 'ground-truth' in data:
                assert data['ground-truth'].dtype == np.float64 and data['ground-truth'].shape == out_gt[i].shape
                has_gt[i], out_gt[i], out_times[i] = True, data['ground-truth'], data['times']
            drawn_off.append(len(drawn))
    n_mix = np.diff(drawn_off)
    idx = np.array([g for g, _ in drawn], dtype=np.int64)
    start = np.array([s for _, s in drawn], dtype=np.int64)
    annotated = idx >= first[1]
    per_item = [annotated[a:b] for a, b in zip(drawn_off[:-1], drawn_off[1:])]
    # what the tests rely on: every kind of item and of excerpt occurs
    assert any(not a.any() for a in per_item) and any(a.all() and len(a) > 1 for a in per_item)
    assert any(a.any() and not a.all() for a in per_item) and n_mix.min() == 1 and n_mix.max() == 5
    assert all(has_gt[i] == per_item[i].any() for i in range(N_ITEMS))
    assert (start < 0).any() and out_gt.max() == 1.0 and (out_gt.sum(axis=(1, 2)) > 0).sum() == has_gt.sum()
    flat = [n for d in LENGTHS for n in d]
    assert all(g in idx for g in range(len(flat))), 'every track should be drawn at least once'
    notes = [closed_form_annotations(g, flat[g], midi_freqs) for g in range(first[1], len(flat))]
    out = {'sample_rate': np.array(SAMPLE_RATE), 'n_secs': np.array(N_SECS), 'n_min': np.array(N_MIN), 'n_max': np.array(N_MAX),
           'mix_seed': np.array(MIX_SEED), 'seeds': np.array(SEEDS), 'dataset_first': first.astype(np.int64),
           'track_lengths': np.array(flat, dtype=np.int64), 'track_audio': np.concatenate([a[0].numpy() for a in audio]),
           'midi_freqs': midi_freqs, 'block_length': np.array(cqt.block_length), 'max_window_length': np.array(cqt.max_window_length),
           'ann_frames': np.array([len(t) for t, _ in notes], dtype=np.int64), 'ann_times': np.concatenate([t for t, _ in notes]),
           'ann_counts': np.concatenate([[len(f) for f in mp] for _, mp in notes]).astype(np.int64),
           'ann_values': np.concatenate([np.concatenate(mp) for _, mp in notes]),
           'audio': out_audio, 'ground_truth': out_gt, 'times': out_times, 'has_gt': has_gt, 'n_mix': n_mix.astype(np.int64),
           'drawn_index': idx, 'drawn_start': start}
    print('n_mix', n_mix.tolist(), 'annotated stems per item', [int(a.sum()) for a in per_item], 'padded stems', int((start < 0).sum()),
          'clamped elements', int((out_gt == 1.0).sum()))
    path = os.path.join(HERE, 'mix.npz')
    np.savez_compressed(path, **out)
    print('mix.npz', os.path.getsize(path))


if __name__ == '__main__':
    main()
