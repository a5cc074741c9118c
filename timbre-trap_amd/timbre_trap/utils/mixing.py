"""
Random stem mixtures next to the hot path: what ``StemMixingDataset.__getitem__`` (reference
``timbre_trap/datasets/BaseDataset.py:272-332``) does per item -- 2 to 5 random stems, a random excerpt of each
(``AudioDataset.slice_audio``, ``AudioDataset.py:88-143``), the sum of their audio, the sum of the annotated stems' target maps clamped
to [0, 1] -- for a whole batch, from audio and annotations that stay on the device.

The random draws stay on the host and are the reference's, in its order (``StemMixer.plan``): they decide WHICH samples and frames a
mixture holds.  What scales with the batch runs in HIP kernels (csrc/mix.hip):

  tt_mix_audio    every stem's excerpt gathered from the resident ``AudioBank`` (slice or zero padding) and the groups summed
  tt_mix_targets  the annotated stems' float64 maps -- formed by ``PitchBank.targets`` -- summed per item and clamped

Summation order.  The reference adds with ``torch.sum(dim=0)`` on the CPU.  For 2 to 4 stems that equals an explicit loop over the
stems from zero, value for value, in float32 and float64; with 5 stems it does too except in the last (fewer than 64) elements of a
row, which torch's CPU sum adds in another grouping that depends on the host's vector width (tests/test_mix_restatement.py pins and
describes both).  The kernels' contract therefore is the explicit loop, in stem order, the audio-only group and the annotated group
added separately and then to each other (the ``+=`` of ``BaseDataset.py:320``): the reference's bits for every group of up to 4 stems,
and for a group of 5 up to a last-place unit in those last samples.  The sign of a zero is not part of the contract.
"""

import numpy as np
import torch

from .. import _hip
from .notes import _cuda_device
from .pitch import PitchBank
from .slicing import slice_times

__all__ = ['AudioBank', 'StemSource', 'StemMixer', 'mix_tiles', 'mix_targets']


def mix_tiles():
    """(output samples per workgroup of tt_mix_audio, output elements per workgroup of tt_mix_targets): the sizes the tests straddle."""
    lib = _hip.lib()
    return lib.tt_mix_tile(), lib.tt_mix_targets_tile()


def _int_table(values, dtype, what):
    a = np.asarray(values)
    if a.size and a.dtype.kind not in 'iu':
        raise TypeError('%s must be integers (got %s)' % (what, a.dtype))
    return np.ascontiguousarray(a.reshape(-1), dtype=dtype)


def _check_item_off(item_off, n_stems):
    if item_off.size < 1 or item_off[0] != 0 or item_off[-1] != n_stems or (np.diff(item_off) < 0).any():
        raise ValueError('item_off must run from 0 to the number of stems (%d) without decreasing' % n_stems)


def mix_targets(maps, item_off, dtype=torch.float32, out=None):
    """
    ``torch.sum(maps[item_off[b]:item_off[b + 1]], dim=0).clamp(0, 1)`` of every item b (``BaseDataset.py:323``), added in float64 in
    stem order: (B, F, T) in ``dtype`` -- ``torch.float64``, or ``torch.float32`` = its ``.float()`` (``train.py:394``).  ``maps``: float64
    (S, F, T) on the device, e.g. what ``PitchBank.targets(..., dtype=torch.float64)`` or stacked ``notes_to_activations`` maps give.
    An item without a map is zeros.  One launch (tt_mix_targets).  ``out``: a contiguous (B, F, T) device tensor of ``dtype`` to write into.
    """
    if dtype not in (torch.float32, torch.float64):
        raise ValueError('dtype must be torch.float32 or torch.float64 (got %s)' % dtype)
    _hip.require_cuda(maps)
    if maps.dtype != torch.float64 or maps.dim() != 3:
        raise ValueError('maps must be float64 (S, F, T) (got %s %s)' % (maps.dtype, tuple(maps.shape)))
    maps = maps.contiguous()
    S, F, T = maps.shape
    off = _int_table(item_off, np.int32, 'item_off')
    _check_item_off(off, S)
    B = len(off) - 1
    if out is None:
        out = torch.empty((B, F, T), dtype=dtype, device=maps.device)
    elif out.shape != (B, F, T) or out.dtype != dtype or out.device != maps.device or not out.is_contiguous():
        raise ValueError('out must be a contiguous %s tensor of shape %s on %s' % (dtype, (B, F, T), maps.device))
    if B * F * T:
        off_d = torch.from_numpy(off).to(maps.device)
        with torch.cuda.device(maps.device):
            _hip.check(_hip.lib().tt_mix_targets(_hip.ptr(maps) if S else None, _hip.ptr(off_d), B, F, T, int(dtype == torch.float32),
                                                 _hip.ptr(out), _hip.stream_ptr()), 'tt_mix_targets')
    return out


class AudioBank:
    """
    The audio of a dataset, resident on the device.  ``tracks``: a sequence of ``1 x N`` or ``N`` float32 tensors as ``prepare_audio``
    returns them (on any device); they are concatenated into one arena on ``device`` here, once, and the ``(base, length)`` table is kept
    on the host (``table``) and on the device.  ``excerpts`` and ``mix`` then cut and sum any batch of excerpts in one launch.
    The bank belongs in the process that drives the device.  A non-CUDA ``device`` raises ``RuntimeError``: there is no CPU fallback.
    """

    def __init__(self, tracks, device='cuda'):
        self.device = _cuda_device(device)
        flat = []
        for n, t in enumerate(tracks):
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() > 2 or (t.dim() == 2 and t.size(0) != 1):
                raise ValueError('track %d: expected a float32 tensor of shape (1, N) or (N)' % n)
            flat.append(t.reshape(-1))
        self.table = np.zeros((len(flat), 2), dtype=np.int64)
        self.table[:, 1] = [len(t) for t in flat]
        self.table[1:, 0] = np.cumsum(self.table[:-1, 1])
        # one allocation, filled track by track: no second copy of the dataset on the device
        self.arena = torch.empty(int(self.table[:, 1].sum()), dtype=torch.float32, device=self.device)
        for (base, length), t in zip(self.table, flat):
            self.arena[base:base + length].copy_(t)
        self.table_d = torch.from_numpy(self.table.reshape(-1)).to(self.device)
        self.device = self.arena.device

    def __len__(self):
        return len(self.table)

    def mix(self, stem_track, stem_start, item_off, item_split, n_samples):
        """
        (B, 1, n_samples) float32 on the device: item b is the sum of its stems ``item_off[b] .. item_off[b + 1]``, the first
        ``item_split[b]`` of them (audio-only group) and the rest (annotated group) added separately in stem order and then to each
        other.  Stem s is track ``stem_track[s]`` from sample ``stem_start[s]``; a negative start is that much silence in front of the
        track, and silence follows its end.  One launch (tt_mix_audio).  An id outside the bank raises ``IndexError``.
        """
        trk = _int_table(stem_track, np.int32, 'stem_track')
        start = _int_table(stem_start, np.int64, 'stem_start')
        off = _int_table(item_off, np.int32, 'item_off')
        split = _int_table(item_split, np.int32, 'item_split')
        S, B, N = len(trk), len(off) - 1, int(n_samples)
        if start.shape != trk.shape or N < 0:
            raise ValueError('stem_track and stem_start must have one entry per stem, n_samples >= 0')
        _check_item_off(off, S)
        if split.shape != (B,) or (split < 0).any() or (split > np.diff(off)).any():
            raise ValueError('item_split must hold, per item, a count between 0 and its number of stems')
        if S and (trk.min() < 0 or trk.max() >= len(self.table)):
            raise IndexError('track id outside [0, %d)' % len(self.table))
        y = torch.empty((B, 1, N), dtype=torch.float32, device=self.device)
        if B * N:
            # one upload for the four tables: int64 [S] starts, then int32 [S] ids, [B + 1] offsets, [B] splits
            packed = np.concatenate([start.view(np.int32), trk, off, split])
            packed_d = torch.from_numpy(packed).to(self.device)
            p0 = packed_d.data_ptr()
            at = lambda n: _hip.c_void_p(p0 + 4 * n)                              # noqa: E731
            with torch.cuda.device(self.device):
                _hip.check(_hip.lib().tt_mix_audio(_hip.ptr(self.arena), _hip.ptr(self.table_d), len(self.table), at(2 * S), at(0),
                                                   at(3 * S), at(3 * S + B + 1), B, N, _hip.ptr(y), _hip.stream_ptr()), 'tt_mix_audio')
        return y

    def excerpts(self, track_ids, starts, n_samples):
        """``slice_audio(track, n_samples, offset_s)`` of every (track id, start) pair, stacked: (B, 1, n_samples).  ``starts[b] >= 0``
        is the first sample of the slice, ``-pad_left`` the zero padding of a track shorter than the excerpt."""
        B = len(np.asarray(track_ids).reshape(-1))
        return self.mix(track_ids, starts, np.arange(B + 1), np.zeros(B, dtype=np.int64), n_samples)


class StemSource:
    """
    One pre-instantiated dataset of the reference as ``StemMixer`` sees it.  ``audio``: its tracks' prepared audio (``1 x N`` or ``N``
    float32 tensors, in the dataset's track order); ``annotations``: ``None`` for an ``AudioDataset``, or the list of
    ``(times, multi_pitch)`` that ``get_ground_truth`` returns per track for an ``MPEDataset``.  It owns ``RandomState(seed)`` like the
    dataset does (``BaseDataset.py:60``): the excerpt offsets of its stems are drawn from it.
    """

    def __init__(self, audio, annotations=None, seed=0):
        self.audio = list(audio)
        self.annotations = None if annotations is None else list(annotations)
        if self.annotations is not None and len(self.annotations) != len(self.audio):
            raise ValueError('%d annotations for %d tracks' % (len(self.annotations), len(self.audio)))
        self.lengths = [int(a.shape[-1]) for a in self.audio]
        self.rng = np.random.RandomState(seed)

    def __len__(self):
        return len(self.audio)


class StemMixer:
    """
    ``StemMixingDataset(datasets, tracks_per_epoch, n_min, n_max, seed)`` (``BaseDataset.py:222-332``) over ``sources`` (``StemSource``
    objects in the order of ``datasets``), for whole batches: ``plan`` makes the reference's random draws on the host, ``batch`` cuts,
    sums and clamps on the device.  ``cqt``: the transform whose frame grid, sample rate and bins the datasets share; ``n_secs``: the
    excerpt length every dataset was given.  The first ``batch`` (or ``upload``) puts all audio into one ``AudioBank`` and all annotations
    into one ``PitchBank``, once; a non-CUDA ``device`` raises ``RuntimeError`` here.  ``map_budget_bytes`` bounds the float64 stem maps
    alive at once in ``batch``.
    """

    def __init__(self, sources, cqt, n_secs, tracks_per_epoch, n_min=2, n_max=5, seed=0, n_bins_blur_decay=2.5, device='cuda',
                 map_budget_bytes=256 << 20):
        dev = _cuda_device(device)
        if n_min > n_max or n_min < 0:
            raise ValueError('need 0 <= n_min <= n_max (got %s, %s)' % (n_min, n_max))
        self.sources = list(sources)
        self.cqt, self.n_secs, self.tracks_per_epoch = cqt, n_secs, tracks_per_epoch
        self.n_min, self.n_max = n_min, n_max
        self.n_bins_blur_decay, self.map_budget_bytes = n_bins_blur_decay, int(map_budget_bytes)
        self.sample_rate = cqt.sample_rate
        self.n_samples = int(n_secs * self.sample_rate)                           # slice_audio's default (AudioDataset.py:111)
        self.n_frames = cqt.get_expected_frames(cqt.get_expected_samples(n_secs))  # slice_times' default (PitchDataset.py:100-104)
        self.rng = np.random.RandomState(seed)                                    # BaseDataset.py:255
        # the ComboDataset index space (BaseDataset.py:208-214): global index (= id in the audio bank) -> source, id in the pitch bank or -1
        self._source_of, self._pitch_id, annotations = [], [], []
        for k, src in enumerate(self.sources):
            for n in range(len(src)):
                self._source_of.append(k)
                self._pitch_id.append(-1 if src.annotations is None else len(annotations))
                if src.annotations is not None:
                    annotations.append(src.annotations[n])
        self._lengths = [n for src in self.sources for n in src.lengths]
        self._track_times = {}
        self._annotations = annotations
        self.device, self.audio_bank, self.pitch_bank = dev, None, None

    def upload(self):
        """All audio into one ``AudioBank`` and all annotations into one ``PitchBank`` (``None`` without annotations), once; ``batch``
        calls this on first use, so that ``plan`` needs no device."""
        if self.audio_bank is None:
            self.audio_bank = AudioBank([a for src in self.sources for a in src.audio], self.device)
            if self._annotations:
                self.pitch_bank = PitchBank(self._annotations, self.cqt.get_midi_freqs(), None, self.device)
            self.device = self.audio_bank.device
        return self

    def __len__(self):
        return self.tracks_per_epoch

    def _full_track_times(self, g):
        """``cqt.get_times(cqt.get_expected_frames(n_samples))`` of track g (``PitchDataset.py:175``), formed once per track."""
        if g not in self._track_times:
            self._track_times[g] = self.cqt.get_times(self.cqt.get_expected_frames(self._lengths[g]))
        return self._track_times[g]

    def plan(self, indices):
        """
        The draws of ``StemMixingDataset.__getitem__`` for every index, in order -- host only, no device work.  Per item: the number of
        stems from the mixer's generator, a shuffle of the whole index space, then per chosen stem, in the shuffled order, one offset
        from ITS source's generator with the bounds of ``slice_audio`` (a track at least as long as the excerpt: a start in
        ``[0, n - n_samples]``; a shorter one: ``pad_left`` in ``[0, pad_total)``, stored as ``-pad_left``).  An annotated stem's frame
        times are ``slice_times(full track times, offset_t=offset_t)`` (``MPEDataset.py:73-80``, ``PitchDataset.py:175-179``), which
        draws nothing.  Within an item the audio-only stems come first, then the annotated ones, each group in drawn order
        (``separate_ground_truth``).  Returns a dict of the flat tables the kernels take -- ``stem_track`` int32 (S) (bank ids =
        global indices), ``stem_start`` int64 (S), ``item_off`` int32 (B + 1), ``item_split`` int32 (B) -- plus ``n_mix`` (B),
        ``drawn`` (the stems in drawn order, before grouping: list of B lists of (global index, start)), and per annotated stem, in
        table order, ``pitch_track`` int64 (A) (ids in the pitch bank), ``pitch_times`` float64 (A, T) and ``pitch_off`` int32 (B + 1).
        """
        total = len(self._lengths)
        stem_track, stem_start, item_off, item_split, n_mixes, drawn = [], [], [0], [], [], []
        pitch_track, pitch_times, pitch_off = [], [], [0]
        for _ in indices:
            n_mix = self.rng.randint(self.n_min, self.n_max + 1)
            idcs = np.arange(total)
            self.rng.shuffle(idcs)
            audio_only, annotated, order = [], [], []
            for g in idcs[:n_mix]:
                g = int(g)
                n, rng = self._lengths[g], self.sources[self._source_of[g]].rng
                if n >= self.n_samples:
                    start = int(rng.randint(0, n - self.n_samples + 1))
                else:
                    start = -int(rng.randint(0, self.n_samples - n))
                order.append((g, start))
                if self._pitch_id[g] < 0:
                    audio_only.append((g, start))
                else:
                    annotated.append((g, start))
                    times, _ = slice_times(self._full_track_times(g), offset_t=start / self.sample_rate, cqt=self.cqt, n_secs=self.n_secs,
                                           sample_rate=self.sample_rate)
                    pitch_track.append(self._pitch_id[g])
                    pitch_times.append(times)
            for g, start in audio_only + annotated:
                stem_track.append(g)
                stem_start.append(start)
            item_off.append(len(stem_track))
            item_split.append(len(audio_only))
            pitch_off.append(len(pitch_track))
            n_mixes.append(n_mix)
            drawn.append(order)
        return dict(stem_track=np.array(stem_track, dtype=np.int32), stem_start=np.array(stem_start, dtype=np.int64),
                    item_off=np.array(item_off, dtype=np.int32), item_split=np.array(item_split, dtype=np.int32),
                    n_mix=np.array(n_mixes, dtype=np.int64), drawn=drawn, pitch_track=np.array(pitch_track, dtype=np.int64),
                    pitch_times=np.array(pitch_times, dtype=np.float64).reshape(len(pitch_track), self.n_frames),
                    pitch_off=np.array(pitch_off, dtype=np.int32))

    def _chunks(self, pitch_off):
        """Runs of whole items [b0, b1) whose annotated stems' float64 maps fit ``map_budget_bytes`` (one item at least)."""
        per_map = len(self.pitch_bank.midi_freqs) * self.n_frames * 8
        most = max(1, self.map_budget_bytes // max(1, per_map))
        B, b0 = len(pitch_off) - 1, 0
        while b0 < B:
            b1 = b0 + 1
            while b1 < B and pitch_off[b1 + 1] - pitch_off[b0] <= most:
                b1 += 1
            yield b0, b1
            b0 = b1

    def batch(self, indices, dtype=torch.float32):
        """
        The mixtures of ``indices`` as one batch, with the reference's keys: ``track`` = ``[str(index), ...]``; ``audio`` (B, 1, N)
        float32 on the device; and, when a source has annotations, ``ground_truth`` (B, F, T) on the device in ``dtype`` --
        ``torch.float64`` is the reference's array bit for bit, ``torch.float32`` its ``.float()`` -- ``times`` (B, T) float64 ndarray,
        the times of each item's first annotated stem (``BaseDataset.py:326``; NaN rows for items without one), and ``annotated`` bool
        (B).  An item without an annotated stem has a zero map.  ``plan``, one tt_mix_audio launch, then per chunk of whole items one
        ``PitchBank.targets(..., dtype=torch.float64)`` and one tt_mix_targets launch.
        """
        if dtype not in (torch.float32, torch.float64):
            raise ValueError('dtype must be torch.float32 or torch.float64 (got %s)' % dtype)
        indices = list(indices)
        self.upload()
        p = self.plan(indices)
        data = {'track': [str(i) for i in indices],
                'audio': self.audio_bank.mix(p['stem_track'], p['stem_start'], p['item_off'], p['item_split'], self.n_samples)}
        if self.pitch_bank is None:
            return data
        B, F, T = len(indices), len(self.pitch_bank.midi_freqs), self.n_frames
        off = p['pitch_off']
        gt = torch.empty((B, F, T), dtype=dtype, device=self.device)
        for b0, b1 in self._chunks(off):
            s0, s1 = off[b0], off[b1]
            maps = self.pitch_bank.targets(p['pitch_track'][s0:s1], p['pitch_times'][s0:s1], self.n_bins_blur_decay, torch.float64) \
                if s1 > s0 else torch.empty((0, F, T), dtype=torch.float64, device=self.device)
            mix_targets(maps, off[b0:b1 + 1] - s0, dtype, out=gt[b0:b1])
        annotated = np.diff(off) > 0
        times = np.full((B, T), np.nan)
        times[annotated] = p['pitch_times'][off[:-1][annotated]]
        data.update(ground_truth=gt, times=times, annotated=annotated)
        data['ground-truth'] = gt                                                  # the spelling of the reference's constants.KEY_GROUND_TRUTH
        return data
