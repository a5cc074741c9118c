"""
Note events from activation maps: the way back from ``utils/notes.py``.  ``TimbreTrap.transcribe`` ends at a (B, F, T) map and
``peaks_above`` / ``mpe_compact`` turn it into per-frame bin lists; here the map becomes notes -- pitch row, onset frame, end frame,
strength -- without leaving the device (csrc/events.hip), and the notes become the arrays ``NoteDataset.get_ground_truth`` returns or a
Standard MIDI File.  The reference has no counterpart: it stops at frame-level estimates.

  tt_events_mask     one 64-bit word per (item, pitch row, 64 frames): which frames of the row hold a bin that passes the predicate of
                     ``peaks_above`` (peaks_only) / ``threshold``
  tt_events_count    per word, how many notes start and how many end in it, gaps of up to ``max_gap`` frames bridged
  (two prefix sums)  note slots in ascending (item, row, onset) order; ONE total comes back to size the arrays
  tt_events_fill     item, row, onset, end of every candidate note
  tt_events_finish   active frames, peak value and the ``min_frames`` verdict per candidate

Everything is an integer or an exact fp32 maximum, so the results can be compared with ``==``.
"""

import struct
from collections import namedtuple

import numpy as np
import torch

from .. import _hip

__all__ = ['NoteEvents', 'note_events', 'events_to_notes', 'write_midi']

NoteEvents = namedtuple('NoteEvents', ('item', 'row', 'onset', 'end', 'n_active', 'peak', 'pitch'))
NoteEvents.__doc__ = """Notes as device tensors of one length, in ascending (item, row, onset) order (or per item by (onset, row)): ``item``,
``row``, ``onset``, ``end`` (exclusive), ``n_active`` int32; ``peak`` float32; ``pitch`` float64 MIDI numbers."""

MAX_GAP = 63                                   # what one neighbouring mask word can bridge


def _event_activations(activations):
    if not isinstance(activations, torch.Tensor):
        raise RuntimeError('note events are formed on the device from a GPU tensor of activations (got %s)' % type(activations).__name__)
    _hip.require_cuda(activations)
    x = activations.detach()
    if x.dim() == 2:
        x = x[None]
    if x.dim() != 3:
        raise ValueError('activations must be (F, T) or (B, F, T) (got %s)' % (tuple(activations.shape),))
    if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError('unsupported dtype %s' % x.dtype)
    return x.to(torch.float32).contiguous()


def _pitch_rows(midi_freqs, F, resolution, bin_groups):
    """(group_off int32 [P + 1], pitch float64 [P]) on the host."""
    midi_freqs = np.asarray(midi_freqs, dtype=np.float64)
    if midi_freqs.shape != (F,):
        raise ValueError('midi_freqs must hold one value per bin (%d), got shape %s' % (F, midi_freqs.shape))
    if bin_groups is not None:
        off = np.asarray(bin_groups)
        if off.ndim != 1 or len(off) < 1 or not np.issubdtype(off.dtype, np.integer):
            raise ValueError('bin_groups must be a 1-d table of integer offsets')
        off = off.astype(np.int64)
        if np.any(off[1:] < off[:-1]) or off[0] < 0 or off[-1] > F:
            raise ValueError('bin_groups must be ascending and lie within [0, %d]' % F)
        sums = np.concatenate([[0.0], np.cumsum(midi_freqs)])
        n = np.diff(off)
        with np.errstate(invalid='ignore', divide='ignore'):
            pitch = np.where(n > 0, (sums[off[1:]] - sums[off[:-1]]) / n, np.nan)         # the mean of the row's bins; an empty row has none
        return off.astype(np.int32), pitch
    if resolution == 'bin':
        return np.arange(F + 1, dtype=np.int32), midi_freqs.copy()
    if resolution != 'semitone':
        raise ValueError("resolution must be 'semitone' or 'bin' (got %r)" % (resolution,))
    if F == 0:
        return np.zeros(1, dtype=np.int32), np.empty(0)
    if np.any(midi_freqs[1:] < midi_freqs[:-1]) or not np.all(np.isfinite(midi_freqs)):
        raise ValueError('midi_freqs must be finite and ascending to be grouped by semitone')
    semi = np.floor(midi_freqs + 0.5).astype(np.int64)
    numbers = np.arange(semi[0], semi[-1] + 1)
    off = np.concatenate([np.searchsorted(semi, numbers, side='left'), [F]])
    return off.astype(np.int32), numbers.astype(np.float64)


def _empty(dev):
    i32 = lambda: torch.empty(0, dtype=torch.int32, device=dev)                           # noqa: E731
    return NoteEvents(i32(), i32(), i32(), i32(), i32(), torch.empty(0, dtype=torch.float32, device=dev),
                      torch.empty(0, dtype=torch.float64, device=dev))


def note_events(activations, midi_freqs, t=0.5, peaks_only=True, n_valid_bins=0, resolution='semitone', bin_groups=None, max_gap=0,
                min_frames=1, order='pitch'):
    """
    Notes from ``activations`` -- a CUDA fp32 / fp16 / bf16 tensor (F, T) or (B, F, T), 16-bit upcast to fp32 -- as a ``NoteEvents`` tuple
    of device tensors.  CPU tensors raise ``RuntimeError``: there is no CPU fallback.

    A bin is active where ``peaks_above(x, t, n_valid_bins)`` (``peaks_only``) or ``threshold`` of the masked map is 1.  Bins are grouped
    into pitch rows: ``resolution='semitone'`` puts bin f into the row of ``floor(midi_freqs[f] + 0.5)`` (``pitch`` = that number),
    ``'bin'`` gives every bin its own row (``pitch = midi_freqs[f]``), ``bin_groups`` -- an ascending table of P + 1 offsets within
    [0, F] -- makes row p of the bins ``[bin_groups[p], bin_groups[p + 1])`` (``pitch`` = the mean of their ``midi_freqs``; NaN for an
    empty row, which never sounds).  A frame of a row is active when one of its bins is.  Runs of at most ``max_gap`` (0..63) inactive
    frames between two active ones are bridged; every maximal run of the result is a note from ``onset`` to ``end`` (exclusive, so
    ``end - onset`` frames), kept if it spans at least ``min_frames`` frames.  ``n_active`` counts the active frames of the note and
    ``peak`` is the largest activation among its active bins, an exact fp32 value of the map.

    The defaults ``max_gap=0, min_frames=1`` are the neutral ones -- the notes are exactly the runs of active frames.  Which values
    score best on real transcriptions has not been measured; choose them on data.

    ``order='pitch'``: ascending (item, row, onset).  ``order='onset'``: per item by (onset, row), through a stable device sort.
    """
    x = _event_activations(activations)
    B, F, T = x.shape
    if order not in ('pitch', 'onset'):
        raise ValueError("order must be 'pitch' or 'onset' (got %r)" % (order,))
    max_gap, min_frames = int(max_gap), int(min_frames)
    if not 0 <= max_gap <= MAX_GAP:
        raise ValueError('max_gap must lie in [0, %d] (got %d)' % (MAX_GAP, max_gap))
    if min_frames < 1:
        raise ValueError('min_frames must be at least 1 (got %d)' % min_frames)
    group_off, pitch = _pitch_rows(midi_freqs, F, resolution, bin_groups)
    P, dev = len(group_off) - 1, x.device
    if B == 0 or F == 0 or T == 0 or P == 0:
        return _empty(dev)
    lib = _hip.lib()
    mode = 2 if peaks_only else 1
    W = (T + 63) // 64
    off_d = torch.from_numpy(group_off).to(dev)
    mask = torch.empty(B * P * W, dtype=torch.int64, device=dev)
    n_on = torch.empty(B * P * W, dtype=torch.int32, device=dev)
    n_end = torch.empty_like(n_on)
    with torch.cuda.device(dev):
        st = _hip.stream_ptr()
        _hip.check(lib.tt_events_mask(_hip.ptr(x), B, F, T, float(t), mode, int(n_valid_bins), _hip.ptr(off_d), P, _hip.ptr(mask), st),
                   'tt_events_mask')
        _hip.check(lib.tt_events_count(_hip.ptr(mask), B, P, T, max_gap, _hip.ptr(n_on), _hip.ptr(n_end), st), 'tt_events_count')
        on_sum = torch.cumsum(n_on, 0, dtype=torch.int64)
        total = int(on_sum[-1])                                       # the first of at most two values that come back
        if total == 0:
            return _empty(dev)
        on_off = on_sum - n_on
        end_off = torch.cumsum(n_end, 0, dtype=torch.int64) - n_end
        item, row, onset, end, n_active, keep = (torch.empty(total, dtype=torch.int32, device=dev) for _ in range(6))
        peak = torch.empty(total, dtype=torch.float32, device=dev)
        _hip.check(lib.tt_events_fill(_hip.ptr(mask), B, P, T, max_gap, _hip.ptr(on_off), _hip.ptr(end_off), total, _hip.ptr(item),
                                      _hip.ptr(row), _hip.ptr(onset), _hip.ptr(end), st), 'tt_events_fill')
        _hip.check(lib.tt_events_finish(_hip.ptr(x), B, F, T, float(t), mode, int(n_valid_bins), _hip.ptr(off_d), P, _hip.ptr(mask),
                                        _hip.ptr(item), _hip.ptr(row), _hip.ptr(onset), _hip.ptr(end), total, min_frames, _hip.ptr(n_active),
                                        _hip.ptr(peak), _hip.ptr(keep), st), 'tt_events_finish')
        fields = [item, row, onset, end, n_active, peak]
        if min_frames > 1:                                            # every candidate spans a frame: nothing to drop at 1
            kept = torch.nonzero(keep, as_tuple=False).squeeze(1)     # the second value that comes back: how many are kept
            fields = [f.index_select(0, kept) for f in fields]
        if order == 'onset' and fields[0].numel():
            by_onset = torch.argsort(fields[2], stable=True)          # (onset, item, row) ...
            perm = by_onset[torch.argsort(fields[0][by_onset], stable=True)]          # ... then (item, onset, row)
            fields = [f[perm] for f in fields]
        return NoteEvents(*fields, torch.from_numpy(pitch).to(dev)[fields[1].long()])


def events_to_notes(events, hop_seconds, item=0):
    """
    The notes of one batch item on the host, in the shape ``NoteDataset.get_ground_truth`` returns: ``(pitches float64 [L], intervals
    float64 [L, 2])`` with onset / offset in seconds.  ``hop_seconds``: seconds per frame, or the pair ``(hop_length, sample_rate)`` --
    then the times are ``frame * hop_length / sample_rate``, the arithmetic of ``CQT.get_times``, so an onset is exactly the time of its
    frame and ``end == T`` is one hop past the last frame without any extrapolation.
    """
    sel = (events.item == int(item)).cpu().numpy()
    frames = np.stack([events.onset.cpu().numpy()[sel], events.end.cpu().numpy()[sel]], axis=1).astype(np.int64).reshape(-1, 2)
    if isinstance(hop_seconds, (tuple, list)):
        hop_length, sample_rate = hop_seconds
        intervals = frames * hop_length / sample_rate
    else:
        intervals = frames * float(hop_seconds)
    return events.pitch.cpu().numpy()[sel].astype(np.float64), intervals.astype(np.float64)


def _vlq(n):
    """A MIDI variable-length quantity: seven bits per byte, most significant first, the top bit set on all but the last."""
    out = [n & 0x7F]
    n >>= 7
    while n:
        out.append(0x80 | (n & 0x7F))
        n >>= 7
    return bytes(reversed(out))


def write_midi(file, pitches, intervals, velocities=None, tempo_bpm=120, ticks_per_beat=480):
    """
    Notes -> a format-0 Standard MIDI File (header chunk, one track: a tempo meta event, note-on / note-off events on channel 0 with
    variable-length delta times, end-of-track), written byte by byte: no MIDI package is needed.  ``file``: a path or a binary file
    object.  ``pitches`` in MIDI numbers, rounded and clipped to 0..127; ``intervals`` (L, 2) in seconds, converted to ticks as
    ``round(seconds * ticks_per_beat * tempo_bpm / 60)``.  Events are ordered by (tick, note-off before note-on, pitch).
    ``velocities``: one strength per note on the scale of the activations, such as ``NoteEvents.peak``; the velocity byte is
    ``1 + round(126 * clip(strength, 0, 1))``, so it is never 0 (a note-on with velocity 0 means note-off).  None: strength 0.5
    throughout, velocity 64.  Returns the bytes written.
    """
    pitches = np.asarray(pitches, dtype=np.float64).ravel()
    intervals = np.asarray(intervals, dtype=np.float64).reshape(-1, 2)
    if len(pitches) != len(intervals):
        raise ValueError('pitches (%d) and intervals (%d) must hold one entry per note' % (len(pitches), len(intervals)))
    if not 1 <= int(ticks_per_beat) <= 0x7FFF:
        raise ValueError('ticks_per_beat must lie in [1, 32767]')
    if not (np.all(np.isfinite(pitches)) and np.all(np.isfinite(intervals)) and np.all(intervals >= 0)):
        raise ValueError('pitches and times must be finite, times non-negative')
    note = np.clip(np.rint(pitches), 0, 127).astype(np.int64)
    strength = np.full(len(note), 0.5) if velocities is None else np.asarray(velocities, dtype=np.float64).ravel()
    if len(strength) != len(note):
        raise ValueError('velocities must hold one entry per note')
    vel = 1 + np.rint(126.0 * np.clip(np.nan_to_num(strength, nan=0.0), 0.0, 1.0)).astype(np.int64)
    ticks = np.rint(intervals * ticks_per_beat * tempo_bpm / 60.0).astype(np.int64)
    events = [(int(on), 1, int(n), int(v)) for (on, _), n, v in zip(ticks, note, vel)]
    events += [(int(off), 0, int(n), 0) for (_, off), n in zip(ticks, note)]
    events.sort(key=lambda e: e[:3])
    track = bytearray(b'\x00\xff\x51\x03' + struct.pack('>I', int(round(60e6 / tempo_bpm)))[1:])
    now = 0
    for tick, is_on, n, v in events:
        track += _vlq(tick - now) + bytes([0x90 if is_on else 0x80, n, v])
        now = tick
    track += b'\x00\xff\x2f\x00'
    data = b'MThd' + struct.pack('>IHHH', 6, 0, 1, int(ticks_per_beat)) + b'MTrk' + struct.pack('>I', len(track)) + bytes(track)
    if hasattr(file, 'write'):
        file.write(data)
    else:
        with open(file, 'wb') as f:
            f.write(data)
    return data
