"""
Pitch contours and pitch bends: what the five bins per semitone of the map are for.  ``note_events`` (utils/events.py) reports a note
as a pitch row and ``activations_to_multi_pitch`` reports bin centres; here every frame of a note, and every entry of the per-frame bin
lists, gets a pitch refined below the bin spacing by a parabola through the bin and its two neighbours along F -- on the device
(csrc/contours.hip), from the map where ``transcribe`` left it -- and the notes become a Standard MIDI File with pitch bends.  The
reference has no counterpart: it stops at per-frame lists of bin centres.

  tt_contours_notes   per frame of every note: the strongest passing bin of the note's row, its value, the sub-bin offset ``delta`` in
                      [-0.5, 0.5] bins, the pitch in float64 MIDI numbers, the bend in integer units against the row's pitch; per note
                      the count, sum, minimum and maximum of the bends over its voiced frames
  tt_contours_frames  ``delta`` and pitch of every entry of the lists ``mpe_compact`` returns

The semantics are stated in include/ttrap.h and restated in NumPy by tests/contours_ref.py; every result is an integer, an exact fp32
value or a float64 value formed by a fixed sequence of individually rounded operations, so the two are compared with ``==``.
"""

import struct
from collections import namedtuple

import numpy as np
import torch

from .. import _hip
from .events import _event_activations, _pitch_rows, _vlq
from .metrics.mpe import _mpe_activations, mpe_compact

__all__ = ['NoteContours', 'note_contours', 'refined_pitches', 'refine_multi_pitch', 'activations_to_multi_pitch_refined',
           'contours_to_bends', 'write_midi_bends']

NoteContours = namedtuple('NoteContours', ('frame_off', 'bin', 'delta', 'value', 'pitch', 'bend', 'n_voiced', 'bend_sum', 'bend_min',
                                           'bend_max', 'units'))
NoteContours.__doc__ = """Contours of L notes as device tensors.  ``frame_off`` int64 [L + 1]: note i owns the slots
``frame_off[i]:frame_off[i + 1]``, one per frame from its onset to its end.  Per slot: ``bin`` int32 (-1: no bin of the row passes in
that frame -- it was bridged by ``max_gap``), ``delta`` float32 in [-0.5, 0.5] bins, ``value`` float32 (the map at ``bin``), ``pitch``
float64 MIDI (NaN at ``bin == -1``), ``bend`` int32 in units of ``1 / units`` semitone against the note's ``pitch``.  Per note, over
its frames with ``bin >= 0``: ``n_voiced`` int32, ``bend_sum`` int64, ``bend_min`` / ``bend_max`` int32.  ``units``: a Python int."""


def _empty(dev, units):
    z = lambda dtype, n=0: torch.zeros(n, dtype=dtype, device=dev)                        # noqa: E731
    return NoteContours(z(torch.int64, 1), z(torch.int32), z(torch.float32), z(torch.float32), z(torch.float64), z(torch.int32),
                        z(torch.int32), z(torch.int64), z(torch.int32), z(torch.int32), units)


def note_contours(activations, events, midi_freqs, t=0.5, peaks_only=True, n_valid_bins=0, resolution='semitone', bin_groups=None,
                  units_per_semitone=4096):
    """
    The pitch contour of every note of ``events`` (a ``NoteEvents`` tuple, in either order) on ``activations`` -- the CUDA fp32 / fp16
    / bf16 map (F, T) or (B, F, T) the events were formed from, 16-bit upcast to fp32 -- as a ``NoteContours`` tuple of device tensors.
    CPU tensors raise ``RuntimeError``: there is no CPU fallback.  An empty ``events`` returns empty tensors without a launch.

    ``t``, ``peaks_only``, ``n_valid_bins``, ``resolution`` and ``bin_groups`` MUST be the ones ``note_events`` was called with: they
    decide which bins pass and which bins a row owns, and a note is followed through the passing bins of its own row.  ``ValueError``
    if a row of ``events`` does not exist under this grouping.

    Per frame of a note, among the bins of its row that pass the predicate the one with the largest activation (ties: the lowest) is
    refined: with b the map at the bin and a, c at the bins below and above (zero beyond the ends and from ``n_valid_bins`` upwards),
    ``delta = 0.5 (a - c) / ((a - b) + (c - b))`` clamped to [-0.5, 0.5] -- the vertex of the parabola through the three -- and 0 when
    b is not the largest of the three, the three are equal or one is not finite; ``pitch = midi_freqs[bin] + delta * (the spacing of
    midi_freqs towards the side delta points to)`` in float64; ``bend = rint((pitch - events.pitch) * units_per_semitone)``.  The
    contour is not smoothed.
    """
    x = _event_activations(activations)
    B, F, T = x.shape
    units = int(units_per_semitone)
    if units < 1 or units > 1 << 20:
        raise ValueError('units_per_semitone must lie in [1, 2^20] (got %r)' % (units_per_semitone,))
    group_off, row_pitch = _pitch_rows(midi_freqs, F, resolution, bin_groups)
    P, dev = len(group_off) - 1, x.device
    for f in events[:6]:
        _hip.require_cuda(f)
    L = events.item.numel()
    if L == 0 or B == 0 or F == 0 or T == 0 or P == 0:
        return _empty(dev, units)
    item, row, onset, end = (f.to(torch.int32).contiguous() for f in (events.item, events.row, events.onset, events.end))
    frames = (end - onset).clamp_min(0)
    frame_off = torch.zeros(L + 1, dtype=torch.int64, device=dev)
    frame_off[1:] = torch.cumsum(frames, 0, dtype=torch.int64)
    top_row, total = (int(v) for v in torch.stack([row.max().long(), frame_off[-1]]).tolist())      # the one read: sizes the arrays
    if top_row >= P:
        raise ValueError('events hold row %d but the grouping has %d rows: pass the grouping arguments the events were made with'
                         % (top_row, P))
    bin_, bend = (torch.empty(total, dtype=torch.int32, device=dev) for _ in range(2))
    delta, value = (torch.empty(total, dtype=torch.float32, device=dev) for _ in range(2))
    pitch = torch.empty(total, dtype=torch.float64, device=dev)
    n_voiced, bend_min, bend_max = (torch.empty(L, dtype=torch.int32, device=dev) for _ in range(3))
    bend_sum = torch.empty(L, dtype=torch.int64, device=dev)
    off_d = torch.from_numpy(group_off).to(dev)
    m_d = torch.from_numpy(np.array(midi_freqs, dtype=np.float64)).to(dev)         # (a copy: the caller's table may be read-only)
    rp_d = torch.from_numpy(np.array(row_pitch, dtype=np.float64)).to(dev)
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().tt_contours_notes(
            _hip.ptr(x), B, F, T, float(t), 2 if peaks_only else 1, int(n_valid_bins), _hip.ptr(off_d), P, _hip.ptr(m_d), _hip.ptr(rp_d),
            units, _hip.ptr(item), _hip.ptr(row), _hip.ptr(onset), _hip.ptr(end), L, _hip.ptr(frame_off), _hip.ptr(bin_), _hip.ptr(delta),
            _hip.ptr(value), _hip.ptr(pitch), _hip.ptr(bend), _hip.ptr(n_voiced), _hip.ptr(bend_sum), _hip.ptr(bend_min),
            _hip.ptr(bend_max), _hip.stream_ptr()), 'tt_contours_notes')
    return NoteContours(frame_off, bin_, delta, value, pitch, bend, n_voiced, bend_sum, bend_min, bend_max, units)


def refined_pitches(events, contours):
    """One pitch per note, float64 [L] on the device: ``events.pitch`` plus the mean bend of the note's voiced frames,
    ``bend_sum / (n_voiced * units)``; ``events.pitch`` itself where the note has no voiced frame."""
    n = contours.n_voiced.double() * float(contours.units)
    mean = contours.bend_sum.double() / torch.where(n > 0, n, torch.ones_like(n))
    return torch.where(n > 0, events.pitch + mean, events.pitch)


def refine_multi_pitch(activations, midi_freqs, t=0.5, peaks_only=True, n_valid_bins=0):
    """
    ``mpe_compact``'s per-frame lists of active bins with a refined pitch per entry, on the device: ``(est_off int64 [T + 1], est_bins
    int32 [n], delta float32 [n], pitch float64 [n])``, frame f's entries at ``est_off[f]:est_off[f + 1]``.  ``delta`` and ``pitch``
    as in ``note_contours``.  ``activations``: a CUDA tensor (F, T) or (1, F, T).
    """
    x = _mpe_activations(activations)
    F, T = x.shape
    midi_freqs = np.array(midi_freqs, dtype=np.float64)
    if midi_freqs.shape != (F,):
        raise ValueError('midi_freqs must hold one value per bin (%d), got shape %s' % (F, midi_freqs.shape))
    est_off, est_bins, _, _ = mpe_compact(x, t, peaks_only, n_valid_bins)
    dev = x.device
    n = int(est_off[-1])                                              # the one read: how many entries the lists hold
    est_bins = est_bins[:n]
    delta = torch.empty(n, dtype=torch.float32, device=dev)
    pitch = torch.empty(n, dtype=torch.float64, device=dev)
    if n:
        m_d = torch.from_numpy(midi_freqs).to(dev)
        with torch.cuda.device(dev):
            _hip.check(_hip.lib().tt_contours_frames(_hip.ptr(x), F, T, int(n_valid_bins), _hip.ptr(est_off), _hip.ptr(est_bins), n,
                                                     _hip.ptr(m_d), _hip.ptr(delta), _hip.ptr(pitch), _hip.stream_ptr()),
                       'tt_contours_frames')
    return est_off, est_bins, delta, pitch


def activations_to_multi_pitch_refined(activations, midi_freqs, peaks_only=False, t=0.5, n_valid_bins=0):
    """
    ``activations_to_multi_pitch`` with refined pitches: (F, T) activations on the device -> a host list of T float64 arrays with the
    active pitches in Hz, ascending bins, ``440 * 2 ** ((pitch - 69) / 12)`` of ``refine_multi_pitch``'s pitches.  Where every
    ``delta`` is 0 the result equals ``activations_to_multi_pitch``'s.
    """
    est_off, _, _, pitch = refine_multi_pitch(activations, midi_freqs, t, peaks_only, n_valid_bins)
    off, pitch = est_off.cpu().numpy(), pitch.cpu().numpy()
    hz = 440.0 * (2.0 ** ((pitch - 69.0) / 12.0))
    return [hz[off[i]:off[i + 1]] if off[i + 1] > off[i] else np.empty(0) for i in range(len(off) - 1)]


def _rescale(bend, num, den):
    """round(bend * num / den) on Python / int64 integers, halves away from zero."""
    mag = (2 * np.abs(bend) * num + den) // (2 * den)
    return np.where(bend < 0, -mag, mag)


def contours_to_bends(events, contours, item=0, bend_range=2):
    """
    The contours of one batch item on the host, in the form ``write_midi_bends`` takes: ``(frames, bends)``, two lists with one int64
    array per note of the item, in the order of ``events`` (that of ``events_to_notes``).  ``frames[i]``: the frame indices of the
    note's voiced frames (``bin >= 0``); ``bends[i]``: the bend there on the 14-bit scale of a MIDI pitch-bend message whose range
    (RPN 0) is ``bend_range`` semitones -- 8192 / ``bend_range`` per semitone -- as ``round(bend * 8192 / (bend_range * units))`` in
    integer arithmetic, halves rounded away from zero, not yet clamped.  The times of the frames are ``times[frames[i]]`` of the frame
    grid the map was computed on.
    """
    bend_range = int(bend_range)
    if bend_range < 1:
        raise ValueError('bend_range must be a positive number of semitones')
    sel = np.flatnonzero((events.item == int(item)).cpu().numpy())
    off, onset = contours.frame_off.cpu().numpy(), events.onset.cpu().numpy().astype(np.int64)
    bin_, bend = contours.bin.cpu().numpy(), contours.bend.cpu().numpy().astype(np.int64)
    frames, bends = [], []
    for i in sel:
        voiced = np.flatnonzero(bin_[off[i]:off[i + 1]] >= 0)
        frames.append(onset[i] + voiced)
        bends.append(_rescale(bend[off[i]:off[i + 1]][voiced], 8192, bend_range * int(contours.units)).astype(np.int64))
    return frames, bends


def write_midi_bends(file, pitches, intervals, bends, frame_times, velocities=None, bend_range=2, tempo_bpm=120, ticks_per_beat=480):
    """
    Notes with pitch bends -> a format-0 Standard MIDI File, byte by byte like ``write_midi`` (whose output is a different file: all
    notes on channel 0, no bends).  ``pitches``, ``intervals``, ``velocities``, ticks: as for ``write_midi``.  ``bends``: per note an
    array of bend values on the 14-bit scale (0 = no bend, 8192 / ``bend_range`` per semitone; ``contours_to_bends``), clamped to
    [-8192, 8191]; ``frame_times``: per note the times in seconds at which they apply, non-decreasing.

    A bend moves a whole channel, so every note gets a channel to itself for the whole of its interval: notes are taken in order of
    onset tick (then of position) and given the lowest of the channels 1 to 15 whose earlier notes have all ended by that tick.  A note
    that finds none goes to channel 0 without bends; the RETURN VALUE is the number of such notes.  At tick 0 every channel in use
    among 1 to 15 has its bend range (RPN 0) set to ``bend_range`` semitones: controllers 101 = 0, 100 = 0, 6 = ``bend_range``, 38 = 0.
    The bend of a note's channel is centred (0xE0 00 40) at the tick of its note-on, before it; after that a bend event is written only
    when the 14-bit value differs from that of the frame before (from the centre, for the first), and only at ticks before the
    note's end.  Events that share a tick are ordered: note-offs (by pitch) come before bends (by channel, then in time order), and
    bends before note-ons (by pitch).  The file is written to ``file`` (a path or a binary file object).
    """
    pitches = np.asarray(pitches, dtype=np.float64).ravel()
    intervals = np.asarray(intervals, dtype=np.float64).reshape(-1, 2)
    L = len(pitches)
    if len(intervals) != L or len(bends) != L or len(frame_times) != L:
        raise ValueError('pitches, intervals, bends and frame_times must hold one entry per note')
    if not 1 <= int(ticks_per_beat) <= 0x7FFF:
        raise ValueError('ticks_per_beat must lie in [1, 32767]')
    if not 1 <= int(bend_range) <= 127:
        raise ValueError('bend_range must lie in [1, 127] semitones')
    if not (np.all(np.isfinite(pitches)) and np.all(np.isfinite(intervals)) and np.all(intervals >= 0)):
        raise ValueError('pitches and times must be finite, times non-negative')
    note = np.clip(np.rint(pitches), 0, 127).astype(np.int64)
    strength = np.full(L, 0.5) if velocities is None else np.asarray(velocities, dtype=np.float64).ravel()
    if len(strength) != L:
        raise ValueError('velocities must hold one entry per note')
    vel = 1 + np.rint(126.0 * np.clip(np.nan_to_num(strength, nan=0.0), 0.0, 1.0)).astype(np.int64)
    scale = ticks_per_beat * tempo_bpm / 60.0
    ticks = np.rint(intervals * scale).astype(np.int64)
    busy_until = [0] * 16                                             # per channel: the latest end tick of the notes it was given
    events, seq, dropped = [], 0, 0                                   # (tick, kind: 0 off / 1 bend / 2 on, pitch, channel, seq, bytes)
    for i in sorted(range(L), key=lambda k: (int(ticks[k, 0]), k)):
        on, off, n = int(ticks[i, 0]), int(ticks[i, 1]), int(note[i])
        ch = next((c for c in range(1, 16) if busy_until[c] <= on), 0)
        if ch:
            busy_until[ch] = max(off, on)
            values = np.clip(np.asarray(bends[i], dtype=np.int64).ravel(), -8192, 8191)
            times = np.asarray(frame_times[i], dtype=np.float64).ravel()
            if len(values) != len(times) or not np.all(np.isfinite(times)) or np.any(np.diff(times) < 0):
                raise ValueError('note %d: bends and frame_times must be finite arrays of one length, times non-decreasing' % i)
            events.append((on, 1, 0, ch, seq, bytes([0xE0 | ch, 0x00, 0x40])))
            seq += 1
            last = 0
            for v, tk in zip(values.tolist(), np.rint(times * scale).astype(np.int64).tolist()):
                if v != last and tk < off:
                    events.append((max(tk, on), 1, 0, ch, seq, bytes([0xE0 | ch, (v + 8192) & 0x7F, (v + 8192) >> 7])))
                    seq += 1
                    last = v
        else:
            dropped += 1
        events.append((on, 2, n, ch, seq, bytes([0x90 | ch, n, int(vel[i])])))
        events.append((off, 0, n, ch, seq + 1, bytes([0x80 | ch, n, 0])))
        seq += 2
    events.sort(key=lambda e: e[:5])
    track = bytearray(b'\x00\xff\x51\x03' + struct.pack('>I', int(round(60e6 / tempo_bpm)))[1:])
    for ch in sorted({e[3] for e in events if e[3]}):
        for controller, value in ((101, 0), (100, 0), (6, int(bend_range)), (38, 0)):
            track += b'\x00' + bytes([0xB0 | ch, controller, value])
    now = 0
    for tick, _, _, _, _, message in events:
        track += _vlq(tick - now) + message
        now = tick
    track += b'\x00\xff\x2f\x00'
    data = b'MThd' + struct.pack('>IHHH', 6, 0, 1, int(ticks_per_beat)) + b'MTrk' + struct.pack('>I', len(track)) + bytes(track)
    if hasattr(file, 'write'):
        file.write(data)
    else:
        with open(file, 'wb') as f:
            f.write(data)
    return dropped
