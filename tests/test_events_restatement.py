"""
CPU-only: the NumPy reference of the note-event contract (tests/events_ref.py) pinned on hand-written rows whose answers are spelled
out literally and against a brute-force second form (per frame, the distance to the previous and to the next active frame); the MIDI
writer against a literal byte string and a small reader; and the round-trip notes of tests/test_gpu_events.py run through the host
route (notes -> per-frame lists -> float64 target map -> peaks) plus the reference, which shows that the reference alone recovers
every one of them.  Everything is integers and exact fp32 values: every assertion is ``==``.

``random_map`` / ``crafted`` / ``round_trip_case`` / ``read_midi`` / ``host_pass`` are shared with tests/test_gpu_events.py.
"""

import functools
import io
import struct

import numpy as np
import pytest

from oracle import postprocessing as opp
from oracle import targets as otg
from timbre_trap.utils.events import _pitch_rows, write_midi
from timbre_trap.utils.notes import _host_spans, notes_to_multi_pitch
from timbre_trap.utils.targets import midi_to_hz

from events_ref import note_events_ref, row_notes, runs
from test_mpe_restatement import MIDI_FREQS

INF, NAN = np.float32(np.inf), np.float32(np.nan)
F37, B37, FV37 = 37, 3, 33
GROUPS37 = np.array([2, 5, 5, 9, 16, 17, 30, 36], dtype=np.int32)       # P = 7: bins 0, 1, 36 in no row, row 1 empty, FV37 cuts row 6
RANDOM_T = (1, 63, 64, 65, 127, 128, 129, 300)
DENSITIES = (0.02, 0.3, 0.9)
GAP_MIN = ((0, 1), (1, 1), (5, 3), (63, 1), (63, 64))
THR = 0.5


# ---- shared inputs ------------------------------------------------------------------------------------------------------------------

def host_pass(x, thr=THR, mode=2, fv=0):
    """The predicate on the host for the CPU tests (oracle/postprocessing.py on the masked float64 map): (B, F, T) bool."""
    y = np.array(x, dtype=np.float64)
    if 0 < fv < y.shape[-2]:
        y[..., fv:, :] = 0.0
    return opp.threshold(opp.filter_non_peaks(y) if mode == 2 else y, thr) > 0


@functools.lru_cache(maxsize=None)
def random_map(density, n_frames, seed=0):
    """fp32 (B37, F37, n_frames): a floor below the threshold, values in [0.5, 1) at a fraction ``density`` of the positions, which are
    drawn per (item, bin) in runs along time so that notes of many lengths and gaps of many lengths occur."""
    rng = np.random.default_rng([seed, n_frames, int(density * 1000)])
    shape = (B37, F37, n_frames)
    x = 0.45 * rng.random(shape)
    high = rng.random(shape) < density
    stretch = rng.random(shape) < 0.6                                   # a position copies its left neighbour's state: runs
    for t in range(1, n_frames):
        high[..., t] = np.where(stretch[..., t], high[..., t - 1], high[..., t])
    x[high] = 0.5 + 0.5 * rng.random(int(high.sum()))
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def _rows(T, *spans_per_row, value=0.9):
    """(1, R, T) fp32 for 'bin' rows under mode 1: row r is ``value`` on the given (start, end exclusive) spans, 0 elsewhere."""
    x = np.zeros((1, len(spans_per_row), T), dtype=np.float32)
    for r, spans in enumerate(spans_per_row):
        for s, e in spans:
            x[0, r, s:e] = value
    return x


def _identity(F):
    return np.arange(F + 1, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def crafted():
    """name -> dict(x, group_off, mode, fv, gap, minf, want): ``want`` lists (item, row, onset, end, n_active) literally."""
    c = {}
    # a note spanning three words
    c['three_words'] = dict(x=_rows(200, [(10, 180)]), want=[(0, 0, 10, 180, 170)])
    # a gap of five zeros straddling the boundary between word 0 and word 1
    x = _rows(130, [(50, 62), (67, 80)])
    c['straddle_gap_equals_max'] = dict(x=x, gap=5, want=[(0, 0, 50, 80, 25)])
    c['straddle_gap_exceeds_max'] = dict(x=x, gap=4, want=[(0, 0, 50, 62, 12), (0, 0, 67, 80, 13)])
    # one at bit 0 of word 1, then a gap that starts at bit 1: 63 zeros are bridged by max_gap = 63, 64 are not
    c['gap_63'] = dict(x=_rows(200, [(64, 65), (128, 129)]), gap=63, want=[(0, 0, 64, 129, 2)])
    c['gap_64'] = dict(x=_rows(200, [(64, 65), (129, 130)]), gap=63, want=[(0, 0, 64, 65, 1), (0, 0, 129, 130, 1)])
    c['all_ones'] = dict(x=_rows(130, [(0, 130)]), gap=7, want=[(0, 0, 0, 130, 130)])
    # 1010...1 over 129 frames: ceil(129 / 2) = 65 notes, the most a row can hold at max_gap = 0
    c['alternating'] = dict(x=_rows(129, [(t, t + 1) for t in range(0, 129, 2)]), want=[(0, 0, t, t + 1, 1) for t in range(0, 129, 2)])
    # leading and trailing zeros are never filled; the notes touch neither end
    c['ends_not_filled'] = dict(x=_rows(70, [(3, 5), (60, 66)]), gap=10, want=[(0, 0, 3, 5, 2), (0, 0, 60, 66, 6)])
    c['touching_both_ends'] = dict(x=_rows(65, [(0, 2), (64, 65)]), want=[(0, 0, 0, 2, 2), (0, 0, 64, 65, 1)])
    # min_frames removes a merged note: 2 + 3 zeros + 2 = 7 frames < 8, the second note has 8
    c['min_frames_drops_merged'] = dict(x=_rows(40, [(1, 3), (6, 8), (20, 28)]), gap=3, minf=8, want=[(0, 0, 20, 28, 8)])
    # the last row of item 0 ends in a one and the first row of item 1 starts with one -- also row to row within an item; T a whole
    # number of words, so the two bits are neighbours in memory
    for T in (64, 70):
        x = np.zeros((2, 2, T), dtype=np.float32)
        x[0, 0, T - 2:] = 0.9
        x[0, 1, 0] = x[0, 1, T - 1] = 0.8
        x[1, 0, 0:3] = 0.7
        x[1, 1, 5] = 0.6
        # row 1 of item 0 holds T - 2 zeros between its two ones: bridged at T = 64 (62 <= 63), not at T = 70
        mid = [(0, 1, 0, T, 2)] if T == 64 else [(0, 1, 0, 1, 1), (0, 1, T - 1, T, 1)]
        c['neighbouring_rows_T%d' % T] = dict(x=x, gap=63, want=[(0, 0, T - 2, T, 2)] + mid + [(1, 0, 0, 3, 3), (1, 1, 5, 6, 1)],
                                              peaks=[np.float32(v) for v in ((0.9, 0.8, 0.7, 0.6) if T == 64 else (0.9, 0.8, 0.8, 0.7, 0.6))])
    # f_valid = 4 cuts through the group [2, 6): bins 4 and 5 read as zero however large; mode 2 makes bin 3 a peak over its masked
    # neighbour
    x = np.zeros((1, 8, 6), dtype=np.float32)
    x[0, 4, 0], x[0, 5, 1] = 0.9, 0.95                                  # masked rows alone: inactive frames
    x[0, 3, 2], x[0, 4, 2] = 0.6, 0.99                                  # bin 3 is valid, its larger upper neighbour is masked
    x[0, 2, 4], x[0, 3, 4] = 0.7, 0.8
    groups = np.array([0, 2, 6, 8], dtype=np.int32)
    c['f_valid_cuts_group_threshold'] = dict(x=x, group_off=groups, fv=4, mode=1, want=[(0, 1, 2, 3, 1), (0, 1, 4, 5, 1)])
    c['f_valid_cuts_group_peaks'] = dict(x=x, group_off=groups, fv=4, mode=2, want=[(0, 1, 2, 3, 1), (0, 1, 4, 5, 1)])
    # a plateau holds no strict peak; next to it a proper peak
    x = np.zeros((1, 6, 4), dtype=np.float32)
    x[0, 1:4, 0] = 0.8
    x[0, 1, 2], x[0, 2, 2], x[0, 3, 2] = 0.6, 0.9, 0.6
    c['plateau'] = dict(x=x, group_off=np.array([0, 6], dtype=np.int32), mode=2, want=[(0, 0, 2, 3, 1)])
    # NaN never passes and shields its neighbours in peak mode; +inf passes and is reported as the peak
    x = np.zeros((1, 4, 8), dtype=np.float32)
    x[0, 1, 0] = NAN
    x[0, 1, 2], x[0, 2, 2] = 0.9, NAN
    x[0, 1, 4], x[0, 1, 5] = INF, 0.7
    c['nan_inf_threshold'] = dict(x=x, group_off=np.array([0, 4], dtype=np.int32), mode=1, want=[(0, 0, 2, 3, 1), (0, 0, 4, 6, 2)],
                                  peaks=[np.float32(0.9), INF])
    c['nan_inf_peaks'] = dict(x=x, group_off=np.array([0, 4], dtype=np.int32), mode=2, want=[(0, 0, 4, 6, 2)], peaks=[INF])
    for name, d in c.items():
        d.setdefault('group_off', _identity(d['x'].shape[1]))
        for k, v in dict(mode=1, fv=0, gap=0, minf=1).items():
            d.setdefault(k, v)
        d['x'].setflags(write=False)
    return c


def as_rows(ev):
    """The five integer arrays as a list of tuples."""
    return [tuple(int(v) for v in r) for r in zip(*ev[:5])]


@functools.lru_cache(maxsize=None)
def round_trip_case(n_notes=40, n_frames=300, seed=0):
    """About forty notes on integer MIDI pitches over a 300-frame grid: same-pitch notes at least two frames apart, notes that sound
    together at least two semitones apart.  -> dict(pitches Hz, intervals s, times, midi (int), lo, hi)."""
    rng = np.random.default_rng([seed, 4040])
    times = np.arange(n_frames) * (1.0 / 341.0)
    notes = []
    while len(notes) < n_notes:
        m, lo = int(rng.integers(30, 100)), int(rng.integers(0, n_frames - 1))
        hi = min(n_frames, lo + int(rng.integers(1, 40)))
        if all(abs(m - m2) >= 2 or lo >= hi2 + 2 or lo2 >= hi + 2 for m2, lo2, hi2 in notes):
            notes.append((m, lo, hi))
    midi = np.array([n[0] for n in notes])
    lo, hi = np.array([n[1] for n in notes]), np.array([n[2] for n in notes])
    hop = times[1]
    intervals = np.stack([(lo - 0.3) * hop, (hi - 0.4) * hop], axis=1)
    got_lo, got_hi = _host_spans(intervals, times)
    assert np.array_equal(got_lo, lo) and np.array_equal(got_hi, hi)
    return dict(pitches=midi_to_hz(midi.astype(np.float64)), intervals=intervals, times=times, midi=midi, lo=lo, hi=hi)


def round_trip_want(case):
    """(row, onset, end) per note in (row, onset) order, rows counted from the lowest semitone of MIDI_FREQS."""
    first = int(np.floor(MIDI_FREQS[0] + 0.5))
    return sorted((int(m) - first, int(a), int(b)) for m, a, b in zip(case['midi'], case['lo'], case['hi']))


def read_midi(data):
    """A format-0 Standard MIDI File -> (ticks_per_beat, microseconds per beat, [(tick, 'on' / 'off', pitch, velocity), ...])."""
    assert data[:4] == b'MThd' and struct.unpack('>IHHH', data[4:14])[:3] == (6, 0, 1)
    tpb = struct.unpack('>H', data[12:14])[0]
    assert data[14:18] == b'MTrk'
    n = struct.unpack('>I', data[18:22])[0]
    body, pos, tick, tempo, events, ended = data[22:22 + n], 0, 0, None, [], False
    assert len(data) == 22 + n
    while pos < len(body):
        assert not ended
        delta = 0
        while True:
            byte = body[pos]
            pos += 1
            delta = (delta << 7) | (byte & 0x7F)
            if not byte & 0x80:
                break
        tick += delta
        status = body[pos]
        if status == 0xFF:
            kind, length = body[pos + 1], body[pos + 2]
            payload = body[pos + 3:pos + 3 + length]
            pos += 3 + length
            if kind == 0x51:
                tempo = int.from_bytes(payload, 'big')
            ended = kind == 0x2F
        else:
            assert status in (0x90, 0x80)
            events.append((tick, 'on' if status == 0x90 else 'off', body[pos + 1], body[pos + 2]))
            pos += 3
    assert ended
    return tpb, tempo, events


# ---- the reference on hand-written rows -----------------------------------------------------------------------------------------------

def test_runs_and_row_notes_literally():
    row = [0, 1, 1, 0, 0, 1, 0, 0, 0, 1, 1, 1, 0]
    assert runs(row) == [(1, 3), (5, 6), (9, 12)]
    assert row_notes(row) == [(1, 3), (5, 6), (9, 12)]
    assert row_notes(row, max_gap=1) == [(1, 3), (5, 6), (9, 12)]                 # gaps of 2 and 3
    assert row_notes(row, max_gap=2) == [(1, 6), (9, 12)]                         # a gap of exactly max_gap is filled
    assert row_notes(row, max_gap=3) == [(1, 12)]
    assert row_notes(row, max_gap=3, min_frames=11) == [(1, 12)] and row_notes(row, max_gap=3, min_frames=12) == []
    assert row_notes(row, max_gap=2, min_frames=4) == [(1, 6)]
    assert row_notes(row, min_frames=2) == [(1, 3), (9, 12)]
    assert row_notes([0, 0, 0], max_gap=63) == [] and row_notes([1], max_gap=63) == [(0, 1)] and row_notes([]) == []
    assert row_notes([1, 0, 1]) == [(0, 1), (2, 3)] and row_notes([1, 0, 1], max_gap=1) == [(0, 3)]
    assert row_notes([0, 0, 1, 0, 0], max_gap=63) == [(2, 3)]                     # leading / trailing zeros stay


@pytest.mark.parametrize('name', sorted(crafted()))
def test_reference_on_crafted_rows(name):
    c = crafted()[name]
    ev = note_events_ref(host_pass(c['x'], THR, c['mode'], c['fv']), c['x'], c['group_off'], c['gap'], c['minf'])
    assert as_rows(ev) == c['want']
    assert all(a.dtype == np.int32 for a in ev[:5]) and ev[5].dtype == np.float32
    if 'peaks' in c:
        assert list(ev[5]) == c['peaks']


def test_reference_empty_group_and_outside_bins():
    x = random_map(0.3, 65)
    ev = note_events_ref(host_pass(x, THR, 1), x, GROUPS37)
    assert len(ev[0]) > 50 and 1 not in set(ev[1].tolist()) and set(ev[1].tolist()) == {0, 2, 3, 4, 5, 6}
    only_outside = np.zeros((1, F37, 10), dtype=np.float32)
    only_outside[0, [0, 1, 36], :] = 0.9                                          # bins of no row
    assert len(note_events_ref(host_pass(only_outside, THR, 1), only_outside, GROUPS37)[0]) == 0
    # peak: the largest PASSING value -- under mode 2 a larger non-peak value of the row does not count
    y = np.zeros((1, 4, 1), dtype=np.float32)
    y[0, :, 0] = (0.6, 0.2, 0.8, 0.9)
    ev = note_events_ref(host_pass(y, THR, 2), y, np.array([0, 3, 4], dtype=np.int32))
    assert as_rows(ev) == [(0, 0, 0, 1, 1), (0, 1, 0, 1, 1)] and list(ev[5]) == [np.float32(0.6), np.float32(0.9)]


def brute_force(a, max_gap, min_frames):
    """Second form: frame t opens a note iff it is active and the previous active frame lies more than max_gap + 1 back (or there is
    none); it closes one iff the next active frame lies more than max_gap + 1 ahead.  Openings and closings pair up in order."""
    T = len(a)
    back, ahead = np.full(T, T + 64), np.full(T, T + 64)
    last = None
    for t in range(T):
        if last is not None:
            back[t] = t - last
        if a[t]:
            last = t
    nxt = None
    for t in range(T - 1, -1, -1):
        if nxt is not None:
            ahead[t] = nxt - t
        if a[t]:
            nxt = t
    ons = [t for t in range(T) if a[t] and back[t] > max_gap + 1]
    ends = [t + 1 for t in range(T) if a[t] and ahead[t] > max_gap + 1]
    assert len(ons) == len(ends)
    return [(s, e) for s, e in zip(ons, ends) if e - s >= min_frames]


@pytest.mark.parametrize('gap,minf', GAP_MIN + ((2, 2), (62, 5)))
def test_reference_is_the_brute_force_form(gap, minf):
    n = 0
    for density in DENSITIES:
        for T in (1, 2, 65, 300):
            x = random_map(density, T, seed=1)
            a = (x >= THR).any(axis=1)                                            # (B, T): all bins as one row
            for row in a:
                assert row_notes(row, gap, minf) == brute_force(row, gap, minf)
                n += len(row_notes(row, gap, minf))
    assert n > 0 or minf > 60


def test_groupings_of_the_default_geometry():
    off, pitch = _pitch_rows(MIDI_FREQS, 540, 'semitone', None)
    semi = np.floor(MIDI_FREQS + 0.5)
    assert off[0] == 0 and off[-1] == 540 and np.all(np.diff(off) >= 0) and len(off) == len(pitch) + 1
    assert pitch[0] == semi[0] and pitch[-1] == semi[-1] and np.array_equal(np.diff(pitch), np.ones(len(pitch) - 1))
    for p in range(len(pitch)):
        assert np.all(semi[off[p]:off[p + 1]] == pitch[p])
    assert np.all(np.diff(off)[1:-1] == 5) and 1 <= np.diff(off)[0] <= 5 and 1 <= np.diff(off)[-1] <= 5       # five bins per semitone
    off, pitch = _pitch_rows(MIDI_FREQS, 540, 'bin', None)
    assert np.array_equal(off, np.arange(541)) and np.array_equal(pitch, MIDI_FREQS)
    off, pitch = _pitch_rows(np.arange(37.0), 37, 'semitone', GROUPS37)
    assert np.array_equal(off, GROUPS37) and pitch[0] == 3.0 and np.isnan(pitch[1]) and pitch[-1] == 32.5
    for bad in ([3, 2], [-1, 4], [0, 38], [0.5, 2.0]):
        with pytest.raises(ValueError):
            _pitch_rows(np.arange(37.0), 37, 'semitone', np.array(bad))
    with pytest.raises(ValueError):
        _pitch_rows(MIDI_FREQS, 540, 'octave', None)
    with pytest.raises(ValueError):
        _pitch_rows(MIDI_FREQS[:5], 540, 'bin', None)


# ---- the MIDI writer ------------------------------------------------------------------------------------------------------------------

def test_write_midi_two_notes_literally():
    # 120 bpm, 480 ticks per beat: 960 ticks per second.  C4 from 0 to 0.5 s at strength 1, E4 from 0.25 s to 0.5 s at strength 0.5
    data = write_midi(io.BytesIO(), [60, 64.4], [[0.0, 0.5], [0.25, 0.5]], velocities=[1.0, 0.5])
    want = (b'MThd\x00\x00\x00\x06\x00\x00\x00\x01\x01\xe0'
            b'MTrk\x00\x00\x00\x1d'
            b'\x00\xff\x51\x03\x07\xa1\x20'                   # 500 000 us per beat
            b'\x00\x90\x3c\x7f'                               # tick 0: C4 on, velocity 127
            b'\x81\x70\x90\x40\x40'                           # + 240: E4 on, velocity 64
            b'\x81\x70\x80\x3c\x00'                           # + 240 = 480: offs before ons, then by pitch: C4 off
            b'\x00\x80\x40\x00'                               # E4 off
            b'\x00\xff\x2f\x00')
    assert data == want
    assert read_midi(data) == (480, 500000, [(0, 'on', 60, 127), (240, 'on', 64, 64), (480, 'off', 60, 0), (480, 'off', 64, 0)])
    buf = io.BytesIO()
    assert write_midi(buf, [60, 64.4], [[0.0, 0.5], [0.25, 0.5]], velocities=[1.0, 0.5]) == buf.getvalue() == want
    # a note-off and a note-on of the same pitch on one tick: the off comes first
    _, _, ev = read_midi(write_midi(io.BytesIO(), [60, 60], [[0.0, 1.0], [1.0, 2.0]]))
    assert ev == [(0, 'on', 60, 64), (960, 'off', 60, 0), (960, 'on', 60, 64), (1920, 'off', 60, 0)]
    assert read_midi(write_midi(io.BytesIO(), [], np.empty((0, 2)))) == (480, 500000, [])
    assert read_midi(write_midi(io.BytesIO(), [200, -3], [[0, 1], [0, 1]], velocities=[7.0, -1.0]))[2][:2] == [(0, 'on', 0, 1), (0, 'on', 127, 127)]
    with pytest.raises(ValueError):
        write_midi(io.BytesIO(), [60], [[0.0, 1.0], [1.0, 2.0]])
    with pytest.raises(ValueError):
        write_midi(io.BytesIO(), [60], [[0.0, np.nan]])


def test_write_midi_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    tpb, bpm = 384, 97
    pitches = rng.integers(0, 128, size=50)
    on = rng.integers(0, 3_000_000, size=50)                                      # ticks needing up to four delta bytes
    off = on + rng.integers(1, 50_000, size=50)
    strength = rng.random(50)
    seconds = np.stack([on, off], axis=1) * 60.0 / (tpb * bpm)
    path = tmp_path / 'notes.mid'
    write_midi(str(path), pitches + rng.uniform(-0.49, 0.49, size=50), seconds, strength, tempo_bpm=bpm, ticks_per_beat=tpb)
    got_tpb, tempo, events = read_midi(path.read_bytes())
    assert got_tpb == tpb and tempo == round(60e6 / bpm)
    vel = 1 + np.rint(126 * strength).astype(int)
    want = [(int(t), 'on', int(p), int(v)) for t, p, v in zip(on, pitches, vel)] + [(int(t), 'off', int(p), 0) for t, p in zip(off, pitches)]
    want.sort(key=lambda e: (e[0], e[1] == 'on', e[2]))
    assert events == want and len(events) == 100
    assert [e[0] for e in events] == sorted(e[0] for e in events)


# ---- the round trip of the GPU test, on the host ---------------------------------------------------------------------------------------

def test_reference_recovers_the_round_trip_notes():
    case = round_trip_case()
    assert len(case['midi']) == 40
    lists = notes_to_multi_pitch(case['pitches'], case['intervals'], case['times'])
    target = otg.multi_pitch_to_activations(lists, MIDI_FREQS).astype(np.float32)[None]         # what note_events is handed: fp32
    off, pitch = _pitch_rows(MIDI_FREQS, 540, 'semitone', None)
    ev = note_events_ref(host_pass(target, 0.5, 2), target, off)
    assert [(int(r), int(a), int(b)) for r, a, b in zip(ev[1], ev[2], ev[3])] == round_trip_want(case)
    assert np.array_equal(pitch[ev[1]], np.sort(case['midi']).astype(np.float64))                # ascending rows: ascending pitches
    assert np.array_equal(ev[4], ev[3] - ev[2]) and np.all(ev[5] == np.float32(1.0))            # no frame missing, every peak the clipped 1
