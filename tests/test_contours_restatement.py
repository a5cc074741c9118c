"""
CPU-only: the NumPy reference of the pitch-contour contract (tests/contours_ref.py) pinned on triples whose answers are spelled out
literally, on a parabola with dyadic coefficients (the vertex comes back exactly) and on a synthetic vibrato ridge (the refined pitch
is held against the true centre); the condition that keeps the GPU comparison from passing on zeros -- at least 90 % of the voiced
frames of every generated case have ``delta != 0`` -- checked for every such case; the MIDI writer with pitch bends against a literal
byte string and a small reader; the host helpers ``refined_pitches`` and ``contours_to_bends``.

``M5`` / ``literal_columns`` / ``smooth_map`` / ``random_cases`` / ``crafted`` / ``ridge`` / ``detuned_notes`` / ``reference_run`` /
``read_midi_bends`` are shared with tests/test_gpu_contours.py; what they return is cached and read-only.
"""

import functools
import io
import struct

import numpy as np
import pytest
import torch

from timbre_trap.utils.contours import NoteContours, contours_to_bends, refined_pitches, write_midi_bends
from timbre_trap.utils.events import NoteEvents, _pitch_rows, write_midi

import contours_ref as C
from events_ref import note_events_ref
from test_events_restatement import host_pass

F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)
THR = 0.5
UNITS = 4096
RANDOM_T = (1, 63, 64, 65, 130, 300)
SIGMA = 2 * 2.5 / 5                                                     # bins: the blur of multi_pitch_to_activations at its default decay
M5 = np.array([60.0, 60.25, 60.375, 60.875, 61.875])                   # five bins, every spacing different and dyadic
M5.setflags(write=False)


def frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


# ---- shared inputs ------------------------------------------------------------------------------------------------------------------

def literal_columns():
    """name -> (column of five fp32 values, bin, f_valid, delta wanted, pitch wanted) with M5 as the bins' MIDI numbers."""
    tenth = F32(0.5) * (F32(-0.25) / F32(-1.25))
    third = F32(0.5) * (F32(-0.5) / F32(-1.5))
    fifth = F32(0.5) * (F32(0.5) / F32(-2.5))
    cut = F32(0.5) * (F32(0.25) / (F32(F32(0.25) - F32(1)) + F32(-1)))
    c = {
        'issue_triple': ([0, 0.25, 1, 0.5, 0], 2, 0, tenth, 60.375 + float(tenth) * 0.5),
        'symmetric': ([0, 0.5, 1, 0.5, 0], 2, 0, F32(0), 60.375),
        'plateau': ([0, 0.75, 0.75, 0.75, 0], 2, 0, F32(0), 60.375),
        'larger_neighbour': ([0, 0.875, 0.625, 0.125, 0], 2, 0, F32(0), 60.375),
        'nan_neighbour': ([0, NAN, 0.875, 0.125, 0], 2, 0, F32(0), 60.375),
        'infinite_bin': ([0, 0.125, INF, 0.25, 0], 2, 0, F32(0), 60.375),
        'first_bin_up': ([1, 0.5, 0, 0, 0], 0, 0, third, 60.0 + float(third) * 0.25),
        'first_bin_down': ([1, -0.5, 0, 0, 0], 0, 0, fifth, 60.0 + float(fifth) * 0.25),      # no bin below: the spacing above
        'last_bin_down': ([0, 0, 0, 0.5, 1], 4, 0, -third, 61.875 + float(-third) * 1.0),
        'last_bin_up': ([0, 0, 0, -0.5, 1], 4, 0, -fifth, 61.875 + float(-fifth) * 1.0),        # no bin above: the spacing below
        'neighbour_at_f_valid': ([0, 0.25, 1, 0.96875, 0.96875], 2, 3, cut, 60.375 + float(cut) * 0.125),
    }
    return {k: (frozen(np.array(v[0], dtype=np.float32)),) + v[1:] for k, v in c.items()}


@functools.lru_cache(maxsize=None)
def smooth_map(B, F, T, seed=0):
    """fp32 (B, F, T), smooth along F: sparse spikes of height 0.9 .. 1.2, drawn in runs along time, on a floor of at most 0.05, blurred
    over three bins with (0.2, 0.6, 0.2).  A spike becomes a peak of 0.54 .. 0.77 between unequal neighbours below the threshold."""
    rng = np.random.default_rng([seed, B, F, T])
    shape = (B, F, T)
    high = rng.random(shape) < 0.06
    stretch = rng.random(shape) < 0.7
    for t in range(1, T):
        high[..., t] = np.where(stretch[..., t], high[..., t - 1], high[..., t])
    high[0, 3, 0] = True                                                # a note even at T = 1
    s = 0.05 * rng.random(shape) + np.where(high, 0.9 + 0.3 * rng.random(shape), 0.0)
    pad = np.zeros((B, 1, T))
    up, dn = np.concatenate([pad, s[:, :-1]], 1), np.concatenate([s[:, 1:], pad], 1)
    return frozen((0.2 * up + 0.6 * s + 0.2 * dn).astype(np.float32))


def _uneven(F, seed=3):
    """F ascending MIDI numbers with unequal dyadic spacings."""
    rng = np.random.default_rng(seed)
    return frozen(40.0 + np.concatenate([[0.0], np.cumsum(rng.integers(1, 8, size=F - 1) / 32.0)]))


GROUPS12 = frozen(np.array([0, 5, 12], dtype=np.int32))                 # F = 12 in groups of 5 and 7; f_valid = 9 cuts the second


def random_cases():
    """The random cases of the GPU test as dicts(x, group_off, fv, m); modes and max_gap are applied by the caller."""
    for T in RANDOM_T:
        yield 'groups_T%d' % T, dict(x=smooth_map(2, 12, T), group_off=GROUPS12, fv=9, m=_uneven(12))
        yield 'bins_T%d' % T, dict(x=smooth_map(2, 17, T), group_off=frozen(np.arange(18, dtype=np.int32)), fv=14, m=_uneven(17))


@functools.lru_cache(maxsize=None)
def crafted():
    """name -> dict(x, group_off, mode, fv, gap, m)."""
    c = {}
    rng = np.random.default_rng(77)

    def bump(x, b, f, t0, t1):
        n = t1 - t0
        x[b, f, t0:t1] = 0.6 + 0.4 * rng.random(n)
        x[b, f - 1, t0:t1], x[b, f + 1, t0:t1] = 0.3 * rng.random(n), 0.3 * rng.random(n)

    x = np.zeros((1, 6, 210), dtype=np.float32)
    bump(x, 0, 2, 5, 205)
    c['four_chunks'] = dict(x=x, group_off=np.array([0, 6], dtype=np.int32))
    x = np.zeros((1, 6, 130), dtype=np.float32)
    bump(x, 0, 3, 63, 65)
    c['frames_63_to_65'] = dict(x=x, group_off=np.array([0, 6], dtype=np.int32))
    x = np.zeros((1, 6, 70), dtype=np.float32)
    bump(x, 0, 1, 10, 40)
    bump(x, 0, 4, 20, 60)
    c['neighbouring_rows_share_frames'] = dict(x=x, group_off=np.array([0, 3, 6], dtype=np.int32))
    x = np.zeros((2, 6, 70), dtype=np.float32)
    bump(x, 1, 4, 63, 70)
    c['last_item_ends_at_T'] = dict(x=x, group_off=np.array([1, 3, 6], dtype=np.int32))
    cols = literal_columns()
    plain = [k for k in cols if cols[k][2] == 0]
    x = np.stack([cols[k][0] for k in plain], axis=1)[None]              # (1, 5, n): one literal column per frame
    c['literals_threshold'] = dict(x=x, group_off=np.array([0, 5], dtype=np.int32), m=M5)
    c['literals_peaks_bridged'] = dict(x=x, group_off=np.array([0, 5], dtype=np.int32), mode=2, gap=2, m=M5)
    x = np.stack([cols['neighbour_at_f_valid'][0], cols['issue_triple'][0]], axis=1)[None]
    c['literals_f_valid'] = dict(x=x, group_off=np.array([0, 5], dtype=np.int32), fv=3, m=M5)
    x = np.zeros((1, 5, 4), dtype=np.float32)
    x[0, :, 1] = x[0, :, 2] = (0, 0.875, 0.125, 0.875, 0)               # two equal peaks: the lower bin
    c['tie_lower_bin'] = dict(x=x, group_off=np.array([0, 5], dtype=np.int32), mode=2, m=M5)
    for d in c.values():
        for k, v in dict(mode=1, fv=0, gap=0).items():
            d.setdefault(k, v)
        d.setdefault('m', _uneven(d['x'].shape[1]))
        d['x'].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def ridge(n_frames=130, F=100, centre=50.0, depth=0.4, rate_hz=6.0, frames_per_second=341.0):
    """A Gaussian ridge along F (sigma = SIGMA bins, the blur of multi_pitch_to_activations) whose centre moves as a vibrato of
    +-``depth`` semitones at ``rate_hz``: -> (x fp32 (1, F, T), m float64 (F), true centre in MIDI numbers (T))."""
    m = 40.0 + np.arange(F) / 5.0
    true = centre + depth * np.sin(2 * np.pi * rate_hz * np.arange(n_frames) / frames_per_second)
    x = np.exp(-0.5 * ((np.arange(F)[:, None] - (true[None, :] - 40.0) * 5.0) / SIGMA) ** 2)
    return frozen(x.astype(np.float32)[None]), frozen(m), frozen(true)


@functools.lru_cache(maxsize=None)
def detuned_notes(F=540, T=40):
    """Twelve notes with constant detunings of -30 .. +30 cents, painted as Gaussian ridges: -> (x fp32 (F, T), m (F), semitones,
    detunings in semitones)."""
    m = 16.76557586 + np.arange(F) / 5.0
    semis = 30 + 5 * np.arange(12)
    cents = np.linspace(-30, 30, 12)
    x = np.zeros((F, T))
    for k, (s, c) in enumerate(zip(semis, cents)):
        ridge_ = np.exp(-0.5 * ((np.arange(F) - (s + c / 100.0 - m[0]) * 5.0) / SIGMA) ** 2)
        x[:, 2 + k:2 + k + 20] = np.maximum(x[:, 2 + k:2 + k + 20], ridge_[:, None])
    return frozen(x.astype(np.float32)), frozen(m), semis, cents / 100.0


def reference_run(x, group_off, mode, fv, gap, m, row_pitch=None, passed=None, units=UNITS, minf=1):
    """Events by tests/events_ref.py, then their contours: -> (the six event arrays, the contour dict)."""
    passed = host_pass(x, THR, mode, fv) if passed is None else passed
    ev = note_events_ref(passed, x, group_off, gap, minf)
    if row_pitch is None:
        row_pitch = _pitch_rows(m, x.shape[1], 'semitone', group_off)[1]
    return ev, C.note_contours_ref(passed, x, group_off, m, row_pitch, units, ev[0], ev[1], ev[2], ev[3], fv)


def refined_fraction(out):
    """Share of the voiced frames with a non-zero delta."""
    voiced = out['bin'] >= 0
    return float((out['delta'][voiced] != 0).mean()) if voiced.any() else 0.0


def ridge_error_cents(pitch, true):
    return float(np.abs(pitch - true).max() * 100.0)


def read_midi_bends(data):
    """A format-0 file -> (ticks_per_beat, tempo, [(tick, kind, channel, a, b)]) with kind 'on' / 'off' (a: pitch, b: velocity), 'cc'
    (a: controller, b: value) and 'bend' (a: the signed 14-bit value, b: 0)."""
    assert data[:4] == b'MThd' and struct.unpack('>IHHH', data[4:14])[:3] == (6, 0, 1) and data[14:18] == b'MTrk'
    tpb, n = struct.unpack('>H', data[12:14])[0], struct.unpack('>I', data[18:22])[0]
    body, pos, tick, tempo, events, ended = data[22:22 + n], 0, 0, None, [], False
    assert len(data) == 22 + n
    kinds = {0x90: 'on', 0x80: 'off', 0xB0: 'cc', 0xE0: 'bend'}
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
            if kind == 0x51:
                tempo = int.from_bytes(body[pos + 3:pos + 3 + length], 'big')
            ended = kind == 0x2F
            pos += 3 + length
            continue
        kind, a, b = kinds[status & 0xF0], body[pos + 1], body[pos + 2]
        assert a < 128 and b < 128
        events.append((tick, kind, status & 0x0F) + ((((b << 7) | a) - 8192, 0) if kind == 'bend' else (a, b)))
        pos += 3
    assert ended
    return tpb, tempo, events


# ---- refine, literally --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(literal_columns()))
def test_refine_on_literal_columns(name):
    col, f, fv, want_delta, want_pitch = literal_columns()[name]
    d, p = C.refine(col, f, fv if fv else 5, M5)
    assert d.dtype == np.float32 and d == want_delta and p == want_pitch, (d, p)
    if name in ('symmetric', 'plateau', 'larger_neighbour', 'nan_neighbour', 'infinite_bin'):
        assert d == 0 and p == M5[f]
    else:
        assert d != 0 and abs(d) < 0.5


def test_delta_literals():
    assert C.delta_of(0.25, 1, 0.5) == F32(0.5) * (F32(-0.25) / F32(-1.25)) == F32(0.1)
    assert C.delta_of(0.5, 1, 0.25) == -C.delta_of(0.25, 1, 0.5)
    assert C.delta_of(0.5, 1, 0.5) == 0 and C.delta_of(0.75, 0.75, 0.75) == 0 and C.delta_of(0.875, 0.625, 0.125) == 0
    assert C.delta_of(NAN, 0.875, 0.125) == 0 and C.delta_of(0.125, 0.875, NAN) == 0 and C.delta_of(0.125, NAN, 0.25) == 0
    assert C.delta_of(0.125, INF, 0.25) == 0 and C.delta_of(-INF, 1, 0.25) == 0
    assert C.delta_of(1, 1, 0) == F32(0.5) * (F32(1) / F32(-1)) == F32(-0.5)                  # a two-bin plateau: half way between them
    assert C.delta_of(0, 1, 1) == F32(0.5)
    big = F32(3e38)
    assert C.delta_of(-big, big, -big) == 0 and C.delta_of(big, big, -big) == 0               # a - c overflows: inf / inf gives 0
    # F = 1: no spacing at all
    assert C.pitch_of(np.array([61.5]), 0, F32(0.25)) == 61.5


def test_parabola_with_dyadic_coefficients_returns_its_vertex():
    for vertex in (0.25, -0.25, 0.375, -0.4375, 0.0, 0.5, -0.5):
        a, b, c = (1.0 - 0.25 * (u - vertex) ** 2 for u in (-1.0, 0.0, 1.0))
        assert all(float(F32(v)) == v for v in (a, b, c))                                      # exact in fp32
        assert float(C.delta_of(a, b, c)) == vertex
    col = np.array([0, 0.609375, 0.984375, 0.859375, 0], dtype=np.float32)                     # vertex + 0.25 at bin 2
    assert C.refine(col, 2, 5, M5) == (F32(0.25), 60.375 + 0.25 * 0.5)


def test_bend_literals():
    assert C.bend_of(60.25, 60.0, 2) == 0 and C.bend_of(60.75, 60.0, 2) == 2                   # 0.5 -> 0, 1.5 -> 2: ties to even
    assert C.bend_of(59.75, 60.0, 2) == 0 and C.bend_of(58.75, 60.0, 2) == -2
    assert C.bend_of(60.1, 60.0, 4096) == int(np.rint((60.1 - 60.0) * 4096.0)) == 410
    assert C.bend_of(np.nan, 60.0, 4096) == 0 and C.bend_of(60.0, np.nan, 4096) == 0 and C.bend_of(np.inf, 60.0, 1) == 0
    assert C.bend_of(1e9, 0.0, 4096) == 2 ** 30 and C.bend_of(-1e9, 0.0, 4096) == -2 ** 30


# ---- notes --------------------------------------------------------------------------------------------------------------------------

def test_tie_goes_to_the_lower_bin_and_a_bridged_frame_is_unvoiced():
    c = crafted()['tie_lower_bin']
    ev, out = reference_run(c['x'], c['group_off'], c['mode'], c['fv'], c['gap'], c['m'], row_pitch=np.array([60.0]))
    assert [tuple(int(v) for v in r) for r in zip(*ev[:5])] == [(0, 0, 1, 3, 2)]
    assert out['bin'].tolist() == [1, 1] and out['value'].tolist() == [F32(0.875)] * 2
    d = C.delta_of(0, 0.875, 0.125)
    assert d > 0 and out['delta'].tolist() == [d, d] and out['pitch'].tolist() == [60.25 + float(d) * 0.125] * 2
    # the literal columns under peak picking, gaps of up to two frames bridged: the plateau frame holds no strict peak
    c = crafted()['literals_peaks_bridged']
    ev, out = reference_run(c['x'], c['group_off'], c['mode'], c['fv'], c['gap'], c['m'], row_pitch=np.array([60.5]))
    names = [k for k, v in literal_columns().items() if v[2] == 0]
    assert len(ev[0]) == 1 and ev[3][0] - ev[2][0] == len(names) and ev[4][0] == len(names) - 2
    for k in (names.index('plateau'), names.index('nan_neighbour')):    # ... and a NaN shields the bin next to it
        assert out['bin'][k] == -1 and out['delta'][k] == 0 and out['value'][k] == 0 and np.isnan(out['pitch'][k]) and out['bend'][k] == 0
    assert out['n_voiced'][0] == len(names) - 2 and np.isnan(out['pitch']).sum() == 2
    voiced = out['bin'] >= 0
    assert out['bend_sum'][0] == out['bend'][voiced].astype(np.int64).sum()
    assert out['bend_min'][0] == out['bend'][voiced].min() and out['bend_max'][0] == out['bend'][voiced].max()
    # every literal column, met inside a note, gives its literal answer
    c = crafted()['literals_threshold']
    _, out = reference_run(c['x'], c['group_off'], c['mode'], c['fv'], c['gap'], c['m'], row_pitch=np.array([60.5]))
    for k, name in enumerate(names):
        _, f, _, want_delta, want_pitch = literal_columns()[name]
        if name in ('plateau', 'larger_neighbour'):                      # under the threshold alone a lower bin passes too and wins
            assert out['bin'][k] == 1
            continue
        assert (out['bin'][k], out['delta'][k], out['pitch'][k]) == (f, want_delta, want_pitch), name
        assert out['bend'][k] == int(np.rint((want_pitch - 60.5) * UNITS))
    c = crafted()['literals_f_valid']
    _, out = reference_run(c['x'], c['group_off'], c['mode'], c['fv'], c['gap'], c['m'], row_pitch=np.array([60.5]))
    assert out['delta'][0] == literal_columns()['neighbour_at_f_valid'][3] and out['delta'][1] == C.delta_of(0.25, 1, 0)


def test_vibrato_ridge_is_followed_below_the_half_bin_error():
    """Measured: the largest error of the refined pitch against the true centre of the ridge, against the 10 cents (half a bin) the
    unrefined bin centre can be off by."""
    x, m, true = ridge()
    off, row_pitch = _pitch_rows(m, len(m), 'semitone', None)
    ev, out = reference_run(x, off, 2, 0, 0, m, row_pitch=row_pitch)
    assert len(ev[0]) == 1 and (ev[2][0], ev[3][0]) == (0, 130) and row_pitch[ev[1][0]] == 50.0
    assert np.all(out['bin'] >= 0) and out['n_voiced'][0] == 130
    refined, unrefined = ridge_error_cents(out['pitch'], true), ridge_error_cents(m[out['bin']], true)
    print('vibrato ridge: largest error %.3f cents refined, %.3f cents at the bin centre' % (refined, unrefined))
    assert refined < 10.0
    assert 5.0 < unrefined <= 10.0 + 1e-9                               # the bar is a real one on this map
    assert refined_fraction(out) >= 0.9
    # the bends are the contour on the integer scale: within half a unit of it
    assert np.abs(out['bend'] - (out['pitch'] - 50.0) * UNITS).max() <= 0.5
    assert out['bend_min'][0] < -0.35 * UNITS and out['bend_max'][0] > 0.35 * UNITS


def test_generated_gpu_cases_are_refined_in_nine_frames_of_ten():
    for name, c in random_cases():
        for mode in (1, 2):
            for gap in (0, 2):
                ev, out = reference_run(c['x'], c['group_off'], mode, c['fv'], gap, c['m'])
                assert len(ev[0]) > 0 and refined_fraction(out) >= 0.9, (name, mode, gap, refined_fraction(out))
                assert np.array_equal(out['n_voiced'], ev[4])
    for name in ('four_chunks', 'frames_63_to_65', 'neighbouring_rows_share_frames', 'last_item_ends_at_T'):
        c = crafted()[name]
        ev, out = reference_run(c['x'], c['group_off'], c['mode'], c['fv'], c['gap'], c['m'])
        assert len(ev[0]) > 0 and refined_fraction(out) >= 0.9, name
    x, m, semis, detune = detuned_notes()
    off, row_pitch = _pitch_rows(m, 540, 'semitone', None)
    ev, out = reference_run(x[None], off, 2, 472, 0, m, row_pitch=row_pitch)
    assert refined_fraction(out) >= 0.9 and np.array_equal(row_pitch[ev[1]], semis.astype(np.float64))
    mean = out['bend_sum'] / (out['n_voiced'] * float(UNITS))
    print('detuned notes: largest error of the mean bend %.3f cents' % (np.abs(mean - detune).max() * 100))
    assert np.abs(mean - detune).max() * 100 < DETUNE_BAR_CENTS


# what the reference recovers a constant detuning to on the Gaussian ridge (largest error of the parabola's vertex on a Gaussian of
# sigma = 1 bin: 0.048 bins = 0.96 cents, near a quarter bin off centre -- the figure the vibrato test prints, 0.953), rounded up;
# the GPU round trip is held to the same bar
DETUNE_BAR_CENTS = 1.0


def test_frames_reference_on_a_hand_list():
    cols = literal_columns()
    x = np.stack([cols['issue_triple'][0], cols['first_bin_down'][0]], axis=1)
    delta, pitch = C.refine_frames_ref(x, np.array([0, 1, 3]), np.array([2, 0, 1]), M5)
    assert delta.tolist() == [cols['issue_triple'][3], cols['first_bin_down'][3], 0.0]
    assert pitch.tolist() == [cols['issue_triple'][4], cols['first_bin_down'][4], 60.25]


# ---- the host helpers ------------------------------------------------------------------------------------------------------------------

def _tuples(item, onset, end, pitch, bins, bends, units=UNITS):
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)                                        # noqa: E731
    n = [len(b) for b in bins]
    ev = NoteEvents(i32(item), i32([0] * len(item)), i32(onset), i32(end), i32(n), torch.ones(len(item)), torch.tensor(pitch, dtype=torch.float64))
    flat_bin, flat_bend = sum(bins, []), sum(bends, [])
    voiced = [[b for b, f in zip(bd, bn) if f >= 0] for bd, bn in zip(bends, bins)]
    co = NoteContours(torch.tensor(np.concatenate([[0], np.cumsum(n)]), dtype=torch.int64), i32(flat_bin), torch.zeros(len(flat_bin)),
                      torch.zeros(len(flat_bin)), torch.zeros(len(flat_bin), dtype=torch.float64), i32(flat_bend),
                      i32([len(v) for v in voiced]), torch.tensor([sum(v) for v in voiced], dtype=torch.int64),
                      i32([min(v, default=0) for v in voiced]), i32([max(v, default=0) for v in voiced]), units)
    return ev, co


def test_refined_pitches_and_bends_for_the_writer():
    ev, co = _tuples([0, 0, 1, 0], [5, 9, 0, 20], [8, 11, 2, 21], [60.0, 64.0, 50.0, 70.0],
                     [[3, 3, 3], [7, -1], [1, 1], [-1]], [[100, -300, 200], [2048, 0], [-4096, -4096], [0]])
    got = refined_pitches(ev, co)
    assert got.dtype == torch.float64
    # bends that sum to zero: the semitone itself; one voiced frame; a whole semitone down; no voiced frame: the row's pitch
    assert got.tolist() == [60.0, 64.0 + 2048 / (1 * 4096.0), 49.0, 70.0]
    frames, bends = contours_to_bends(ev, co, item=0, bend_range=2)
    assert [f.tolist() for f in frames] == [[5, 6, 7], [9], []] and [b.tolist() for b in bends] == [[100, -300, 200], [2048], []]
    frames, bends = contours_to_bends(ev, co, item=1, bend_range=2)
    assert [f.tolist() for f in frames] == [[0, 1]] and [b.tolist() for b in bends] == [[-4096, -4096]]
    # other ranges: round(bend * 8192 / (range * units)), halves away from zero
    ev, co = _tuples([0], [0], [8], [60.0], [[1] * 8], [[3, -3, 1, -1, 2, 4096, -4096, 0]])
    assert contours_to_bends(ev, co, bend_range=3)[1][0].tolist() == [2, -2, 1, -1, 1, 2731, -2731, 0]
    assert contours_to_bends(ev, co, bend_range=4)[1][0].tolist() == [2, -2, 1, -1, 1, 2048, -2048, 0]
    assert contours_to_bends(ev, co, bend_range=1)[1][0].tolist() == [6, -6, 2, -2, 4, 8192, -8192, 0]
    with pytest.raises(ValueError):
        contours_to_bends(ev, co, bend_range=0)


# ---- the MIDI writer with bends -----------------------------------------------------------------------------------------------------

TWO_NOTES = dict(pitches=[60, 64.4], intervals=[[0.0, 0.5], [0.25, 0.5]], velocities=[1.0, 0.5])


def test_write_midi_bends_two_overlapping_notes_literally():
    # 960 ticks per second.  C4 from 0 to 0.5 s on channel 1: bends 0, 100, 100, -50 at 0, 0.125, 0.25, 0.375 s; E4 from 0.25 s on
    # channel 2: one bend beyond the range, clamped to 8191
    buf = io.BytesIO()
    dropped = write_midi_bends(buf, bends=[[0, 100, 100, -50], [9000]], frame_times=[[0.0, 0.125, 0.25, 0.375], [0.25]], **TWO_NOTES)
    rpn = lambda ch: b''.join(b'\x00' + bytes([0xB0 | ch, c, v]) for c, v in ((101, 0), (100, 0), (6, 2), (38, 0)))      # noqa: E731
    want = (b'MThd\x00\x00\x00\x06\x00\x00\x00\x01\x01\xe0'
            b'MTrk\x00\x00\x00\x4f'
            b'\x00\xff\x51\x03\x07\xa1\x20' + rpn(1) + rpn(2) +
            b'\x00\xe1\x00\x40'                               # tick 0: channel 1 centred ...
            b'\x00\x91\x3c\x7f'                               # ... before C4 on; the bend 0 of its first frame changes nothing
            b'\x78\xe1\x64\x40'                               # + 120: 8192 + 100 = 0x40 << 7 | 0x64
            b'\x78\xe2\x00\x40'                               # + 120 = 240: channel 2 centred (the repeated 100 on channel 1: nothing),
            b'\x00\xe2\x7f\x7f'                               # its first frame's 8191,
            b'\x00\x92\x40\x40'                               # then E4 on
            b'\x78\xe1\x4e\x3f'                               # + 120 = 360: 8192 - 50 = 0x3f << 7 | 0x4e
            b'\x78\x81\x3c\x00'                               # + 120 = 480: offs by pitch
            b'\x00\x82\x40\x00'
            b'\x00\xff\x2f\x00')
    assert dropped == 0 and buf.getvalue() == want
    tpb, tempo, ev = read_midi_bends(want)
    assert (tpb, tempo) == (480, 500000)
    assert [e for e in ev if e[1] != 'cc'] == [(0, 'bend', 1, 0, 0), (0, 'on', 1, 60, 127), (120, 'bend', 1, 100, 0), (240, 'bend', 2, 0, 0),
                                               (240, 'bend', 2, 8191, 0), (240, 'on', 2, 64, 64), (360, 'bend', 1, -50, 0),
                                               (480, 'off', 1, 60, 0), (480, 'off', 2, 64, 0)]
    # write_midi keeps its bytes for the same notes
    assert write_midi(io.BytesIO(), **TWO_NOTES) == (
        b'MThd\x00\x00\x00\x06\x00\x00\x00\x01\x01\xe0MTrk\x00\x00\x00\x1d\x00\xff\x51\x03\x07\xa1\x20\x00\x90\x3c\x7f\x81\x70\x90\x40\x40'
        b'\x81\x70\x80\x3c\x00\x00\x80\x40\x00\x00\xff\x2f\x00')


def test_write_midi_bends_round_trip_and_channels(tmp_path):
    rng = np.random.default_rng(9)
    L, tpb, bpm = 30, 384, 97
    scale = tpb * bpm / 60.0
    on = np.sort(rng.integers(0, 20000, size=L))
    off = on + rng.integers(50, 3000, size=L)
    pitches = rng.integers(30, 100, size=L)
    frame_ticks = [np.arange(a, b, 16) for a, b in zip(on, off)]
    bends = [rng.integers(-9000, 9000, size=len(f)) // 3 * 3 for f in frame_ticks]
    path = tmp_path / 'bends.mid'
    dropped = write_midi_bends(str(path), pitches, np.stack([on, off], 1) / scale, bends, [f / scale for f in frame_ticks],
                               bend_range=12, tempo_bpm=bpm, ticks_per_beat=tpb)
    got_tpb, tempo, ev = read_midi_bends(path.read_bytes())
    assert got_tpb == tpb and tempo == round(60e6 / bpm) and [e[0] for e in ev] == sorted(e[0] for e in ev)
    ons = sorted((e for e in ev if e[1] == 'on'), key=lambda e: (e[0], e[3]))
    assert len(ons) == L and sum(e[2] == 0 for e in ons) == dropped
    # replay: the bend in force on a note's channel at each of its frames is the clamped bend handed in; one note per channel at a time
    state, sounding, trace = {}, {}, {}
    for tick, kind, ch, a, b in ev:
        if kind == 'cc':
            assert tick == 0 and ch >= 1
            state.setdefault(('rpn', ch), []).append((a, b))
        elif kind == 'bend':
            state[ch] = a
            trace.setdefault(ch, []).append((tick, a))
        elif kind == 'on':
            assert ch == 0 or (ch not in sounding and state.get(ch) is not None)
            if ch:
                sounding[ch] = (tick, a)
        elif ch:
            assert sounding.pop(ch)[1] == a
    used = {e[2] for e in ons if e[2]}
    assert all(state[('rpn', ch)] == [(101, 0), (100, 0), (6, 12), (38, 0)] for ch in used) and not sounding
    by_start = {}
    for e in ons:
        by_start.setdefault((e[0], e[3]), []).append(e[2])
    for i in range(L):
        ch = by_start[(int(on[i]), int(pitches[i]))].pop(0)
        if ch == 0:
            continue
        events = [(tk, v) for tk, v in trace[ch] if on[i] <= tk < off[i]]
        assert events[0] == (int(on[i]), 0)                             # centred at the note-on's tick
        want, last = [], 0
        for tk, v in zip(frame_ticks[i].tolist(), np.clip(bends[i], -8192, 8191).tolist()):
            if v != last:
                want.append((tk, v))
                last = v
        assert events[1:] == want, i


def test_sixteen_simultaneous_notes_leave_one_without_a_channel():
    buf = io.BytesIO()
    n = 16
    dropped = write_midi_bends(buf, 40 + np.arange(n), [[0.0, 1.0]] * n, [[50 * k] for k in range(n)], [[0.5]] * n)
    assert dropped == 1
    ev = read_midi_bends(buf.getvalue())[2]
    ons = [e for e in ev if e[1] == 'on']
    assert sorted(e[2] for e in ons) == list(range(16)) and [e[3] for e in ons if e[2] == 0] == [55]          # the last one taken
    assert not [e for e in ev if e[1] in ('bend', 'cc') and e[2] == 0]
    assert write_midi_bends(io.BytesIO(), [], np.empty((0, 2)), [], []) == 0
    # a channel is free again at the tick its note ends
    assert write_midi_bends(io.BytesIO(), [60] * 17, [[k, k + 1.0] for k in range(17)], [[]] * 17, [[]] * 17) == 0
    for bad in (dict(bends=[[1]], frame_times=[[0.1, 0.2]]), dict(bends=[[1, 2]], frame_times=[[0.2, 0.1]]), dict(bends=[], frame_times=[])):
        with pytest.raises(ValueError):
            write_midi_bends(io.BytesIO(), [60], [[0.0, 1.0]], **bad)
    with pytest.raises(ValueError):
        write_midi_bends(io.BytesIO(), [60], [[0.0, 1.0]], [[]], [[]], bend_range=0)
