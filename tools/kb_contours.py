"""
Pitch contours on the device (csrc/contours.hip) against the host route on one machine, on the synthetic five-minute track of
tools/kb_events.py: 540 bins (472 below 5 kHz), 102 400 frames at 341 frames / s, random sparse notes (a peak row with weaker neighbour
rows, a few dropped frames inside every note, a noise floor below the threshold everywhere else).

    python tools/kb_contours.py [--iters 7] [--host-iters 2] [--frames 102400] [--notes 3000] [--unequal]

On that track the two neighbour rows of a note hold the same value, so the parabola is symmetric and nearly every delta is 0
(``refined_share``); ``--unequal`` draws them apart, which changes no byte count and makes the equality check one of non-zero deltas.

One JSON line:
  device_ms      note_events + note_contours on the device tensor, warm, host clock between two device synchronisations (their small reads
                 included), median / min / max over --iters
  events_ms      note_events alone, the same way;  contours_ms: note_contours alone on notes that are already there
  finish_call_ms / contours_call_ms   tt_events_finish alone and tt_contours_notes alone through the C ABI on operands that are already
                 there, between two HIP events, median over --iters: the two kernels read the same bytes of the map under the notes
  download_ms    the (F, T) fp32 map to the host (what the host route pays before it can start)
  host_ref_ms    the NumPy route on the downloaded map: kb_events' vectorised predicate and run detection, then per note the passing bin of
                 the row with the largest value per frame and the refinement of tests/contours_ref.py in kind (fp32 operations rounded one
                 by one, float64 pitch and bend), vectorised over the note's frames
  host_ms        their sum
  equal          every array of the two routes compares equal (==; pitch with NaNs equal)
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'timbre-trap_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from kb_events import F, FV, THR, host_route, synthetic_track  # noqa: E402

UNITS = 4096
FRAME_FIELDS = ('bin', 'delta', 'value', 'pitch', 'bend')
NOTE_FIELDS = ('n_voiced', 'bend_sum', 'bend_min', 'bend_max')


def unequal_track(n_frames, n_notes, rng):
    """kb_events' track with the two neighbour rows of a note drawn apart (0.2 .. 0.5 of the level each, frame by frame).  On the
    original track they are equal wherever no other note touches them, so nearly every delta there is 0; on this one nearly none is."""
    x = (0.3 * rng.random((F, n_frames))).astype(np.float32)
    for _ in range(n_notes):
        f, t0 = int(rng.integers(2, FV - 2)), int(rng.integers(0, n_frames - 1))
        t1 = min(n_frames, t0 + int(rng.integers(10, 700)))
        level = (0.6 + 0.4 * rng.random(t1 - t0)).astype(np.float32)
        level[rng.random(t1 - t0) < 0.02] = 0.2
        x[f, t0:t1] = level
        for g in (f - 1, f + 1):
            x[g, t0:t1] = np.maximum(x[g, t0:t1], (0.2 + 0.3 * rng.random(t1 - t0)).astype(np.float32) * level)
    return x


def host_contours(a, group_off, m, row_pitch, ev):
    """The contour arrays from the downloaded map and the host's notes, vectorised over the frames of a note."""
    f32 = np.float32
    y = a.copy()
    y[FV:] = 0
    up, dn = np.zeros_like(y), np.zeros_like(y)
    up[1:], dn[:-1] = y[:-1], y[1:]
    passed = (y > up) & (y > dn) & (y.astype(np.float64) >= THR)
    above = np.concatenate([np.diff(m), [m[-1] - m[-2]]])            # the spacing delta >= 0 points to; the other side's at the last bin
    below = np.concatenate([[m[1] - m[0]], np.diff(m)])                 # ... and delta < 0; the other side's at bin 0
    _, rows, onsets, ends = ev[:4]
    frame_off = np.concatenate([[0], np.cumsum(ends.astype(np.int64) - onsets)])
    n = int(frame_off[-1])
    out = dict(frame_off=frame_off, bin=np.full(n, -1, np.int32), delta=np.zeros(n, f32), value=np.zeros(n, f32), pitch=np.full(n, np.nan),
               bend=np.zeros(n, np.int32), n_voiced=np.zeros(len(rows), np.int32), bend_sum=np.zeros(len(rows), np.int64),
               bend_min=np.zeros(len(rows), np.int32), bend_max=np.zeros(len(rows), np.int32))
    for i,(p, t0, t1) in enumerate(zip(rows.tolist(), onsets.tolist(), ends.tolist())):
        g0, g1 = group_off[p], group_off[p + 1]
        ok = passed[g0:g1, t0:t1]
        voiced = ok.any(0)
        if not voiced.any():
            continue
        val = np.where(ok, y[g0:g1, t0:t1], f32(-np.inf))
        f = g0 + val.argmax(0)[voiced]                                  # the first of equal maxima: the lowest bin
        t = t0 + np.flatnonzero(voiced)
        b_, a_, c_ = y[f, t], up[f, t], dn[f, t]
        fine = np.isfinite(a_) & np.isfinite(b_) & np.isfinite(c_) & (b_ >= a_) & (b_ >= c_)
        with np.errstate(all='ignore'):
            num, den = a_ - c_, (a_ - b_) + (c_ - b_)
            d = np.where(fine & (den < 0), f32(0.5) * (num / den), f32(0)).astype(f32)
        d = np.clip(np.where(np.isnan(d), f32(0), d), f32(-0.5), f32(0.5)).astype(f32)
        pitch = m[f] + d.astype(np.float64) * np.where(d >= 0, above[f], below[f])
        prod = (pitch - row_pitch[p]) * float(UNITS)
        bend = np.where(np.isfinite(prod), np.clip(np.rint(prod), -2.0 ** 30, 2.0 ** 30), 0.0).astype(np.int32)
        s = frame_off[i] + np.flatnonzero(voiced)
        out['bin'][s], out['delta'][s], out['value'][s], out['pitch'][s], out['bend'][s] = f, d, b_, pitch, bend
        out['n_voiced'][i], out['bend_sum'][i] = len(bend), bend.astype(np.int64).sum()
        out['bend_min'][i], out['bend_max'][i] = bend.min(), bend.max()
    return out


def timed(fn, iters):
    """Median / min / max of the host clock between two device synchronisations, milliseconds."""
    ms = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def between_events(fn, iters):
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=7)
    ap.add_argument('--host-iters', type=int, default=2)
    ap.add_argument('--frames', type=int, default=102400)
    ap.add_argument('--notes', type=int, default=3000)
    ap.add_argument('--max-gap', type=int, default=2)
    ap.add_argument('--min-frames', type=int, default=3)
    ap.add_argument('--unequal', action='store_true', help='draw the neighbour rows of a note apart, so that the deltas are not zero')
    args = ap.parse_args()
    from timbre_trap import _hip
    from timbre_trap.utils import note_contours, note_events
    from timbre_trap.utils.events import _pitch_rows
    dev = torch.device('cuda:0')
    midi_freqs = 16.76557586 + np.arange(F) / 5.0
    track = unequal_track if args.unequal else synthetic_track
    x = torch.from_numpy(track(args.frames, args.notes, np.random.default_rng(args.frames))).to(dev)
    group_off, row_pitch = _pitch_rows(midi_freqs, F, 'semitone', None)
    kw = dict(t=THR, n_valid_bins=FV)

    def events():
        return note_events(x, midi_freqs, max_gap=args.max_gap, min_frames=args.min_frames, **kw)

    def both():
        ev = events()
        return ev, note_contours(x, ev, midi_freqs, units_per_semitone=UNITS, **kw)

    ev, co = both()                                            # once untimed: lazy kernel loading, allocator growth
    both()
    device_ms, events_ms = timed(both, args.iters), timed(events, args.iters)
    contours_ms = timed(lambda: note_contours(x, ev, midi_freqs, units_per_semitone=UNITS, **kw), args.iters)

    # the two kernels that read the map under the notes, alone: operands in place, one C-ABI call each between two HIP events
    lib, st = _hip.lib(), _hip.stream_ptr()
    L, T, P = ev.item.numel(), args.frames, len(group_off) - 1
    off_d = torch.from_numpy(group_off).to(dev)
    m_d, rp_d = torch.from_numpy(midi_freqs).to(dev), torch.from_numpy(row_pitch).to(dev)
    mask = torch.empty(P * ((T + 63) // 64), dtype=torch.int64, device=dev)
    _hip.check(lib.tt_events_mask(_hip.ptr(x), 1, F, T, THR, 2, FV, _hip.ptr(off_d), P, _hip.ptr(mask), st), 'tt_events_mask')
    n_active, keep, peak = torch.empty_like(ev.item), torch.empty_like(ev.item), torch.empty_like(ev.peak)
    outs = [torch.empty_like(t) for t in co[1:-1]]

    def finish_call():
        _hip.check(lib.tt_events_finish(_hip.ptr(x), 1, F, T, THR, 2, FV, _hip.ptr(off_d), P, _hip.ptr(mask), _hip.ptr(ev.item), _hip.ptr(ev.row),
                                        _hip.ptr(ev.onset), _hip.ptr(ev.end), L, args.min_frames, _hip.ptr(n_active), _hip.ptr(peak),
                                        _hip.ptr(keep), st), 'tt_events_finish')

    def contours_call():
        _hip.check(lib.tt_contours_notes(_hip.ptr(x), 1, F, T, THR, 2, FV, _hip.ptr(off_d), P, _hip.ptr(m_d), _hip.ptr(rp_d), UNITS,
                                         _hip.ptr(ev.item), _hip.ptr(ev.row), _hip.ptr(ev.onset), _hip.ptr(ev.end), L, _hip.ptr(co.frame_off),
                                         *(_hip.ptr(t) for t in outs), st), 'tt_contours_notes')

    finish_call()
    contours_call()
    finish_ms, call_ms = between_events(finish_call, args.iters), between_events(contours_call, args.iters)
    calls_equal = torch.equal(n_active, ev.n_active) and all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(outs, co[1:-1]))

    down, ref, host_ev, host_co = [], [], None, None
    for _ in range(args.host_iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a = x.cpu().numpy()
        t1 = time.perf_counter()
        host_ev = host_route(a, group_off.tolist(), args.max_gap, args.min_frames)
        host_co = host_contours(a, group_off.tolist(), midi_freqs, row_pitch, host_ev)
        down.append((t1 - t0) * 1e3)
        ref.append((time.perf_counter() - t1) * 1e3)
    med = statistics.median
    equal = None
    if host_co is not None:
        equal = all(np.array_equal(getattr(ev, n).cpu().numpy(), h) for n, h in zip(ev._fields, host_ev))
        equal = equal and all(np.array_equal(getattr(co, n).cpu().numpy(), host_co[n], equal_nan=(n == 'pitch'))
                              for n in ('frame_off',) + FRAME_FIELDS + NOTE_FIELDS)
    host_ms = med(down) + med(ref) if down else None
    r3 = lambda v: tuple(round(u, 3) for u in v)                                          # noqa: E731
    print(json.dumps(dict(frames=args.frames, seconds=round(args.frames / 341.0, 1), bins=F, rows=P, notes_drawn=args.notes,
                          unequal_neighbours=bool(args.unequal), max_gap=args.max_gap, min_frames=args.min_frames, events=L, note_frames=int(co.frame_off[-1]),
                          voiced_frames=int(co.n_voiced.sum()), refined_share=round(float((co.delta[co.bin >= 0] != 0).float().mean()), 3),
                          map_mb=round(F * args.frames * 4 / 1e6, 1), device_ms=r3(device_ms), events_ms=r3(events_ms),
                          contours_ms=r3(contours_ms), finish_call_ms=r3(finish_ms), contours_call_ms=r3(call_ms),
                          contours_over_finish=round(call_ms[0] / finish_ms[0], 2), calls_equal=bool(calls_equal),
                          download_ms=round(med(down), 1) if down else None, host_ref_ms=round(med(ref), 1) if down else None,
                          host_ms=round(host_ms, 1) if down else None,
                          host_over_device=round(host_ms / device_ms[0], 1) if down else None, equal=equal)), flush=True)


if __name__ == '__main__':
    main()
