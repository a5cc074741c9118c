"""
NumPy reference of the pitch-contour contract (include/ttrap.h: tt_contours_*; timbre_trap.utils.note_contours / refine_multi_pitch):
plain loops over notes, frames and bins, ``np.float32`` scalars for ``delta`` -- every operation rounded on its own -- and float64 for the
rest.  tests/test_contours_restatement.py pins it on literal answers; tests/test_gpu_contours.py holds the device route to it with ``==``.

The predicate is NOT restated here: the caller hands over the boolean pass mask (B, F, T) (on the GPU: the downloaded output of
``_device_pick``), the map ``x`` (B, F, T) fp32, the offset table ``group_off`` (P + 1: row p owns the bins ``[group_off[p],
group_off[p + 1])``), ``m`` (F float64, the MIDI number of every bin) and ``row_pitch`` (P float64).

The semantics, once more:

refine(f, t).  b = x[f], a = x[f - 1], c = x[f + 1] at frame t; a neighbour beyond either end or at f >= f_valid reads as 0.  If a, b, c
are all finite, b >= a and b >= c, in fp32 with every operation rounded on its own: num = a - c; den = (a - b) + (c - b);
delta = 0.5 * (num / den) if den < 0 else 0 (a NaN quotient -- inf / inf -- gives 0); delta is clamped to [-0.5, 0.5].  Otherwise delta
= 0.  In float64: pitch = m[f] + delta * step with step = m[f + 1] - m[f] for delta >= 0 and m[f] - m[f - 1] otherwise; where that
neighbour does not exist, the other side's spacing; 0 at F = 1.

Per frame t in [onset, end) of a note: among the bins of the note's row that pass, the one with the largest x (ties: the lowest bin;
+inf allowed) gives bin, value = x[bin], delta, pitch and bend = rint((pitch - row_pitch[row]) * units) (float64, ties to even),
clamped to [-2^30, 2^30], 0 for a non-finite product.  No passing bin: bin = -1, delta = 0, value = 0, pitch = NaN, bend = 0.
Per note over the frames with bin >= 0: n_voiced, bend_sum (int64), bend_min, bend_max (0 and 0 where n_voiced is 0).
"""

import numpy as np

FRAME_FIELDS = ('bin', 'delta', 'value', 'pitch', 'bend')
NOTE_FIELDS = ('n_voiced', 'bend_sum', 'bend_min', 'bend_max')
F32 = np.float32


def delta_of(a, b, c):
    """The fp32 offset of the triple (below, at, above the bin)."""
    a, b, c = F32(a), F32(b), F32(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c) and b >= a and b >= c):
        return F32(0)
    with np.errstate(all='ignore'):
        num = F32(a - c)
        den = F32(F32(a - b) + F32(c - b))
        d = F32(0)
        if den < 0:
            d = F32(F32(0.5) * F32(num / den))
    if np.isnan(d):
        d = F32(0)
    if d < F32(-0.5):
        d = F32(-0.5)
    if d > F32(0.5):
        d = F32(0.5)
    return d


def pitch_of(m, f, delta):
    """m[f] + delta * step in float64."""
    F = len(m)
    step = np.float64(0)
    if F > 1:
        if delta >= 0:
            step = m[f + 1] - m[f] if f + 1 < F else m[f] - m[f - 1]
        else:
            step = m[f] - m[f - 1] if f > 0 else m[f + 1] - m[f]
    with np.errstate(all='ignore'):
        return np.float64(m[f]) + np.float64(np.float64(delta) * np.float64(step))


def refine(col, f, fv, m):
    """(delta fp32, pitch float64) at bin f of one frame (col: the F values of the frame)."""
    F = len(col)
    rd = lambda g: col[g] if 0 <= g < fv else F32(0)                                      # noqa: E731
    d = delta_of(rd(f - 1), col[f], rd(f + 1))
    return d, pitch_of(m, f, d)


def bend_of(pitch, row_pitch, units):
    with np.errstate(all='ignore'):
        prod = np.float64(np.float64(pitch) - np.float64(row_pitch)) * np.float64(units)
    if not np.isfinite(prod):
        return 0
    return int(min(max(np.rint(prod), -2.0 ** 30), 2.0 ** 30))


def _fv(F, f_valid):
    return f_valid if 0 < f_valid < F else F


def note_contours_ref(passed, x, group_off, m, row_pitch, units, item, row, onset, end, f_valid=0):
    """-> dict: frame_off int64 [L + 1]; bin int32, delta fp32, value fp32, pitch float64, bend int32 per frame slot; n_voiced int32,
    bend_sum int64, bend_min int32, bend_max int32 per note."""
    x = np.asarray(x, dtype=np.float32)
    passed = np.asarray(passed, dtype=bool)
    m = np.asarray(m, dtype=np.float64)
    F = x.shape[1]
    fv = _fv(F, f_valid)
    L = len(item)
    frame_off = np.zeros(L + 1, dtype=np.int64)
    frame_off[1:] = np.cumsum(np.asarray(end, dtype=np.int64) - np.asarray(onset, dtype=np.int64))
    n = int(frame_off[-1])
    out = dict(frame_off=frame_off, bin=np.full(n, -1, dtype=np.int32), delta=np.zeros(n, dtype=np.float32),
               value=np.zeros(n, dtype=np.float32), pitch=np.full(n, np.nan), bend=np.zeros(n, dtype=np.int32),
               n_voiced=np.zeros(L, dtype=np.int32), bend_sum=np.zeros(L, dtype=np.int64), bend_min=np.zeros(L, dtype=np.int32),
               bend_max=np.zeros(L, dtype=np.int32))
    for i in range(L):
        b, p = int(item[i]), int(row[i])
        g0, g1 = int(group_off[p]), int(group_off[p + 1])
        bends = []
        for k, t in enumerate(range(int(onset[i]), int(end[i]))):
            best = -1
            for f in range(g0, g1):
                if passed[b, f, t] and (best < 0 or x[b, f, t] > x[b, best, t]):
                    best = f
            if best < 0:
                continue
            s = frame_off[i] + k
            d, pt = refine(x[b, :, t], best, fv, m)
            out['bin'][s], out['delta'][s], out['value'][s], out['pitch'][s] = best, d, x[b, best, t], pt
            out['bend'][s] = bend_of(pt, row_pitch[p], units)
            bends.append(int(out['bend'][s]))
        if bends:
            out['n_voiced'][i], out['bend_sum'][i], out['bend_min'][i], out['bend_max'][i] = len(bends), sum(bends), min(bends), max(bends)
    return out


def refine_frames_ref(x, est_off, est_bins, m, f_valid=0):
    """(delta fp32 [n], pitch float64 [n]) of the per-frame bin lists (est_off [T + 1], est_bins [n]) on the map x (F, T)."""
    x = np.asarray(x, dtype=np.float32)
    m = np.asarray(m, dtype=np.float64)
    fv = _fv(x.shape[0], f_valid)
    n = int(est_off[-1])
    delta, pitch = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float64)
    for t in range(x.shape[1]):
        for j in range(int(est_off[t]), int(est_off[t + 1])):
            delta[j], pitch[j] = refine(x[:, t], int(est_bins[j]), fv, m)
    return delta, pitch
