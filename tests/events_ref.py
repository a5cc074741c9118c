"""
NumPy reference of the note-event contract (include/ttrap.h: tt_events_*; timbre_trap.utils.note_events), derived differently from the
kernels: no bit words and no prefix sums -- runs by ``np.diff`` on zero-padded rows, gaps filled and short notes dropped by explicit
loops over the runs.  tests/test_events_restatement.py pins it on hand-written rows and against a second, brute-force form;
tests/test_gpu_events.py holds the device route to it with ``==``.

The predicate is NOT restated here: the caller hands over the boolean pass mask (B, F, T) (on the GPU: the downloaded output of
``_device_pick``), the map ``x`` (B, F, T) fp32 and the offset table ``group_off`` (P + 1, ascending: row p owns the bins
``[group_off[p], group_off[p + 1])``).
"""

import numpy as np

FIELDS = ('item', 'row', 'onset', 'end', 'n_active', 'peak')


def row_activity(passed, x, group_off):
    """a (B, P, T) bool: OR of ``passed`` over the row's bins; v (B, P, T) fp32: max of x over the row's PASSING bins (-inf where none)."""
    passed = np.asarray(passed, dtype=bool)
    x = np.asarray(x, dtype=np.float32)
    B, F, T = passed.shape
    P = len(group_off) - 1
    a = np.zeros((B, P, T), dtype=bool)
    v = np.full((B, P, T), -np.inf, dtype=np.float32)
    for p in range(P):
        g0, g1 = int(group_off[p]), int(group_off[p + 1])
        if g1 > g0:
            a[:, p] = passed[:, g0:g1].any(axis=1)
            v[:, p] = np.where(passed[:, g0:g1], x[:, g0:g1], np.float32(-np.inf)).max(axis=1)
    return a, v


def runs(row):
    """Maximal runs of ones of a 0/1 row as (start, end exclusive) pairs, from the +1 / -1 steps of the zero-padded row."""
    d = np.diff(np.concatenate([[0], np.asarray(row, dtype=np.int8), [0]]))
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def row_notes(row, max_gap=0, min_frames=1):
    """The kept notes of one row as (t0, end exclusive) pairs: neighbouring runs are merged while the zeros between them number at most
    ``max_gap`` (zeros before the first and after the last run have a one on one side only and are never filled), then notes shorter
    than ``min_frames`` are dropped."""
    merged = []
    for s, e in runs(row):
        if merged and s - merged[-1][1] <= max_gap:
            merged[-1][1] = e
        else:
            merged.append([s, e])
    return [(s, e) for s, e in merged if e - s >= min_frames]


def note_events_ref(passed, x, group_off, max_gap=0, min_frames=1):
    """The six arrays of the contract, in ascending (item, row, onset) order: item, row, onset, end, n_active (int32), peak (float32)."""
    a, v = row_activity(passed, x, group_off)
    out = []
    for b in range(a.shape[0]):
        for p in range(a.shape[1]):
            for s, e in row_notes(a[b, p], max_gap, min_frames):
                on = a[b, p, s:e]
                out.append((b, p, s, e, int(on.sum()), v[b, p, s:e][on].max()))
    cols = list(zip(*out)) if out else [()] * 6
    return tuple(np.array(c, dtype=np.float32 if k == 5 else np.int32) for k, c in enumerate(cols))
