"""
Note-level scoring on the device (csrc/notescore.hip) against the two host routes on one machine, on a synthetic five-minute track:
6000 reference notes with uniform onsets and integer pitches; the estimate drops 20 % of them, moves the onsets of the rest by about
30 ms, detunes them slightly and adds 30 % notes of its own.

    python tools/kb_notescore.py [--iters 9] [--host-iters 3] [--notes 6000] [--seconds 300]

One JSON line:
  device_ms       note_counts_device(est, ref) with both note lists already on the device (four tensors each), warm, host clock between
                  two device synchronisations -- the per-round flag reads and the one copy back included; median / min / max over --iters
  device_up_ms    the same with the reference given as host arrays (uploaded inside the call)
  windowed_ms     note_counts on host arrays: candidates by searchsorted inside the onset window, Kuhn's search on adjacency lists
  dense_ms        the usual host route: dense n_ref x n_est hit matrices from np.subtract.outer, then the same search on their non-zeros
  download_ms     the four estimate tensors to the host (what either host route pays first when the notes were formed on the device)
  equal           the four integers of the three routes compare equal (==)
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'timbre-trap_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def synthetic_track(n_ref, seconds, rng, jitter=0.03, extra=0.3, missing=0.2):
    on = np.sort(rng.uniform(0.0, seconds, n_ref))
    ref_p = rng.integers(36, 96, n_ref).astype(np.float64)
    ref_iv = np.stack([on, on + rng.uniform(0.05, 1.0, n_ref)], axis=1)
    keep = rng.random(n_ref) >= missing
    m, n_extra = int(keep.sum()), int(round(extra * n_ref))
    x_on = rng.uniform(0.0, seconds, n_extra)
    est_p = np.concatenate([ref_p[keep] + rng.normal(0.0, 0.25, m), rng.integers(36, 96, n_extra).astype(np.float64)])
    est_on = np.concatenate([on[keep] + rng.normal(0.0, jitter, m), x_on])
    est_off = np.concatenate([ref_iv[keep, 1] + rng.normal(0.0, 0.06, m), x_on + rng.uniform(0.05, 1.0, n_extra)])
    order = rng.permutation(len(est_p))
    return ref_p, ref_iv, est_p[order].copy(), np.stack([est_on, est_off], axis=1)[order].copy()


def dense_route(ref_p, ref_iv, est_p, est_iv, kuhn):
    """(n_ref, n_est, tp, tp_no_offset) through dense hit matrices."""
    onset = np.around(np.abs(np.subtract.outer(ref_iv[:, 0], est_iv[:, 0])), 4) <= 0.05
    pitch = np.abs(np.subtract.outer(ref_p, est_p)) <= 0.5
    tol = np.maximum(0.2 * (ref_iv[:, 1] - ref_iv[:, 0]), 0.05)
    offset = np.around(np.abs(np.subtract.outer(ref_iv[:, 1], est_iv[:, 1])), 4) <= tol[:, None]
    hit = onset & pitch
    out = []
    for h in (hit & offset, hit):
        i, k = np.nonzero(h)
        out.append(kuhn(len(ref_p), len(est_p), i, k))
    return (len(ref_p), len(est_p)) + tuple(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=9)
    ap.add_argument('--host-iters', type=int, default=3)
    ap.add_argument('--notes', type=int, default=6000)
    ap.add_argument('--seconds', type=float, default=300.0)
    args = ap.parse_args()
    from timbre_trap.utils import note_counts, note_counts_device
    from timbre_trap.utils.metrics.notescore import _kuhn
    if not torch.cuda.is_available():
        raise SystemExit('kb_notescore.py measures on the GPU; there is none here')
    dev = torch.device('cuda:0')
    case = synthetic_track(args.notes, args.seconds, np.random.default_rng(args.notes))
    ref_p, ref_iv, est_p, est_iv = case
    up = lambda p, iv: (torch.zeros(len(p), dtype=torch.int32, device=dev), torch.from_numpy(p).to(dev),                  # noqa: E731
                        torch.from_numpy(iv[:, 0].copy()).to(dev), torch.from_numpy(iv[:, 1].copy()).to(dev))
    est_d, ref_d = up(est_p, est_iv), up(ref_p, ref_iv)

    def timed(fn):
        fn()                                                   # once untimed: lazy kernel loading, allocator growth
        fn()
        ms = []
        for _ in range(args.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    got = note_counts_device(est_d, ref_d, n_items=1)
    dev_ms = timed(lambda: note_counts_device(est_d, ref_d, n_items=1))
    up_ms = timed(lambda: note_counts_device(est_d, [(ref_p, ref_iv)]))

    win_ms, dense_ms, down_ms, windowed, dense = [], [], [], None, None
    for _ in range(args.host_iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_est = [t.cpu().numpy() for t in est_d]
        down_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        windowed = note_counts(ref_p, ref_iv, host_est[1], np.stack(host_est[2:], axis=1))
        win_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        dense = dense_route(ref_p, ref_iv, est_p, est_iv, _kuhn)
        dense_ms.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median
    mine = (int(got.n_ref[0]), int(got.n_est[0]), int(got.tp[0]), int(got.tp_no_offset[0]))
    equal = None if windowed is None else bool(mine == tuple(windowed) == tuple(dense))
    r3 = lambda v: round(v, 3)                                 # noqa: E731
    print(json.dumps(dict(notes=args.notes, seconds=args.seconds, n_ref=mine[0], n_est=mine[1], tp=mine[2], tp_no_offset=mine[3],
                          n_fallback=got.n_fallback,
                          device_ms=r3(med(dev_ms)), device_ms_min=r3(min(dev_ms)), device_ms_max=r3(max(dev_ms)),
                          device_up_ms=r3(med(up_ms)), device_up_ms_min=r3(min(up_ms)), device_up_ms_max=r3(max(up_ms)),
                          download_ms=r3(med(down_ms)) if down_ms else None,
                          windowed_ms=round(med(win_ms), 1) if win_ms else None, windowed_ms_min=round(min(win_ms), 1) if win_ms else None,
                          dense_ms=round(med(dense_ms), 1) if dense_ms else None, dense_ms_min=round(min(dense_ms), 1) if dense_ms else None,
                          windowed_over_device=round(med(win_ms) / med(dev_ms), 1) if win_ms else None,
                          dense_over_device=round(med(dense_ms) / med(dev_ms), 1) if dense_ms else None, equal=equal)), flush=True)


if __name__ == '__main__':
    main()
