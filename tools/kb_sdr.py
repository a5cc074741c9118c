"""
The device SDR (csrc/sdr.hip) against the host function on one machine, at the shapes evaluate() meets: (1, 1, N) for
N = 66150 (3 s), 22050 x 30 and 22050 x 300 (a 5-minute track), filter_length 512.

    python tools/kb_sdr.py [--iters 20] [--host-iters 1] [--lengths 66150,661500,6615000]

Per length one JSON line:
  device_ms        `SignalDistortionRatio().to(device)(p, t).item()` as evaluate.py:122-127 calls it, between two HIP events (the
                   second recorded after .item() returned), median over --iters
  correlate_ms     tt_sdr_correlate alone (correlation kernel + the ordered sum of its chunk rows) on preallocated buffers
  gfma_per_s       2 L N float64 multiply-adds / correlate_ms
  finish_ms        tt_sdr_finish alone (normalisation + 511 Levinson steps in one wave)
  host_ms          signal_distortion_ratio on the same tensors moved to the host (copy included, as evaluate() would pay it)
  diff_db          |signal_distortion_ratio_device - host| in float64
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'timbre-trap_amd'))

import torch  # noqa: E402


def event_ms(fn, iters):
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--host-iters', type=int, default=1)
    ap.add_argument('--lengths', default='66150,661500,6615000')
    args = ap.parse_args()
    from timbre_trap import _hip
    from timbre_trap.utils import SignalDistortionRatio, signal_distortion_ratio, signal_distortion_ratio_device
    dev = torch.device('cuda:0')
    lib, L = _hip.lib(), 512
    module = SignalDistortionRatio().to(dev)
    for n in (int(v) for v in args.lengths.split(',')):
        g = torch.Generator().manual_seed(n)
        t = torch.randn(1, 1, n, generator=g)
        t = t + 0.9 * torch.roll(t, 1, -1)                    # coloured target
        p = (0.7 * t + 0.1 * torch.randn(1, 1, n, generator=g)).to(dev)
        t = t.to(dev)
        module(p, t).item()                                   # once untimed: lazy kernel loading, allocator growth
        value = signal_distortion_ratio_device(p, t).item()   # float64 (the module returns preds' dtype)
        dev_ms = event_ms(lambda: module(p, t).item(), args.iters)
        scratch = torch.empty(lib.tt_sdr_scratch_bytes(1, n, L) // 8, dtype=torch.float64, device=dev)
        rb = torch.empty(1, 2 * L + 1, dtype=torch.float64, device=dev)
        out = torch.empty(2, dtype=torch.float64, device=dev)
        st = _hip.stream_ptr()
        corr_ms = event_ms(lambda: _hip.check(lib.tt_sdr_correlate(_hip.ptr(p), _hip.ptr(t), 1, n, L, None, _hip.ptr(scratch), _hip.ptr(rb), st)),
                           args.iters)
        fin_ms = event_ms(lambda: _hip.check(lib.tt_sdr_finish(_hip.ptr(rb), 1, L, 0.0, 0, _hip.ptr(out[0:]), _hip.ptr(out[1:]), st)), args.iters)
        host, ref = [], float('nan')                           # --host-iters 0: device figures only (profiler runs)
        for _ in range(args.host_iters):
            t0 = time.perf_counter()
            ref = float(signal_distortion_ratio(p, t).reshape(-1)[0])
            host.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps(dict(N=n, seconds=round(n / 22050, 2), filter_length=L, sdr_db=round(value, 6), diff_db=abs(value - ref),
                              device_ms=round(dev_ms[0], 4), device_ms_min=round(dev_ms[1], 4), device_ms_max=round(dev_ms[2], 4),
                              correlate_ms=round(corr_ms[0], 4), gfma_per_s=round(2 * L * n / corr_ms[0] / 1e6, 1),
                              finish_ms=round(fin_ms[0], 4), host_ms=round(statistics.median(host), 1) if host else None,
                              host_over_device=round(statistics.median(host) / dev_ms[0], 1) if host else None)), flush=True)


if __name__ == '__main__':
    main()
