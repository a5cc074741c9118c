"""
The device audio preparation (csrc/resample.hip; timbre_trap.utils.prepare_audio) against the host route on one machine, at the
shape AudioDataset.get_audio meets: a five-minute stereo track at 48 kHz and at 44.1 kHz -> mono 22.05 kHz, inf-normalised.

    python tools/kb_resample.py [--seconds 300] [--rounds 5] [--iters 10] [--host-iters 5] [--threads 16] [--out FILE]

Per source rate one JSON line (times in ms; every device figure is a median over --rounds rounds of --iters event-timed calls each,
with the smallest and largest round median next to it as the spread):
  device_ms          prepare_audio on a track that is already on the device: two launches (mix + polyphase FIR + peaks, division)
  resample_ms        tt_resample alone on preallocated buffers (peaks included);  gfma_per_s = Lout K multiply-adds / resample_ms
  normalize_ms       tt_resample_normalize alone
  upload_ms          the raw (2, N) fp32 track from pinned host memory to the device (non_blocking copy between the events)
  device_upload_ms   upload + prepare_audio between one pair of events: what a loader pays per track
  pageable_ms        the same from ordinary (pageable) host memory
  host_ms            torch.mean -> fp32 conv1d with the same taps (torchaudio's arithmetic) -> division, on --threads CPU threads of
                     the same machine; median / min / max of --host-iters runs by the wall clock, after one untimed run
  host_over_device   host_ms / device_upload_ms
  max_abs_diff       largest |device - host| over the normalised track (both fp32 routes; the peak is 1)
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


def event_ms(fn, iters):
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def rounds_ms(fn, rounds, iters):
    """(median, min, max) over the round medians."""
    fn()                                                           # once untimed: lazy kernel loading, allocator growth
    torch.cuda.synchronize()
    meds = [event_ms(fn, iters) for _ in range(rounds)]
    return [round(v, 4) for v in (statistics.median(meds), min(meds), max(meds))]


def host_route(track, taps32, orig, width, n_out):
    mono = torch.mean(track, dim=0, keepdim=True)
    padded = torch.nn.functional.pad(mono[None], (width, width + orig))
    y = torch.nn.functional.conv1d(padded, taps32[:, None], stride=orig).transpose(1, 2).reshape(1, -1)[:, :n_out]
    peak = y.abs().max()
    if peak:
        y /= peak
    return y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=300.0)
    ap.add_argument('--rates', default='48000,44100')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--host-iters', type=int, default=5)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    args = ap.parse_args()
    from timbre_trap import _hip
    from timbre_trap.utils import prepare_audio, sinc_resample_kernel
    from timbre_trap.utils import audio
    if not torch.cuda.is_available():
        raise SystemExit('kb_resample needs the GPU: no time is reported without one')
    torch.set_num_threads(args.threads)
    dev = torch.device('cuda:0')
    lib, target = _hip.lib(), 22050
    for fs in (int(v) for v in args.rates.split(',')):
        n = int(round(args.seconds * fs))
        g = torch.Generator().manual_seed(fs)
        host_track = (torch.rand(2, n, generator=g) - 0.5)
        pinned = host_track.pin_memory()
        x = host_track.to(dev)
        taps, width, orig, new = sinc_resample_kernel(fs, target)
        K, n_out = taps.shape[1], -(-new * n // orig)

        dev_ms = rounds_ms(lambda: prepare_audio(x, fs, target), args.rounds, args.iters)
        xb = x[None].contiguous()
        y = torch.empty(1, n_out, device=dev)
        n_part = lib.tt_resample_partials(n, orig, new)
        part = torch.empty(1, n_part, device=dev)
        taps_t = audio._taps_on(dev, orig, new, 6, 0.99)
        st = _hip.stream_ptr()
        rs_ms = rounds_ms(lambda: _hip.check(lib.tt_resample(_hip.ptr(xb), 1, 2, n, _hip.ptr(taps_t), orig, new, width, _hip.ptr(y), n_out,
                                                             _hip.ptr(part), st)), args.rounds, args.iters)
        nm_ms = rounds_ms(lambda: _hip.check(lib.tt_resample_normalize(_hip.ptr(y), 1, n_out, _hip.ptr(part), n_part, st)), args.rounds, args.iters)
        up_ms = rounds_ms(lambda: pinned.to(dev, non_blocking=True), args.rounds, args.iters)
        du_ms = rounds_ms(lambda: prepare_audio(pinned.to(dev, non_blocking=True), fs, target), args.rounds, args.iters)
        pg_ms = rounds_ms(lambda: prepare_audio(host_track.to(dev), fs, target), args.rounds, args.iters)

        taps32 = torch.from_numpy(taps.astype(np.float32))
        host, ref = [], None
        if args.host_iters:
            host_route(host_track, taps32, orig, width, n_out)          # once untimed: thread-pool start, allocator growth
        for _ in range(args.host_iters):
            t0 = time.perf_counter()
            ref = host_route(host_track, taps32, orig, width, n_out)
            host.append((time.perf_counter() - t0) * 1e3)
        got = prepare_audio(x, fs, target).cpu()
        diff = float((got - ref).abs().max()) if ref is not None else None
        line = json.dumps(dict(fs=fs, seconds=args.seconds, N=n, N_out=n_out, orig=orig, new=new, K=K, device_ms=dev_ms, resample_ms=rs_ms,
                               gfma_per_s=round(n_out * K / rs_ms[0] / 1e6, 1), normalize_ms=nm_ms, upload_ms=up_ms,
                               upload_gb_per_s=round(2 * n * 4 / up_ms[0] / 1e6, 1), device_upload_ms=du_ms, pageable_ms=pg_ms,
                               host_threads=args.threads,
                               host_ms=[round(v, 1) for v in (statistics.median(host), min(host), max(host))] if host else None,
                               host_over_device=round(statistics.median(host) / du_ms[0], 1) if host else None, max_abs_diff=diff))
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
