"""
The FiLM variant on the bench shape (64 clips x 3 s, model_complexity 2, latent 128, consistency on, FusedAdamW):
  * tt_film_fwd in its pair form and tt_film_bwd (dx + the four parameter gradients) on latents 64 x 128 x 1024, event-timed, with the
    bytes they move and the bandwidth that makes;
  * the train step of reference experiments/train.py:404-496 for TimbreTrap and TimbreTrapFiLM, timed ALTERNATELY in one process, under
    bf16 and under fp16 autocast.

    python tools/kb_film.py [--clips 64] [--steps 20] [--warmup 3] [--rounds 3] [--dtypes bf16,fp16]

One JSON line per configuration: for the kernels microseconds per call (median, min, max over the rounds) and GB/s; for the steps ms/step
(median over the rounds and their spread), audio-s/s, peak memory, ratio to the TimbreTrap step of the same round.
"""

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'timbre-trap_amd'))

import torch  # noqa: E402

SR, SECS = 22050, 3


def make_step(model, opt, dtype):
    from timbre_trap.framework import compute_consistency_loss, compute_reconstruction_loss, compute_transcription_loss

    def step(audio, target):
        coefficients = model.sliCQ(audio)
        with torch.autocast(device_type='cuda', dtype=dtype):
            rec, _, trn, trn_rec, trn_scr, _ = model(audio, True)
            act = model.to_activations(trn)
            l_sp, l_sc = compute_consistency_loss(trn_rec, trn_scr, trn)
            total = compute_reconstruction_loss(rec, coefficients) + compute_transcription_loss(act, target, True) + (l_sp + l_sc)
            opt.zero_grad()
            total.backward()
        opt.step()
        return total
    return step


def time_it(fn, n):
    fn()                                                      # once untimed: lazy kernel loading, allocator growth
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def event_us(fn, n):
    """Microseconds per call between two events on the launch stream around n calls (after one untimed call)."""
    fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / n


def kernels(args, dev):
    from timbre_trap import _hip
    lib, P = _hip.lib(), _hip.ptr
    B, D, T = args.clips, 128, 1024
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, D, T, generator=g).to(dev)
    dy = torch.randn(2 * B, D, T, generator=g).to(dev)
    gw, gb, bw, bb = (torch.randn(s, generator=g).to(dev) for s in ((D, 2), (D,), (D, 2), (D,)))
    y, dx = torch.empty(2 * B, D, T, device=dev), torch.empty(B, D, T, device=dev)
    grads = [torch.zeros_like(p) for p in (gw, gb, bw, bb)]
    ws = torch.empty(lib.tt_film_scratch_bytes(B, D, T, 2), dtype=torch.uint8, device=dev)
    cond = (ctypes.c_float * 4)(0.0, 1.0, 1.0, 0.0)
    st = _hip.stream_ptr()
    n = B * D * T * 4
    calls = dict(
        film_fwd_pair=(lambda: _hip.check(lib.tt_film_fwd(P(x), P(gw), P(gb), P(bw), P(bb), cond, P(y), B, D, T, 2, st), 'tt_film_fwd'), 3 * n),
        film_bwd_pair=(lambda: _hip.check(lib.tt_film_bwd(P(x), P(dy), P(gw), P(gb), cond, P(dx), P(grads[0]), P(grads[1]), P(grads[2]),
                                                          P(grads[3]), P(ws), B, D, T, 2, st), 'tt_film_bwd'), 4 * n),
        film_bwd_pair_dx_only=(lambda: _hip.check(lib.tt_film_bwd(None, P(dy), P(gw), P(gb), cond, P(dx), None, None, None, None, None,
                                                                  B, D, T, 2, st), 'tt_film_bwd'), 3 * n))
    for name, (fn, nbytes) in calls.items():
        us = [event_us(fn, args.steps * 10) for _ in range(args.rounds)]
        med = statistics.median(us)
        print(json.dumps(dict(config=name, shape=[B, D, T], bytes_moved=nbytes, us_per_call=round(med, 2), us_min=round(min(us), 2),
                              us_max=round(max(us), 2), gb_per_s=round(nbytes / med / 1e3, 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clips', type=int, default=64)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--dtypes', default='bf16,fp16')
    ap.add_argument('--only', default=None, help='time one class only (for a profiler run): TimbreTrap or TimbreTrapFiLM')
    args = ap.parse_args()
    from timbre_trap.framework import TimbreTrap, TimbreTrapFiLM
    from timbre_trap.utils import FusedAdamW
    dev = torch.device('cuda:0')
    if args.only is None:
        kernels(args, dev)
    g = torch.Generator().manual_seed(0)
    audio = (torch.rand(args.clips, 1, SR * SECS, generator=g) * 2 - 1).to(dev)
    target = (torch.rand(args.clips, 540, 1024, generator=g) < 0.01).float().to(dev)
    classes = [c for c in (TimbreTrap, TimbreTrapFiLM) if args.only in (None, c.__name__)]
    for dname in args.dtypes.split(','):
        dtype = dict(bf16=torch.bfloat16, fp16=torch.float16)[dname]
        steps, times, peaks = {}, {c.__name__: [] for c in classes}, {}
        for cls in classes:
            torch.manual_seed(0)
            model = cls(SR, 9, 60, SECS, latent_size=128, model_complexity=2).to(dev)
            opt = FusedAdamW(model.parameters(), lr=1e-4, max_norm=10.0)
            steps[cls.__name__] = make_step(model, opt, dtype)
            for _ in range(args.warmup):
                steps[cls.__name__](audio, target)
        for _ in range(args.rounds):                          # alternate: drift of the machine hits both classes alike
            for name, step in steps.items():
                torch.cuda.reset_peak_memory_stats()
                times[name].append(time_it(lambda: step(audio, target), args.steps))
                peaks[name] = torch.cuda.max_memory_allocated() / 2 ** 30
        for name, ts in times.items():
            row = dict(config='%s_%s' % (name, dname), clips=args.clips, steps=args.steps, rounds=args.rounds,
                       ms_per_step=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3),
                       audio_s_per_s=round(args.clips * SECS / (statistics.median(ts) / 1e3), 1), peak_gib=round(peaks[name], 2))
            if 'TimbreTrap' in times and name != 'TimbreTrap':
                ratios = [t / c for t, c in zip(ts, times['TimbreTrap'])]
                row.update(ratio_to_complex=round(statistics.median(ratios), 4), ratio_min=round(min(ratios), 4),
                           ratio_max=round(max(ratios), 4))
            print(json.dumps(row), flush=True)
        del steps
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
