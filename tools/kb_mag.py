"""
Magnitude variants vs the complex model on the bench shape (64 clips x 3 s, model_complexity 2, latent 128, consistency on, FusedAdamW):
the train step of reference experiments/train.py:404-496 including the :406-413 branches (the magnitude / dB reconstruction target),
TimbreTrap, TimbreTrapMag and TimbreTrapMagDB timed ALTERNATELY in one process, under bf16 and under fp16 autocast; then the front end
alone (CQT + torch norm vs the fused magnitude, the torch per-clip dB loop vs tt_decibels).

    python tools/kb_mag.py [--clips 64] [--steps 20] [--warmup 3] [--rounds 3] [--dtypes bf16,fp16]

One JSON line per configuration: ms/step (median over the rounds, and their spread), audio-s/s, peak memory, ratio to the complex step
of the same round.
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

SR, SECS = 22050, 3


def make_step(model, opt, dtype):
    from timbre_trap.framework import (TimbreTrapMag, TimbreTrapMagDB, compute_consistency_loss, compute_reconstruction_loss,
                                       compute_transcription_loss)

    def step(audio, target):
        coefficients = model.sliCQ(audio)
        if isinstance(model, TimbreTrapMag):                 # train.py:406-413
            coefficients = model.sliCQ.to_magnitude(coefficients).unsqueeze(-3)
        if isinstance(model, TimbreTrapMagDB):
            coefficients = model.sliCQ.to_decibels(coefficients)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clips', type=int, default=64)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--dtypes', default='bf16,fp16')
    ap.add_argument('--only', default=None, help='time one class only (for a profiler run): TimbreTrap, TimbreTrapMag or TimbreTrapMagDB')
    args = ap.parse_args()
    from timbre_trap.framework import CQT, TimbreTrap, TimbreTrapMag, TimbreTrapMagDB
    from timbre_trap.utils import FusedAdamW
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    audio = (torch.rand(args.clips, 1, SR * SECS, generator=g) * 2 - 1).to(dev)
    target = (torch.rand(args.clips, 540, 1024, generator=g) < 0.01).float().to(dev)
    classes = [c for c in (TimbreTrap, TimbreTrapMag, TimbreTrapMagDB) if args.only in (None, c.__name__)]
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
        for _ in range(args.rounds):                          # alternate: drift of the machine hits every class alike
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
    if args.only is not None:
        return
    # ---- the front end alone
    cqt = CQT(9, 60, SR, SECS).to(dev)
    with torch.no_grad():
        c = cqt(audio)
        m = cqt.magnitude(audio)
        n = args.steps

        def db_loop(x):
            out = []
            for v in x:
                d = 20.0 * torch.log10(torch.clamp(v, min=1e-10))
                d = torch.maximum(d, d.max() - 80.0)
                out.append((1 + (d - d.max()) / 80).unsqueeze(0))
            return torch.cat(out, 0)
        rows = dict(cqt_then_torch_norm=time_it(lambda: cqt(audio).norm(p=2, dim=-3), n),
                    cqt_fused_magnitude=time_it(lambda: cqt.magnitude(audio), n),
                    magnitude_kernel=time_it(lambda: CQT.to_magnitude(c), n),
                    torch_norm=time_it(lambda: c.norm(p=2, dim=-3), n),
                    decibels_torch_loop=time_it(lambda: db_loop(m), n),
                    decibels_kernels=time_it(lambda: CQT.to_decibels(m), n))
        err = float((CQT.to_decibels(m) - db_loop(m)).abs().max())
    print(json.dumps(dict(config='front_end', clips=args.clips, **{k: round(v, 4) for k, v in rows.items()}, db_max_abs_diff=err)), flush=True)


if __name__ == '__main__':
    main()
