"""
One Griffin-Lim iteration of tt_cqt_griffin_lim on the bench shape (64 clips x 1 block of 3 s), beside its two yardsticks:

  * the composed iteration: tt_cqt_forward with complex output, the projection mag c / |c| as torch expressions, tt_cqt_inverse -- which
    writes and re-reads the coefficients and their projection (CQT.griffin_lim with the private flag that keeps this route reachable);
  * tt_cqt_forward_mag_bwd, nearly the same launches: the fused iteration adds the momentum's pass over the audio, the partial sums of the
    convergence and their reduction (when asked) to them.

The cost of ONE iteration is the difference of two calls, (t(n_iter = 1 + K) - t(1)) / K: a steady-state iteration with its extrapolation,
without the call's fixed part.  It is reported with and without the convergence, beside the single call t(1).

    python tools/kb_griffin_lim.py [--clips 64] [--calls 20] [--rounds 5] [--iters 8] [--out profiles/kb_griffin_lim.txt]

Event timing; every round times each entry of a pair once, ALTERNATELY, in one process; per entry the median over the rounds with its
minimum and maximum, per pair the ratio of the medians and the spread the yardstick shows between its own rounds (max / min).  One JSON
line per pair, printed and written to --out.
"""

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'timbre-trap_amd'))

import torch  # noqa: E402

SR, SECS, N, M, F = 22050, 3, 66150, 1024, 540


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clips', type=int, default=64)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=8, help='K: iterations added to the one-iteration call to price one')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kb_griffin_lim.txt'))
    args = ap.parse_args()
    from timbre_trap import _hip
    from timbre_trap.framework import CQT
    dev = torch.device('cuda:0')
    cq = CQT(9, 60, SR, SECS).to(dev)
    lib, P, st = _hip.lib(), _hip.ptr, _hip.stream_ptr()
    ps = cq._plan_struct(dev)
    plan = ctypes.byref(ps)
    B, K = args.clips, args.iters
    g = torch.Generator().manual_seed(0)
    audio = (torch.rand(B, 1, N, generator=g) * 2 - 1).to(dev)
    audio_out = torch.empty_like(audio)
    mag = cq.magnitude(audio) * (0.5 + torch.rand(B, F, M, generator=g)).to(dev)
    conv = torch.empty(1 + K, B, device=dev)
    scratch = torch.empty(lib.tt_cqt_griffin_lim_scratch_bytes(B, F, cq._sum_len), dtype=torch.uint8, device=dev)
    audio_b, mag_b = B * N * 4, B * F * M * 4

    def fused(n_iter, with_conv):
        return lambda: _hip.check(lib.tt_cqt_griffin_lim(plan, P(mag), P(audio), P(audio_out), P(conv) if with_conv else None, P(scratch),
                                                         B, 1, n_iter, 0.99, 0, st), 'tt_cqt_griffin_lim')

    def composed(n_iter):
        def run():
            cq._gl_composed = True
            try:
                cq.griffin_lim(mag, n_iter=n_iter, momentum=0.99, audio_init=audio, normalize=False)
            finally:
                cq._gl_composed = False
        return run

    def mag_bwd():
        _hip.check(lib.tt_cqt_forward_mag_bwd(plan, P(audio), P(mag), P(audio_out), P(scratch), B, 1, st), 'tt_cqt_forward_mag_bwd')

    def per_iteration(make):
        """(one-iteration call, steady-state iteration) in microseconds"""
        one, many = event_us(make(1), args.calls), event_us(make(1 + K), max(1, args.calls // 4))
        return one, (many - one) / K

    # a steady-state iteration reads the magnitudes and the audio, writes the audio, and the extrapolation reads two and writes one
    iter_b = mag_b + 2 * audio_b + 3 * audio_b
    rows = {k: [] for k in ('fused_one', 'fused_iter', 'fused_conv_one', 'fused_conv_iter', 'composed_one', 'composed_iter', 'mag_bwd')}
    for _ in range(args.rounds):                              # alternate: drift of the machine hits all alike
        rows['mag_bwd'].append(event_us(mag_bwd, args.calls))
        o, i = per_iteration(lambda n: fused(n, False))
        rows['fused_one'].append(o); rows['fused_iter'].append(i)
        o, i = per_iteration(composed)
        rows['composed_one'].append(o); rows['composed_iter'].append(i)
        o, i = per_iteration(lambda n: fused(n, True))
        rows['fused_conv_one'].append(o); rows['fused_conv_iter'].append(i)

    def stat(key):
        t = rows[key]
        return dict(us=round(statistics.median(t), 2), us_min=round(min(t), 2), us_max=round(max(t), 2))

    def spread(key):
        return round(max(rows[key]) / min(rows[key]), 4)

    med = {k: statistics.median(v) for k, v in rows.items()}
    lines = []
    for name, new, yard, yard_name in (
            ('iteration_vs_composed', 'fused_iter', 'composed_iter', 'composed iteration: tt_cqt_forward(complex) + torch projection + tt_cqt_inverse'),
            ('iteration_with_convergence_vs_composed', 'fused_conv_iter', 'composed_iter', 'composed iteration (no convergence)'),
            ('iteration_vs_mag_bwd', 'fused_iter', 'mag_bwd', 'tt_cqt_forward_mag_bwd'),
            ('iteration_with_convergence_vs_mag_bwd', 'fused_conv_iter', 'mag_bwd', 'tt_cqt_forward_mag_bwd'),
            ('single_call_vs_mag_bwd', 'fused_one', 'mag_bwd', 'tt_cqt_forward_mag_bwd'),
            ('single_call_vs_composed', 'fused_one', 'composed_one', 'composed, n_iter = 1')):
        row = dict(config=name, clips=B, calls=args.calls, rounds=args.rounds, iters_added=K, entry='tt_cqt_griffin_lim: ' + new,
                   yardstick=yard_name, algorithmic_bytes=iter_b if 'iter' in new else mag_b + 2 * audio_b,
                   **{'entry_' + k: v for k, v in stat(new).items()}, **{'yardstick_' + k: v for k, v in stat(yard).items()},
                   ratio_to_yardstick=round(med[new] / med[yard], 4), yardstick_own_spread=spread(yard), entry_own_spread=spread(new))
        row['gb_per_s'] = round(row['algorithmic_bytes'] / med[new] / 1e3, 1)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('# python tools/kb_griffin_lim.py --clips %d --calls %d --rounds %d --iters %d   (%s)\n'
                % (B, args.calls, args.rounds, K, torch.cuda.get_device_name(0)))
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
