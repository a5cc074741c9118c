"""
The adjoint entry points of the constant-Q transform on the bench shape (64 clips x 1 block of 3 s), each beside its yardstick:

  * tt_cqt_forward_bwd (planes in)      against tt_cqt_inverse with normalize = 0 -- the same launches on the same bytes;
  * tt_cqt_inverse_bwd (planes out)     against tt_cqt_forward                    -- the same launches on the same bytes;
  * tt_cqt_forward_mag_bwd (fused)      against the composed route: tt_cqt_forward with complex output, torch's norm backward
                                        (dmag c / |c|), tt_cqt_forward_bwd -- which writes and re-reads the coefficients and their gradient.

    python tools/kb_cqt_grad.py [--clips 64] [--calls 50] [--rounds 5] [--out profiles/kb_cqt_grad.txt]

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
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kb_cqt_grad.txt'))
    args = ap.parse_args()
    from timbre_trap import _hip
    from timbre_trap.framework import CQT
    dev = torch.device('cuda:0')
    cq = CQT(9, 60, SR, SECS).to(dev)
    lib, P, st = _hip.lib(), _hip.ptr, _hip.stream_ptr()
    ps = cq._plan_struct(dev)
    plan = ctypes.byref(ps)
    B = args.clips
    g = torch.Generator().manual_seed(0)
    audio = (torch.rand(B, 1, N, generator=g) * 2 - 1).to(dev)
    audio_out = torch.empty_like(audio)
    planes = torch.empty(B, 2, F, M, device=dev)
    planes_out = torch.empty_like(planes)
    cplx = torch.empty(B, 1, F, M, 2, device=dev)
    scratch = cq._scratch(lib, ps, B, dev)
    _hip.check(lib.tt_cqt_forward(plan, P(audio), P(planes), P(scratch), B, 1, 0, st), 'tt_cqt_forward')
    dmag = torch.rand(B, F, M, generator=g).to(dev)
    audio_b, coeff_b = B * N * 4, B * 2 * F * M * 4

    def composed_magnitude_bwd():
        _hip.check(lib.tt_cqt_forward(plan, P(audio), P(cplx), P(scratch), B, 1, 1, st), 'tt_cqt_forward')
        c = torch.view_as_complex(cplx)
        mag = c.abs()
        dc = torch.where(mag == 0, torch.zeros_like(c), c * (dmag[:, None] / mag))      # torch's norm backward
        _hip.check(lib.tt_cqt_forward_bwd(plan, P(torch.view_as_real(dc)), P(audio_out), P(scratch), B, 1, 1, st), 'tt_cqt_forward_bwd')

    pairs = [
        ('analysis_gradient', 'tt_cqt_forward_bwd', 'tt_cqt_inverse(normalize=0)', coeff_b + audio_b,
         lambda: _hip.check(lib.tt_cqt_forward_bwd(plan, P(planes), P(audio_out), P(scratch), B, 1, 0, st), 'tt_cqt_forward_bwd'),
         lambda: _hip.check(lib.tt_cqt_inverse(plan, P(planes), P(audio_out), P(scratch), B, 1, 0, 0, st), 'tt_cqt_inverse')),
        ('synthesis_gradient', 'tt_cqt_inverse_bwd', 'tt_cqt_forward', coeff_b + audio_b,
         lambda: _hip.check(lib.tt_cqt_inverse_bwd(plan, P(audio), P(planes_out), P(scratch), B, 1, 0, st), 'tt_cqt_inverse_bwd'),
         lambda: _hip.check(lib.tt_cqt_forward(plan, P(audio), P(planes_out), P(scratch), B, 1, 0, st), 'tt_cqt_forward')),
        ('magnitude_gradient', 'tt_cqt_forward_mag_bwd', 'composed: tt_cqt_forward(complex) + norm backward + tt_cqt_forward_bwd',
         2 * audio_b + coeff_b // 2,
         lambda: _hip.check(lib.tt_cqt_forward_mag_bwd(plan, P(audio), P(dmag), P(audio_out), P(scratch), B, 1, st), 'tt_cqt_forward_mag_bwd'),
         composed_magnitude_bwd),
    ]
    lines = []
    for name, new, yard, nbytes, fn_new, fn_yard in pairs:
        t_new, t_yard = [], []
        for _ in range(args.rounds):                          # alternate: drift of the machine hits both alike
            t_yard.append(event_us(fn_yard, args.calls))
            t_new.append(event_us(fn_new, args.calls))
        m_new, m_yard = statistics.median(t_new), statistics.median(t_yard)
        row = dict(config=name, clips=B, calls=args.calls, rounds=args.rounds, entry=new, yardstick=yard, algorithmic_bytes=nbytes,
                   us_per_call=round(m_new, 2), us_min=round(min(t_new), 2), us_max=round(max(t_new), 2),
                   gb_per_s=round(nbytes / m_new / 1e3, 1),
                   yardstick_us_per_call=round(m_yard, 2), yardstick_us_min=round(min(t_yard), 2), yardstick_us_max=round(max(t_yard), 2),
                   ratio_to_yardstick=round(m_new / m_yard, 4), yardstick_own_spread=round(max(t_yard) / min(t_yard), 4))
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('# python tools/kb_cqt_grad.py --clips %d --calls %d --rounds %d   (%s)\n' % (B, args.calls, args.rounds, torch.cuda.get_device_name(0)))
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
