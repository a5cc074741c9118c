"""Forward + backward of ONE wide level (three residual blocks, dilation 1, 2, 3) at the bench's plane sizes (64 clips): the split-operand
   training route (ops.X3LevelTrainFn, TTRAP_X3_TRAIN) against three ResBlockFn on the exact-fp32 kernels -- alternating, in one process,
   warmed up, device events, KB_ROUNDS rounds of KB_N passes each.  Per width: milliseconds per forward + backward of either route in every
   round, the spread over the rounds, and the ratio fp32 / x3 (a width whose ratio is not above 1 by more than the spread stays off
   ops.X3_TRAIN_CHANNELS).
   KB_C=16,32 KB_N=5 KB_ROUNDS=3 python tools/kb_x3_train.py"""
import os
import sys
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'timbre-trap_amd'))
from timbre_trap.framework import ops

SHAPES = {32: (64, 65, 1024), 16: (64, 133, 1024)}
DILATIONS = (1, 2, 3)


def passes(fn, n):
    """Milliseconds per call of fn (forward, backward) and of its two halves, over n calls between device events."""
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(n)]
    for e in ev:
        e[0].record()
        y = fn.forward()
        e[1].record()
        fn.backward(y)
        e[2].record()
        del y
    torch.cuda.synchronize()
    fwd = sum(e[0].elapsed_time(e[1]) for e in ev) / n
    bwd = sum(e[1].elapsed_time(e[2]) for e in ev) / n
    return fwd + bwd, fwd, bwd


class Level:
    def __init__(self, route, x, params, dy):
        self.route, self.x, self.params, self.dy = route, x, params, dy

    def forward(self):
        if self.route == 'x3':
            return ops.X3LevelTrainFn.apply(self.x, DILATIONS, *self.params)
        y = self.x
        for i, d in enumerate(DILATIONS):
            y = ops.ResBlockFn.apply(y, *self.params[4 * i:4 * i + 4], d)
        return y

    def backward(self, y):
        torch.autograd.grad(y, [self.x] + self.params, self.dy)


def main():
    ops.PRECISION = 'fp32'
    n, rounds = int(os.environ.get('KB_N', 5)), int(os.environ.get('KB_ROUNDS', 3))
    torch.manual_seed(0)
    for C in [int(c) for c in os.environ.get('KB_C', '16,32').split(',')]:
        B, H, T = SHAPES[C]
        B = int(os.environ.get('KB_B', B))
        x = torch.randn(B, C, H, T, device='cuda').requires_grad_(True)
        params = []
        for _ in DILATIONS:
            params += [torch.randn(C, C, 3, 3, device='cuda') / (3 * C ** 0.5), torch.randn(C, device='cuda') * 0.1,
                       torch.randn(C, C, 1, 1, device='cuda') / C ** 0.5, torch.randn(C, device='cuda') * 0.1]
        params = [p.requires_grad_(True) for p in params]
        dy = torch.randn(B, C, H, T, device='cuda') * 1e-8            # the size of a mean-reduced loss's activation gradients
        levels = {r: Level(r, x, params, dy) for r in ('x3', 'fp32')}
        for lv in levels.values():                                    # warm-up: allocator, kernel attributes, clocks
            passes(lv, 2)
        res = {r: [] for r in levels}
        for _ in range(rounds):
            for r, lv in levels.items():                              # alternating
                res[r].append(passes(lv, n))
        for r in levels:
            tot = [v[0] for v in res[r]]
            print('C%d B%d H%d T%d %-4s fwd+bwd ms per round: %s | mean %.3f spread %.3f | fwd %.3f bwd %.3f'
                  % (C, B, H, T, r, ' '.join('%.3f' % v for v in tot), sum(tot) / len(tot), max(tot) - min(tot),
                     sum(v[1] for v in res[r]) / rounds, sum(v[2] for v in res[r]) / rounds))
        m3, m32 = (sum(v[0] for v in res[r]) / rounds for r in ('x3', 'fp32'))
        spread = max(max(v[0] for v in res[r]) - min(v[0] for v in res[r]) for r in levels)
        print('C%d ratio fp32 / x3 = %.2f (x3 faster by %.3f ms; largest spread %.3f ms)' % (C, m32 / m3, m32 - m3, spread))


if __name__ == '__main__':
    main()
