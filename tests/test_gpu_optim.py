"""
tt_l2norm and tt_adamw_step (csrc/losses.hip) through the C ABI against a float64 restatement of clip_grad_norm_ + AdamW
(oracle/optim.py, anchored to torch in tests/test_optim_restatement.py).

The model-level tests see the optimiser only through parameters within 2e-4 after two steps, and an early AdamW update is about
lr sign(g) whatever the clip coefficient, the weight decay, the place of eps or the step of the bias correction are.  Here the
gradient norms alternate around max_norm over 12 steps, parameters AND moments AND the clipped gradient are compared after every
step, and the bar is taken from the arithmetic: the same recurrence evaluated in fp32 on the CPU differs from float64 by e32; the
kernel may differ by 8 e32 (another association of the same operations, and its norm rounded to fp32).

What a wrong kernel would do here (float64 on the CPU, n = 4099, 12 steps; e32 of the parameters is 3e-7 to 9e-7, so the bar is
at most 7.5e-6): without the factor (1 - lr wd) the parameters move by 2.5e-4 (set 1) and 7.4e-3 (set 2); with step + 1 in the
bias corrections by 6.2e-4, 1.4e-3 and 5.5e-4 (set 3); with eps inside the square root by 7.8e-3, 2.6e-2 and 7.5e-3; with
clip = 1 by 5.4e-3 and 2.6e-2, exp_avg by 12 and 24 (e32 5e-8), and the written gradient by a factor of 39 and 400.  At
n = 2048 * 256 * 4 + 5 and two steps the smallest of these is 5.1e-5 against a bar of 3.2e-6.
"""

import math

import pytest
import torch

from oracle.optim import HYPER, AdamWRestatement, gradient_sequence

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
N_SMALL = 4099                          # no multiple of 4 or 256
N_CAPPED = 2048 * 256 * 4 + 5           # the launch caps the grid at 2048 workgroups: every workgroup takes more than one stride


def _api():
    from timbre_trap import _hip
    return _hip.lib(), _hip.ptr, _hip.check, _hip.stream_ptr()


class _Kernel:
    """The flat buffers of one optimiser and the two C calls, as FusedAdamW makes them."""

    def __init__(self, p0, hp, write_clipped=1):
        self.lib, self.ptr, self.check, self.st = _api()
        self.p = p0.cuda()
        self.g = torch.zeros_like(self.p)
        self.m = torch.zeros_like(self.p)
        self.v = torch.zeros_like(self.p)
        self.hp = hp
        self.clip = bool(hp['max_norm'])
        self.norm = torch.zeros(1, device='cuda') if self.clip else None
        self.skipped = torch.zeros(1, dtype=torch.int32, device='cuda') if self.clip else None
        self.partials = torch.empty(1024, dtype=torch.float64, device='cuda')
        self.calls = 0
        self.write_clipped = write_clipped

    def step(self, grad, poison_norm=False):
        self.g.copy_(grad)
        if self.clip:
            self.check(self.lib.tt_l2norm(self.ptr(self.g), self.ptr(self.norm), self.ptr(self.partials), self.g.numel(), self.st), 'tt_l2norm')
            if poison_norm:
                self.norm.fill_(float('nan'))
        self.calls += 1
        hp = self.hp
        self.check(self.lib.tt_adamw_step(self.ptr(self.p), self.ptr(self.g), self.ptr(self.m), self.ptr(self.v), self.ptr(self.norm),
                                          self.g.numel(), hp['lr'], hp['betas'][0], hp['betas'][1], hp['eps'], hp['weight_decay'], self.calls,
                                          float(hp['max_norm'] or 0.0), self.write_clipped, self.ptr(self.skipped), self.st), 'tt_adamw_step')
        torch.cuda.synchronize()


def _as_passed(hp):
    """The C ABI takes its hyperparameters as floats: what the kernel is given is float32(0.999), not 0.999 (1 - beta2 differs by 1.3e-5
    relative between the two, and so would exp_avg_sq).  The references run on the values that are passed."""
    def f32(x):
        return float(torch.tensor(x, dtype=torch.float32))
    return dict(lr=f32(hp['lr']), betas=(f32(hp['betas'][0]), f32(hp['betas'][1])), eps=f32(hp['eps']), weight_decay=f32(hp['weight_decay']),
                max_norm=f32(hp['max_norm']) if hp['max_norm'] else None)


def _err(got, want):
    return float((got.detach().cpu().double() - want).abs().max())


class _Tracker:
    """Kernel error against float64 next to e32, the error of the fp32 CPU evaluation of the same recurrence (running maximum over
    the steps so far, per quantity); the kernel must stay within 8 e32."""

    def __init__(self, p0, hp):
        self.r64 = AdamWRestatement(p0.double(), **_as_passed(hp))
        self.r32 = AdamWRestatement(p0.clone(), **_as_passed(hp))
        self.e32 = dict(p=0.0, m=0.0, v=0.0)
        self.worst = dict(p=0.0, m=0.0, v=0.0)

    def step(self, grad):
        self.r32.step(grad)
        norm, g64 = self.r64.step(grad.double())
        for k in 'pmv':
            self.e32[k] = max(self.e32[k], float((getattr(self.r32, k).double() - getattr(self.r64, k)).abs().max()))
        return norm, g64

    def check(self, k, what):
        for q, got in (('p', k.p), ('m', k.m), ('v', k.v)):
            e = _err(got, getattr(self.r64, q))
            ratio = e / max(self.e32[q], 1e-300)
            self.worst[q] = max(self.worst[q], ratio)
            assert e <= 8 * self.e32[q], '%s %s: kernel error %.3e, e32 %.3e (ratio %.2f)' % (what, q, e, self.e32[q], ratio)


def _check_gradient(k, grad, g64, norm64, what):
    """write_clipped = 1: the buffer holds g * clip.  Four fp32 roundings lie between the float64 value and the kernel's: the norm, its
    sum with 1e-6, the quotient, the product; where the clip does not act the gradient is bitwise what it was."""
    got = k.g.cpu()
    if not k.clip or float(norm64) + 1e-6 <= k.hp['max_norm'] * (1 - 4 * U):
        assert torch.equal(got, grad), '%s: an unclipped gradient was rewritten' % what
        return 0.0
    bar = ((1 + U) ** 4 - 1) * g64.abs()
    e = (got.double() - g64).abs()
    assert bool((e <= bar).all()), '%s: clipped gradient off by %.3e of the bar' % (what, float((e / bar.clamp_min(1e-300)).max()))
    assert bool((got[::97] == 0).all())
    return float((e / bar.clamp_min(1e-300)).max())


@pytest.mark.parametrize('hp', range(len(HYPER)))
@pytest.mark.parametrize('n,steps', [(N_SMALL, 12), (N_CAPPED, 2)])
def test_adamw_step_matches_float64_after_every_step(n, steps, hp):
    """Parameters, exp_avg, exp_avg_sq, the clipped gradient and the norm after each of 12 steps (2 at the capped-grid size).
    The kernel's ratio to e32 is printed per case (pytest -rP).  Measured on an MI355X (bar 8): parameters 1.00 in all six cases,
    exp_avg at most 1.12 and exp_avg_sq at most 2.05 (n = 4099, set 1; 1.00 elsewhere); the clipped gradient at most 0.47 of its bar."""
    hp = HYPER[hp]
    p0, grads = gradient_sequence(n, steps)
    k, t = _Kernel(p0, hp), _Tracker(p0, hp)
    gworst = 0.0
    for s, grad in enumerate(grads):
        k.step(grad)
        norm64, g64 = t.step(grad)
        what = 'n %d step %d' % (n, s)
        if k.clip:
            assert abs(float(k.norm) - float(norm64)) <= 1e-6 * float(norm64), what
            assert int(k.skipped) == 0
        gworst = max(gworst, _check_gradient(k, grad, g64, norm64, what))
        t.check(k, what)
    print('adamw n %d hp %s: kernel error / e32: p %.2f m %.2f v %.2f | e32 p %.2e | clipped gradient / bar %.2f'
          % (n, hp, t.worst['p'], t.worst['m'], t.worst['v'], t.e32['p'], gworst))


@pytest.mark.parametrize('hp', [0, 1])
def test_write_clipped_0_leaves_the_gradient_buffer_alone(hp, n=N_SMALL, steps=4):
    """The same update (parameters and moments against float64), the flat gradient bitwise untouched although the clip acts."""
    hp = HYPER[hp]
    p0, grads = gradient_sequence(n, steps)
    k, t = _Kernel(p0, hp, write_clipped=0), _Tracker(p0, hp)
    for s, grad in enumerate(grads):
        k.step(grad)
        t.step(grad)
        assert torch.equal(k.g.cpu(), grad)
        t.check(k, 'step %d' % s)


def test_nan_norm_skips_the_step_and_the_bias_corrections(n=N_SMALL, steps=12, at=4):
    """A non-finite norm before step 4: nothing changes, skipped becomes 1, and every later step equals the float64 run WITHOUT that
    call -- the bias corrections count applied updates, not calls."""
    hp = HYPER[0]
    p0, grads = gradient_sequence(n, steps)
    k, t = _Kernel(p0, hp), _Tracker(p0, hp)
    for s, grad in enumerate(grads):
        if s == at:
            before = [x.clone() for x in (k.p, k.m, k.v)]
            k.step(grad, poison_norm=True)
            assert int(k.skipped) == 1
            assert all(torch.equal(a, b) for a, b in zip(before, (k.p, k.m, k.v)))
            assert torch.equal(k.g.cpu(), grad)
        k.step(grad)
        t.step(grad)
        assert int(k.skipped) == (1 if s >= at else 0)
        t.check(k, 'step %d' % s)
    assert k.calls == steps + 1


def test_fused_adamw_passes_its_hyperparameters_in_order(n=N_SMALL, steps=12):
    """The same gradient sequence written into FusedAdamW.flat_grad, hyperparameter set 2 (eps 1e-6, weight decay 0.1, betas 0.8 / 0.95,
    max_norm 1: no two of them equal, so a swapped pair in the call shows)."""
    from timbre_trap.utils import FusedAdamW
    hp = HYPER[1]
    p0, grads = gradient_sequence(n, steps)
    param = torch.nn.Parameter(p0.cuda())
    opt = FusedAdamW([param], **hp)
    t = _Tracker(p0, hp)

    class View:
        pass
    for s, grad in enumerate(grads):
        opt.flat_grad.copy_(grad)
        norm = opt.step()
        torch.cuda.synchronize()
        norm64, _ = t.step(grad)
        assert abs(float(norm) - float(norm64)) <= 1e-6 * float(norm64)
        k = View()
        k.p, k.m, k.v = opt.flat_param, opt.exp_avg, opt.exp_avg_sq
        t.check(k, 'step %d' % s)
        assert param.data_ptr() == opt.flat_param.data_ptr()
    assert int(opt.skipped) == 0


@pytest.mark.parametrize('big', [False, True])
@pytest.mark.parametrize('n', [1, 255, 257, 4099, 1024 * 256 * 8 + 3])
def test_l2norm_matches_float64(n, big):
    """sqrt of a sum accumulated in double, rounded once to fp32: 1e-6 relative.  ``big``: one element of 1e19, whose square (1e38) is
    at the top of the fp32 range -- squared or accumulated in fp32 it would swallow the rest or overflow with the next partial sum."""
    lib, ptr, check, st = _api()
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen)
    if big:
        x[n // 2] = 1e19
    out = torch.full((1,), float('nan'), device='cuda')
    partials = torch.full((1024,), float('nan'), dtype=torch.float64, device='cuda')
    xd = x.cuda()
    check(lib.tt_l2norm(ptr(xd), ptr(out), ptr(partials), n, st), 'tt_l2norm')
    torch.cuda.synchronize()
    want = math.sqrt(float((x.double() ** 2).sum()))
    assert torch.equal(xd.cpu(), x)
    assert abs(float(out) - want) <= 1e-6 * want, (float(out), want)
