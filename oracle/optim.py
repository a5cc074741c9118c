"""
ORACLE (test infrastructure only -- never imported by the product path).

Plain restatement of ``torch.nn.utils.clip_grad_norm_`` followed by ``torch.optim.AdamW.step`` over one flat tensor
(reference experiments/train.py:334, :493-496), in whatever dtype the inputs have.  tests/test_optim_restatement.py anchors it to
torch in float64; tests/test_gpu_optim.py then holds csrc/losses.hip (tt_l2norm, tt_adamw_step) against it.

  clip coefficient   min(1, max_norm / (norm + 1e-6))
  weight decay       decoupled: p <- p (1 - lr wd) before the update
  bias corrections   1 - beta^t with t the number of APPLIED updates
  denominator        sqrt(v) / sqrt(1 - beta2^t) + eps
"""

import math

import torch


HYPER = (dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=10.0),
         dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.1, max_norm=1.0),
         dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None))


def gradient_sequence(n, steps, seed=0):
    """fp32 parameters 0.5 randn and ``steps`` gradients randn * logspace(-9, 0, n) with every 97th element exactly 0, scaled by 40 on
    steps 0, 3, 6, 9 and by 0.05 otherwise: norms of about 390 and 0.5 at n = 4099, so a clip at 10 or 1 acts on some steps only."""
    gen = torch.Generator().manual_seed(seed)
    param = 0.5 * torch.randn(n, generator=gen)
    span = torch.logspace(-9, 0, n)
    grads = []
    for s in range(steps):
        g = torch.randn(n, generator=gen) * span * (40.0 if s % 3 == 0 and s < 12 else 0.05)
        g[::97] = 0.0
        grads.append(g)
    return param, grads


class AdamWRestatement:
    def __init__(self, param, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None):
        self.p = param.clone()
        self.m = torch.zeros_like(param)
        self.v = torch.zeros_like(param)
        self.lr, self.betas, self.eps, self.wd, self.max_norm = lr, betas, eps, weight_decay, max_norm
        self.t = 0

    def step(self, grad):
        """One update from ``grad`` (not modified).  Returns (pre-clip norm or None, the gradient that went into the moments)."""
        b1, b2 = self.betas
        norm = None
        g = grad
        if self.max_norm:
            norm = (grad * grad).sum().sqrt()
            coef = self.max_norm / (norm + 1e-6)
            g = grad * torch.clamp(coef, max=1.0)
        self.t += 1
        self.p = self.p * (1 - self.lr * self.wd)
        self.m = b1 * self.m + (1 - b1) * g
        self.v = b2 * self.v + (1 - b2) * g * g
        step_size = self.lr / (1 - b1 ** self.t)
        denom = self.v.sqrt() / math.sqrt(1 - b2 ** self.t) + self.eps
        self.p = self.p - step_size * (self.m / denom)
        return norm, g
