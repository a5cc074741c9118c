"""
The float64 restatement of clip_grad_norm_ + AdamW that tests/test_gpu_optim.py holds the kernels against (oracle/optim.py) is itself
checked here, on the CPU, against torch.nn.utils.clip_grad_norm_ and torch.optim.AdamW in float64: the reference of the GPU test is
anchored to torch, not to the kernel.
"""

import pytest
import torch

from oracle.optim import HYPER, AdamWRestatement, gradient_sequence


@pytest.mark.parametrize('hp', range(len(HYPER)))
def test_restatement_equals_torch_adamw_in_float64(hp, n=4099, steps=12):
    kw = dict(HYPER[hp])
    max_norm = kw.pop('max_norm')
    p0, grads = gradient_sequence(n, steps)
    ref = AdamWRestatement(p0.double(), max_norm=max_norm, **kw)
    p = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.AdamW([p], **kw)
    coefs = []
    for g in grads:
        p.grad = g.double().clone()
        norm = torch.nn.utils.clip_grad_norm_([p], max_norm) if max_norm else None
        opt.step()
        rnorm, rg = ref.step(g.double())
        if max_norm:
            assert abs(float(rnorm) - float(norm)) <= 1e-14 * float(norm)
            coefs.append(min(1.0, max_norm / (float(norm) + 1e-6)))
        # float64 against float64: a few ulp of the value (different association), far below the fp32 effects the GPU test resolves
        assert float((rg - p.grad).abs().max()) <= 1e-15 * float(p.grad.abs().max())
        st = opt.state[p]
        assert float((ref.p - p.detach()).abs().max()) <= 1e-13
        assert float((ref.m - st['exp_avg']).abs().max()) <= 1e-15 * float(st['exp_avg'].abs().max())
        assert float((ref.v - st['exp_avg_sq']).abs().max()) <= 1e-15 * float(st['exp_avg_sq'].abs().max())
    if max_norm:
        # the inputs do what they are for: the clip acts on some steps and not on others
        assert min(coefs) < 0.1 and max(coefs) == 1.0
