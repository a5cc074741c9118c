"""CPU-only: the magnitude variants TimbreTrapMag / TimbreTrapMagDB construct with the reference's parameters (tests/golden/variants.npz,
recorded from the reference by tests/golden/make_golden_variants.py), FiLM still raises, and the CPU paths of CQT.to_magnitude /
CQT.to_decibels keep their torch arithmetic."""

import numpy as np
import pytest
import torch

CLASSES = ('TimbreTrapMag', 'TimbreTrapMagDB')


def _cls(name):
    import timbre_trap.framework as fw
    return getattr(fw, name)


@pytest.mark.parametrize('name', CLASSES)
@pytest.mark.parametrize('mc', (1, 2))
def test_state_dict_keys_shapes_and_initial_weights_match_the_reference(golden, name, mc):
    g = golden('variants')
    torch.manual_seed(0)
    model = _cls(name)(22050, 9, 60, 3, model_complexity=mc)
    sd = {k: v for k, v in model.state_dict().items() if not k.startswith('sliCQ.')}
    keys = [str(k) for k in g['%s_mc%d_keys' % (name, mc)]]
    assert list(sd) == keys
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in g['%s_mc%d_shapes' % (name, mc)]]
    c0 = 2 * 2 ** (mc - 1)
    assert sd['encoder.convin.0.weight'].shape == (c0, 1, 3, 3)
    assert sd['decoder.convout.weight'].shape == (1, c0, 3, 3) and sd['decoder.convout.bias'].shape == (1,)
    # the default initialisation draws from the RNG in the reference's order: the same seed gives the same weights
    for k in ('encoder.convin.0.weight', 'encoder.convin.0.bias', 'decoder.convout.weight', 'decoder.convout.bias'):
        np.testing.assert_array_equal(sd[k].numpy(), g['%s_mc%d_init.%s' % (name, mc, k)], err_msg=k)
    sums = np.array([float(v.double().sum()) for v in sd.values()])
    np.testing.assert_allclose(sums, g['%s_mc%d_init_sums' % (name, mc)], rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize('name', CLASSES)
def test_reference_shaped_state_dict_loads_strictly(golden, name):
    g = golden('variants')
    model = _cls(name)(22050, 9, 60, 3, latent_size=None, model_complexity=2)
    shapes = [eval(s) for s in g['%s_mc2_shapes' % name]]
    sd = {str(k): torch.full(s, 0.5) for k, s in zip(g['%s_mc2_keys' % name], shapes)}
    model.load_state_dict(sd, strict=True)
    assert float(model.decoder.convout.weight.detach().sum()) == 0.5 * 9 * 4


def test_variants_are_timbre_traps_and_film_still_raises():
    from timbre_trap.framework import FiLM, TimbreTrap, TimbreTrapFiLM, TimbreTrapMag, TimbreTrapMagDB
    m = TimbreTrapMagDB(22050, 9, 60, 3, model_complexity=1, skip_connections=True)
    assert isinstance(m, TimbreTrapMag) and isinstance(m, TimbreTrap) and m.skip_weights.shape == (5,)
    with pytest.raises(NotImplementedError):
        TimbreTrapFiLM(22050, 9, 60, 3)
    with pytest.raises(NotImplementedError):
        FiLM(4, 4)


def test_cpu_magnitude_and_decibels_keep_the_torch_expression():
    from timbre_trap.framework import CQT
    g = torch.Generator().manual_seed(3)
    c = torch.randn(3, 2, 7, 9, generator=g)
    c[1] = 0.0                                                   # an all-zero clip: its dB map is flat at the 1e-10 floor
    m = CQT.to_magnitude(c)
    assert torch.equal(m, c.norm(p=2, dim=-3))
    for rescale in (True, False):
        got = CQT.to_decibels(m, rescale)
        want = []
        for x in m:
            d = 20.0 * torch.log10(torch.clamp(x, min=1e-10))
            d = torch.maximum(d, d.max() - 80.0)
            if rescale:
                d = 1 + (d - d.max()) / 80
            want.append(d)
        assert torch.equal(got, torch.stack(want))
    # an input that requires grad keeps autograd on the CPU expression
    c.requires_grad_(True)
    CQT.to_decibels(CQT.to_magnitude(c)).sum().backward()
    assert c.grad is not None
