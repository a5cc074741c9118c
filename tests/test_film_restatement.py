"""CPU-only: tests/film_ref.py -- the float64 restatement the GPU tests of csrc/film.hip compare against -- is pinned to the FiLM layer
outputs recorded from the reference (tests/golden/film.npz) and to torch autograd of the reference's expression
(modules.py:880-887: ``(x.transpose(-1, -2) * gamma(condition) + beta(condition)).transpose(-1, -2)``)."""

import numpy as np
import pytest
import torch

import film_ref

CONDS = {0: (0.0, 1.0), 1: (1.0, 0.0)}                   # transcribe -> (transcribe, not transcribe)


def _fixture_params(D):
    p = film_ref.distinct_film_parameters(D)
    return [p['film_layer.%s' % k] for k in ('gamma.weight', 'gamma.bias', 'beta.weight', 'beta.bias')]


@pytest.mark.parametrize('tag,D', (('mc1', 32), ('mc2skip', 128)))
def test_forward_restatement_against_the_recorded_layer(golden, tag, D):
    g = golden('film')
    x = torch.from_numpy(g[f'{tag}_film_in'])
    assert x.shape == (2, D, 16)
    gw, gb, bw, bb = _fixture_params(D)
    for t, cond in CONDS.items():
        want = torch.from_numpy(g[f'{tag}_film_out_t{t}'])
        assert want.shape == x.shape and want.dtype == torch.float32
        got = film_ref.film_fwd(x, gw, gb, bw, bb, cond)
        G, Bt = film_ref.coefficients(gw, gb, cond)[0], film_ref.coefficients(bw, bb, cond)[0]
        # four fp32 roundings in the recorded value -- G = weight + bias, Bt likewise, the product, the sum -- and none in the
        # restatement: u (2 |x G| + |Bt| + |y|), to first order (the 1.01)
        bar = 1.01 * film_ref.U32 * (2 * (x.double() * G[:, None]).abs() + Bt[:, None].abs() + want.double().abs())
        assert bool(((got - want.double()).abs() <= bar).all())
        # what the GPU test compares the kernel with bit for bit: for a one-hot condition nn.Linear gives weight[:, k] + bias exactly,
        # and the layer is the UNFUSED fp32 expression
        k = 0 if t else 1
        G32, B32 = gw[:, k] + gb, bw[:, k] + bb
        assert torch.equal(G32, G.float()) and torch.equal(B32, Bt.float())
        assert torch.equal(x * G32[:, None] + B32[:, None], want)
    # the two conditions are recorded as different maps
    assert not np.array_equal(g[f'{tag}_film_out_t0'], g[f'{tag}_film_out_t1'])


def test_pair_form_is_the_two_single_forms():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 7, 5, generator=g)
    gw, gb, bw, bb = (torch.randn(s, generator=g) for s in ((7, 2), (7,), (7, 2), (7,)))
    pair = film_ref.film_fwd(x, gw, gb, bw, bb, (0.0, 1.0, 1.0, 0.0))
    assert pair.shape == (6, 7, 5)
    assert torch.equal(pair[:3], film_ref.film_fwd(x, gw, gb, bw, bb, (0.0, 1.0)))
    assert torch.equal(pair[3:], film_ref.film_fwd(x, gw, gb, bw, bb, (1.0, 0.0)))


@pytest.mark.parametrize('cond', ((0.0, 1.0), (1.0, 0.0), (0.3, -1.7), (0.0, 1.0, 1.0, 0.0), (0.25, 0.5, -2.0, 0.75)))
def test_restatement_against_autograd_of_the_reference_expression(cond):
    g = torch.Generator().manual_seed(len(cond) * 10 + int(cond[0] * 8))
    B, D, T = 3, 6, 11
    R = len(cond) // 2
    x = torch.randn(B, D, T, generator=g, dtype=torch.float64).requires_grad_(True)
    gamma, beta = torch.nn.Linear(2, D).double(), torch.nn.Linear(2, D).double()
    with torch.no_grad():
        for p in list(gamma.parameters()) + list(beta.parameters()):
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64))
    dy = torch.randn(R * B, D, T, generator=g, dtype=torch.float64)
    ys = []
    for r in range(R):
        c = torch.tensor(cond[2 * r: 2 * r + 2], dtype=torch.float64)
        ys.append((x.transpose(-1, -2) * gamma(c) + beta(c)).transpose(-1, -2))
    y = torch.cat(ys, dim=0)
    y.backward(dy)
    args = (gamma.weight.detach(), gamma.bias.detach(), beta.weight.detach(), beta.bias.detach())
    np.testing.assert_allclose(film_ref.film_fwd(x.detach(), *args, cond).numpy(), y.detach().numpy(), rtol=1e-13, atol=1e-13)
    got = film_ref.film_bwd(x.detach(), dy, args[0], args[1], cond)
    for name, want in (('dx', x.grad), ('dgw', gamma.weight.grad), ('dgb', gamma.bias.grad), ('dbw', beta.weight.grad),
                       ('dbb', beta.bias.grad)):
        np.testing.assert_allclose(got[name].numpy(), want.numpy(), rtol=1e-12, atol=1e-12, err_msg=name)
        if name != 'dx':
            assert bool((got['abs_' + name] >= got[name].abs() - 1e-12).all()), name


# ---- the composed CPU oracle of the model (what the GPU inference test compares with) against the recorded reference -------------------

KW = dict(mc1=dict(model_complexity=1, latent_size=32), mc2skip=dict(model_complexity=2, latent_size=128, skip_connections=True))
OUTPUTS = ('reconstruction', 'latents', 'transcription', 'transcription_rec', 'transcription_scr')


def _stub_forward(audio):
    import stub_cqt
    from oracle import nsgt
    return torch.from_numpy(nsgt.to_real(stub_cqt.stub_encode(audio, 540, 64, 16).numpy())).contiguous()


def fixture_state_dict(tag):
    from oracle import autoencoder as oae
    D = KW[tag]['latent_size']
    return film_ref.fixture_overrides(oae.closed_form_state_dict(film_ref.film_shapes(oae.state_dict_shapes(540, **KW[tag]), D)), D)


@pytest.mark.parametrize('tag', ('mc1', 'mc2skip'))
def test_composed_oracle_against_the_recorded_model(golden, tag):
    import stub_cqt
    from oracle import autoencoder as oae
    g = golden('film')
    sd = fixture_state_dict(tag)
    assert [k for k in sd if k != 'skip_weights'] == [str(k) for k in g['mc%d_keys' % KW[tag]['model_complexity']]]
    audio = stub_cqt.closed_form_audio(2, 64)
    with torch.no_grad():
        res = film_ref.oracle_forward(_stub_forward(audio), sd)
    assert film_ref.separation(res[0], res[2]) >= 10
    for name, t in zip(OUTPUTS, res):
        want = g[f'{tag}_fwd_{name}']
        got = t if want.shape == tuple(t.shape) else t[:, :, ::8, ::2]
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-4, atol=1e-4, err_msg=name)
    act = oae.to_activations(res[2])
    np.testing.assert_allclose((act[:, ::2] if tag == 'mc1' else act[:, ::8, ::2]).numpy(), g[f'{tag}_act'], rtol=1e-4, atol=1e-5)
    if tag != 'mc1':
        return
    from oracle import nsgt
    long_audio = stub_cqt.closed_form_audio(1, 160)
    chunked = film_ref.oracle_chunked(long_audio, sd, _stub_forward, 64, 16)
    for t, key in ((True, 'chunked_trn'), (False, 'chunked_rec')):
        assert chunked[t].shape == (1, 2, 540, 48)
        np.testing.assert_allclose(chunked[t][:, :, ::12].numpy(), g[f'mc1_{key}'], rtol=1e-4, atol=1e-4)
    padded = torch.from_numpy(nsgt.pad_to_block_length(long_audio.numpy(), 64))
    one = film_ref.oracle_inference(_stub_forward(padded), sd)[False]
    np.testing.assert_allclose(one[:, :, ::12].numpy(), g['mc1_inference'], rtol=1e-4, atol=1e-4)
