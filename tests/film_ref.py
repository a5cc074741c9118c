"""
Float64 restatement of the FiLM layer of TimbreTrapFiLM (reference modules.py:847-889) over the arguments of tt_film_fwd / tt_film_bwd
(include/ttrap.h), pinned to values recorded from the reference and to torch autograd by tests/test_film_restatement.py; plus the
closed-form FiLM parameters and state dict that tests/golden/make_golden_film.py records its fixtures with.

    x (B, D, T), gw / bw (D, 2), gb / bb (D), cond: R x 2 values c_r = (c_r0, c_r1)
    G_r = gw[:, 0] c_r0 + gw[:, 1] c_r1 + gb      Bt_r likewise      y[r B + b] = x[b] G_r[:, None] + Bt_r[:, None]
"""

import math

import torch

F64 = torch.float64


def _cond(cond):
    c = torch.as_tensor(cond, dtype=F64).reshape(-1, 2)
    assert c.size(0) in (1, 2)
    return c


def coefficients(w, b, cond):
    """(R, D): gamma(c_r) or beta(c_r) of nn.Linear(2, D) with weight w (D, 2) and bias b (D)."""
    return _cond(cond) @ w.to(F64).t() + b.to(F64)


def film_fwd(x, gw, gb, bw, bb, cond):
    """y (R B, D, T) float64."""
    G, Bt = coefficients(gw, gb, cond), coefficients(bw, bb, cond)
    x = x.to(F64)
    return torch.cat([x * G[r][:, None] + Bt[r][:, None] for r in range(G.size(0))], dim=0)


def film_bwd(x, dy, gw, gb, cond):
    """dy (R B, D, T) -> dict of float64 gradients dx (B, D, T), dgw (D, 2), dgb (D), dbw (D, 2), dbb (D), and under 'abs_' + name the
    same sums over the ABSOLUTE values of their terms (what a rounding-error bar of a sum scales with)."""
    c = _cond(cond)
    R = c.size(0)
    G = coefficients(gw, gb, cond)
    x = x.to(F64)
    B = x.size(0)
    dy = dy.to(F64).reshape(R, B, x.size(1), x.size(2))
    out = dict(dx=sum(G[r][:, None] * dy[r] for r in range(R)))
    for tag, fn in (('', lambda t: t), ('abs_', torch.abs)):
        P = torch.stack([fn(x * dy[r]).sum(dim=(0, 2)) for r in range(R)])           # (R, D)
        S = torch.stack([fn(dy[r]).sum(dim=(0, 2)) for r in range(R)])
        cc = fn(c)
        out[tag + 'dgw'] = torch.einsum('rj,rd->dj', cc, P)
        out[tag + 'dgb'] = P.sum(dim=0)
        out[tag + 'dbw'] = torch.einsum('rj,rd->dj', cc, S)
        out[tag + 'dbb'] = S.sum(dim=0)
    return out


def distinct_film_parameters(D):
    """FiLM parameters under which the two conditions give clearly different maps (the closed-form weights of the other layers give
    gamma / beta columns that differ by ~1e-5 of the output: a swapped condition would pass a 1e-4 test)."""
    d = torch.arange(D, dtype=F64)
    k = torch.arange(2, dtype=F64)
    i = 2 * d[:, None] + k[None, :]
    return {'film_layer.gamma.weight': (0.6 * torch.sin(0.37 * i + 0.11)).float(),
            'film_layer.gamma.bias': (1 + 0.25 * torch.sin(0.91 * d)).float(),
            'film_layer.beta.weight': (2.0 * torch.sin(0.53 * i + 1.3)).float(),
            'film_layer.beta.bias': (0.1 * torch.sin(0.29 * d + 0.7)).float()}


def film_shapes(shapes, latent_size):
    """The state-dict shapes of TimbreTrapFiLM from those of TimbreTrap (same registration order: Decoder.convin without the indicator
    channel, the FiLM layer's four entries last)."""
    shapes = dict(shapes)
    w = shapes['decoder.convin.0.weight']
    assert w[0] == latent_size + 1
    shapes['decoder.convin.0.weight'] = (latent_size,) + tuple(w[1:])
    for name in ('gamma', 'beta'):
        shapes['film_layer.%s.weight' % name] = (latent_size, 2)
        shapes['film_layer.%s.bias' % name] = (latent_size,)
    return shapes


def fixture_overrides(sd, latent_size):
    """What the fixtures change in a closed-form state dict ``sd`` of TimbreTrapFiLM (in place): the FiLM parameters above, and
    Decoder.convin's weight x 30 so that the latents' share of the output is visible."""
    sd.update(distinct_film_parameters(latent_size))
    sd['decoder.convin.0.weight'] = sd['decoder.convin.0.weight'] * 30
    return sd


def separation(rec, trn, rtol=1e-4, atol=1e-4):
    """max |rec - trn| in units of the tolerance a comparison of either against its recorded value uses: the fixtures assert >= 10."""
    return float((rec - trn).abs().max()) / (atol + rtol * float(rec.abs().max()))


# ---- the CPU oracle of TimbreTrapFiLM, composed from oracle.autoencoder's shape-generic functions and the layer in torch ---------------

def oracle_film(latents, sd, transcribe):
    """FiLM.forward as the reference writes it (modules.py:880-887), on the state dict ``sd``."""
    import torch.nn.functional as Fn
    c = torch.tensor([transcribe, not transcribe], dtype=latents.dtype)
    gamma = Fn.linear(c, sd['film_layer.gamma.weight'], sd['film_layer.gamma.bias'])
    beta = Fn.linear(c, sd['film_layer.beta.weight'], sd['film_layer.beta.bias'])
    return (latents.transpose(-1, -2) * gamma + beta).transpose(-1, -2)


def oracle_decode(latents, sd, embeddings=None, transcribe=False):
    """TimbreTrapFiLM.decode (modules.py:814-844)."""
    from oracle import autoencoder as oae
    return oae.decoder_forward(oracle_film(latents, sd, transcribe), sd, embeddings)


def oracle_forward(coefficients, sd, consistency=True):
    """TimbreTrap.forward (modules.py:338-393) with TimbreTrapFiLM's decode, behind the transform."""
    from oracle import autoencoder as oae
    latents, emb = oae.encoder_forward(coefficients, sd)
    emb = oae.apply_skip_connections(emb, sd)
    rec, trn = oracle_decode(latents, sd, emb, False), oracle_decode(latents, sd, emb, True)
    trn_rec = trn_scr = None
    if consistency:
        lat2, emb2 = oae.encoder_forward(trn, sd)
        emb2 = oae.apply_skip_connections(emb2, sd)
        trn_rec, trn_scr = oracle_decode(lat2, sd, emb2, False), oracle_decode(lat2, sd, emb2, True)
    return rec, latents, trn, trn_rec, trn_scr


def oracle_inference(coefficients, sd, switches=(False,)):
    """{transcribe: TimbreTrapFiLM.inference behind the transform} (modules.py:149-177), one encoder pass for all switches."""
    from oracle import autoencoder as oae
    with torch.no_grad():
        latents, emb = oae.encoder_forward(coefficients, sd)
        emb = oae.apply_skip_connections(emb, sd)
        return {t: oracle_decode(latents, sd, emb, t) for t in switches}


def oracle_chunked(audio, sd, cqt_forward, block_length, M, switches=(True, False)):
    """{transcribe: chunked_inference} (modules.py:204-269): 50 %-overlapping blocks, Hann cross-fade, ascending accumulation."""
    import torch.nn.functional as Fn
    audio = Fn.pad(audio, (0, -audio.size(-1) % block_length))
    hop = block_length // 2
    audio = Fn.pad(audio, [hop] * 2)
    n_chunks = (audio.size(-1) - hop) // hop
    window = torch.signal.windows.hann(M, dtype=torch.float32)
    n_frames = math.ceil((audio.size(-1) / block_length) * M)
    out = {t: torch.zeros((audio.size(0), 2, 540, n_frames)) for t in switches}
    for i in range(n_chunks):
        o = oracle_inference(cqt_forward(audio[..., i * hop: i * hop + block_length]), sd, switches)
        for t in switches:
            out[t][..., i * M // 2: i * M // 2 + M] += window * o[t]
    return {t: v[..., M // 2: -M // 2] for t, v in out.items()}


# unit round-off of fp32, and the bar of tests/test_gpu_film.py for a parameter gradient: one product rounding, a serial run of at most
# 32 terms, at most 26 pairwise levels (2^26 partial sums is beyond any tensor the kernels index), the final += -- 64 u in all on the
# sum of the terms' magnitudes, plus two roundings of the result itself
U32 = 2.0 ** -24


def gradient_bar(abs_terms, result):
    return 64 * U32 * abs_terms + 2 * U32 * result.abs()

