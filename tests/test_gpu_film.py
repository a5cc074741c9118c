"""
GPU parity of the FiLM variant TimbreTrapFiLM (reference modules.py:780-889):
  * the kernels of csrc/film.hip through the C ABI, every operand inside a NaN guard buffer: the forward and the data gradient bit for
    bit against the CPU fp32 expression (every product and sum rounded on its own), the parameter gradients against the float64
    restatement tests/film_ref.py at the bar derived there;
  * the fp32 model route against values recorded from the reference (tests/golden/film.npz), the layer alone bit for bit;
  * inference at model_complexity 2 with the real transform against the CPU oracle composed in tests/film_ref.py (itself pinned to the
    recorded values by tests/test_film_restatement.py);
  * the train step under bf16 / fp16 autocast against the same model on the exact-fp32 HIP route, with the route it takes asserted;
  * run-to-run determinism and the optimiser's flat gradient buffer.
"""

import ctypes

import numpy as np
import pytest
import torch

import film_ref
import stub_cqt
from oracle import autoencoder as oae
from oracle import nsgt

pytestmark = pytest.mark.gpu
N, M, SR = 66150, 1024, 22050
LOGIT_TOL = dict(rtol=1e-4, atol=1e-4)
KW = dict(mc1=dict(model_complexity=1, latent_size=32), mc2=dict(model_complexity=2, latent_size=128),
          mc2skip=dict(model_complexity=2, latent_size=128, skip_connections=True))
OUTPUTS = ('reconstruction', 'latents', 'transcription', 'transcription_rec', 'transcription_scr')
NAN = float('nan')


# ---- the kernels through the C ABI ---------------------------------------------------------------------------------------------------------

PAD = 64                                                  # guard floats on either side (256 bytes: the payload keeps its alignment)


class Guarded:
    """``n`` floats in the middle of a NaN-filled device buffer; ``shift`` = 1 moves the payload by 4 bytes (off the 16-byte grid)."""

    def __init__(self, n, shift=0, fill=None):
        self.buf = torch.full((n + 2 * PAD + 1,), NAN, device='cuda')
        self.lo, self.hi = PAD + shift, PAD + shift + n
        self.t = self.buf[self.lo:self.hi]
        if fill is not None:
            self.t.copy_(fill.reshape(-1))
        assert (self.t.data_ptr() % 16 == 0) == (shift == 0)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def intact(self):
        return bool(torch.isnan(self.buf[:self.lo]).all()) and bool(torch.isnan(self.buf[self.hi:]).all())


def _same(a, b):
    """Bit-level equality of two fp32 tensors, NaN = NaN."""
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _coef32(w, b, c0, c1):
    """gamma(c) / beta(c) as tt_film_fwd forms it, in CPU fp32 (torch rounds every elementwise operation on its own)."""
    return (w[:, 0] * c0 + w[:, 1] * c1) + b


def _fwd32(x, gw, gb, bw, bb, cond):
    ys = []
    for r in range(len(cond) // 2):
        G, Bt = _coef32(gw, gb, *cond[2 * r: 2 * r + 2]), _coef32(bw, bb, *cond[2 * r: 2 * r + 2])
        ys.append(x * G[:, None] + Bt[:, None])
    return torch.cat(ys, dim=0)


def _dx32(dy, gw, gb, cond, B):
    R = len(cond) // 2
    parts = [_coef32(gw, gb, *cond[2 * r: 2 * r + 2])[:, None] * dy[r * B:(r + 1) * B] for r in range(R)]
    return parts[0] if R == 1 else parts[0] + parts[1]


def _carray(cond):
    return (ctypes.c_float * 4)(*(list(cond) + [0.0] * (4 - len(cond))))


def _shapes():
    from timbre_trap import _hip
    tile = _hip.lib().tt_film_tile_frames()
    return tile, ((1, 1, 1), (3, 33, 17), (2, 128, tile + 5), (2, 144, 2 * tile + 4))


CONDS = {1: ((1.0, 0.0), (0.0, 1.0), (0.3, -1.7)), 2: ((0.0, 1.0, 1.0, 0.0), (1.0, 0.0, 0.0, 1.0), (0.25, 0.5, -2.0, 0.75))}
GRADS = ('dgw', 'dgb', 'dbw', 'dbb')


@pytest.mark.parametrize('R', (1, 2))
@pytest.mark.parametrize('case', range(4))
def test_film_kernels_through_the_c_abi(case, R):
    from timbre_trap import _hip
    lib, st = _hip.lib(), _hip.stream_ptr()
    tile, shapes = _shapes()
    B, D, T = shapes[case]
    assert tile == 1024 and lib.tt_film_scratch_bytes(B, D, T, R) == R * 2 * D * B * ((T + tile - 1) // tile) * 4
    g = torch.Generator().manual_seed(100 * case + R)
    x = torch.randn(B, D, T, generator=g)
    gw, gb, bw, bb = (torch.randn(s, generator=g) for s in ((D, 2), (D,), (D, 2), (D,)))
    dy = torch.randn(R * B, D, T, generator=g)
    xs = x.clone()                                        # the forward input: an inf and a NaN planted
    xs.view(-1)[0] = float('inf')
    xs.view(-1)[-1] = NAN
    n = B * D * T
    cu = lib.tt_set_cu_limit(0)
    try:
        for ci, cond in enumerate(CONDS[R]):
            # one pointer at a time 4 bytes off the 16-byte grid (with the first condition only), then fewer workgroups than work items
            variants = [None, 'x', 'y', 'dy', 'dx', 'fewer-workgroups'] if ci == 0 else [None]
            base = None
            for off in variants:
                lib.tt_set_cu_limit(1 if off == 'fewer-workgroups' else cu)
                sh = lambda name: int(off == name)
                # ---- forward
                gx = Guarded(n, sh('x'), xs)
                gp = [Guarded(p.numel(), 0, p) for p in (gw, gb, bw, bb)]
                gy = Guarded(R * n, sh('y'))
                _hip.check(lib.tt_film_fwd(gx.ptr, gp[0].ptr, gp[1].ptr, gp[2].ptr, gp[3].ptr, _carray(cond), gy.ptr, B, D, T, R, st), 'tt_film_fwd')
                y = gy.t.cpu().view(R * B, D, T)
                assert all(b.intact() for b in [gx, gy] + gp), (cond, off)
                assert _same(y, _fwd32(xs, gw, gb, bw, bb, cond)), (cond, off)
                if R == 2:                               # the pair form's halves are the two single calls
                    for r in range(2):
                        g1 = Guarded(n)
                        _hip.check(lib.tt_film_fwd(gx.ptr, gp[0].ptr, gp[1].ptr, gp[2].ptr, gp[3].ptr, _carray(cond[2 * r: 2 * r + 2]), g1.ptr,
                                                   B, D, T, 1, st), 'tt_film_fwd')
                        assert _same(g1.t.cpu().view(B, D, T), y[r * B:(r + 1) * B]) and g1.intact(), (cond, off, r)
                # ---- backward: dx and the four parameter gradients, accumulated onto pre-filled buffers
                gx = Guarded(n, sh('x'), x)
                gdy = Guarded(R * n, sh('dy'), dy)
                gdx = Guarded(n, sh('dx'))
                pre = [torch.randn(s, generator=torch.Generator().manual_seed(7)) for s in ((D, 2), (D,), (D, 2), (D,))]
                gg = [Guarded(p.numel(), 0, p) for p in pre]
                ws = Guarded(lib.tt_film_scratch_bytes(B, D, T, R) // 4)
                args = (gx.ptr, gdy.ptr, gp[0].ptr, gp[1].ptr, _carray(cond))
                _hip.check(lib.tt_film_bwd(*args, gdx.ptr, gg[0].ptr, gg[1].ptr, gg[2].ptr, gg[3].ptr, ws.ptr, B, D, T, R, st), 'tt_film_bwd')
                assert all(b.intact() for b in [gx, gdy, gdx, ws] + gg + gp), (cond, off)
                dx = gdx.t.cpu().view(B, D, T)
                assert _same(dx, _dx32(dy, gw, gb, cond, B)), (cond, off)
                ref = film_ref.film_bwd(x, dy, gw, gb, cond)
                got = {k: b.t.cpu().view(p.shape) for k, b, p in zip(GRADS, gg, pre)}
                for k, p in zip(GRADS, pre):
                    want = p.double() + ref[k]
                    err = (got[k].double() - want).abs()
                    bar = film_ref.gradient_bar(ref['abs_' + k] + p.double().abs(), want)
                    assert bool((err <= bar).all()), (cond, off, k, float((err / bar.clamp_min(1e-300)).max()))
                # ---- dx = NULL, gradients = NULL, a second call: the same bits
                gg2 = [Guarded(p.numel(), 0, p) for p in pre]
                _hip.check(lib.tt_film_bwd(*args, None, gg2[0].ptr, gg2[1].ptr, gg2[2].ptr, gg2[3].ptr, ws.ptr, B, D, T, R, st), 'tt_film_bwd')
                gdx2 = Guarded(n, sh('dx'))
                _hip.check(lib.tt_film_bwd(None, gdy.ptr, gp[0].ptr, gp[1].ptr, _carray(cond), gdx2.ptr, None, None, None, None, None, B, D, T, R, st),
                           'tt_film_bwd')
                gg3 = [Guarded(p.numel(), 0, p) for p in pre]
                gdx3 = Guarded(n, sh('dx'))
                _hip.check(lib.tt_film_bwd(*args, gdx3.ptr, gg3[0].ptr, gg3[1].ptr, gg3[2].ptr, gg3[3].ptr, ws.ptr, B, D, T, R, st), 'tt_film_bwd')
                assert all(b.intact() for b in [gdx2, gdx3, ws] + gg2 + gg3)
                assert torch.equal(gdx2.t.cpu().view(B, D, T), dx) and torch.equal(gdx3.t.cpu().view(B, D, T), dx)
                for k, a, b in zip(GRADS, gg2, gg3):
                    assert torch.equal(a.t.cpu().view(got[k].shape), got[k]) and torch.equal(b.t.cpu().view(got[k].shape), got[k]), (cond, off, k)
                # the scalar path and the grid walk give the vector path's bits, gradients included
                if base is None:
                    base = (y, dx, got)
                else:
                    assert _same(y, base[0]) and torch.equal(dx, base[1]) and all(torch.equal(got[k], base[2][k]) for k in GRADS), (cond, off)
    finally:
        lib.tt_set_cu_limit(cu)
    # half-given gradients and bad sizes are refused before anything is launched
    z = Guarded(4)
    assert lib.tt_film_bwd(z.ptr, z.ptr, z.ptr, z.ptr, _carray((1.0, 0.0)), z.ptr, z.ptr, None, None, None, z.ptr, 1, 1, 1, 1, st) == -1
    assert lib.tt_film_fwd(z.ptr, z.ptr, z.ptr, z.ptr, z.ptr, _carray((1.0, 0.0)), z.ptr, 1, 1, 1, 3, st) == -1
    assert lib.tt_film_scratch_bytes(1, 1, 0, 1) == 0


def test_film_function_gradients_and_frozen_parameters():
    """ops.FilmFn: leading dimensions beyond (B, D, T), autograd against the float64 restatement, ctx.needs_input_grad deciding which
    pointers are NULL, a frozen parameter getting no gradient."""
    from timbre_trap.framework import FiLM
    g = torch.Generator().manual_seed(11)
    f = FiLM(6, 2).cuda()
    x = torch.randn(2, 3, 6, 9, generator=g).cuda().requires_grad_(True)
    dy = torch.randn(2, 3, 6, 9, generator=g).cuda()
    y = f(x, [0.0, 1.0])
    assert y.shape == x.shape
    y.backward(dy)
    P = [p.detach().cpu() for p in (f.gamma.weight, f.gamma.bias, f.beta.weight, f.beta.bias)]
    ref = film_ref.film_bwd(x.detach().cpu().reshape(6, 6, 9), dy.cpu().reshape(6, 6, 9), P[0], P[1], (0.0, 1.0))
    assert torch.equal(y.detach().cpu(), _fwd32(x.detach().cpu().reshape(6, 6, 9), *P, (0.0, 1.0)).view(2, 3, 6, 9))
    assert torch.equal(x.grad.cpu().reshape(6, 6, 9), _dx32(dy.cpu().reshape(6, 6, 9), P[0], P[1], (0.0, 1.0), 6))
    for k, p in zip(GRADS, (f.gamma.weight, f.gamma.bias, f.beta.weight, f.beta.bias)):
        assert bool(((p.grad.cpu().double() - ref[k]).abs() <= film_ref.gradient_bar(ref['abs_' + k], ref[k])).all()), k
    # no input gradient wanted; one parameter frozen
    f.zero_grad()
    f.beta.bias.requires_grad_(False)
    f(x.detach(), torch.tensor([0.0, 1.0])).backward(dy)                 # (a CPU tensor condition: read by value)
    assert f.beta.bias.grad is None and bool(((f.gamma.weight.grad.cpu().double() - ref['dgw']).abs()
                                              <= film_ref.gradient_bar(ref['abs_dgw'], ref['dgw'])).all())
    # nothing but the input wants a gradient
    for p in f.parameters():
        p.requires_grad_(False)
    x.grad = None
    f(x, torch.tensor([0.0, 1.0], device='cuda')).backward(dy)           # (a device tensor condition: one .tolist())
    assert torch.equal(x.grad.cpu().reshape(6, 6, 9), _dx32(dy.cpu().reshape(6, 6, 9), P[0], P[1], (0.0, 1.0), 6))
    with pytest.raises(ValueError):
        f(x, (1.0, 0.0, 0.0))


# ---- the fp32 model route against the recorded reference ----------------------------------------------------------------------------------

def _fixture_sd(tag):
    D = KW[tag]['latent_size']
    return film_ref.fixture_overrides(oae.closed_form_state_dict(film_ref.film_shapes(oae.state_dict_shapes(540, **KW[tag]), D)), D)


def _model(kw, sd=None):
    from timbre_trap.framework import TimbreTrapFiLM
    m = TimbreTrapFiLM(SR, 9, 60, 3, **kw)
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    return m.cuda()


class _coefficients_for_audio:
    """``with _coefficients_for_audio(model, c):`` -- model.sliCQ(audio) returns ``c`` (the transform is pinned on its own)."""

    def __init__(self, model, c):
        self.cqt, self.c = model.sliCQ, c

    def __enter__(self):
        self.cqt.forward = lambda audio: self.c
        return self

    def __exit__(self, *exc):
        del self.cqt.forward
        return False


def _check_outputs(g, tag, res):
    for name, t in zip(OUTPUTS, res):
        want = g[f'{tag}_fwd_{name}']
        t = t.detach().cpu()
        got = t if want.shape == tuple(t.shape) else t[:, :, ::8, ::2]       # (mc2skip: every 8th bin and 2nd frame are recorded)
        np.testing.assert_allclose(got.numpy(), want, err_msg=name, **LOGIT_TOL)
        # ... and the L2 norm of the whole tensor: | ||a|| - ||b|| | <= ||a - b|| <= sqrt(n) atol + rtol ||b||
        norm = float(g[f'{tag}_fwdstat_{name}'][1])
        assert abs(float(t.double().norm()) - norm) <= LOGIT_TOL['atol'] * t.numel() ** 0.5 + LOGIT_TOL['rtol'] * norm, name


@pytest.mark.parametrize('tag', ('mc1', 'mc2skip'))
def test_film_forward_losses_gradients_golden(golden, tag):
    """model.forward (consistency) + the train.py losses + gradients on the fp32 route, the layer alone bit for bit, and the no-grad
    forward, against the reference on closed-form weights whose two conditions differ by >= 10 tolerances."""
    from timbre_trap.framework import compute_consistency_loss, compute_reconstruction_loss, compute_transcription_loss
    g = golden('film')
    assert float(g[f'{tag}_separation']) >= 10
    model = _model(KW[tag], _fixture_sd(tag))
    audio = stub_cqt.closed_form_audio(2, 64)
    coeffs = torch.from_numpy(nsgt.to_real(stub_cqt.stub_encode(audio, 540, 64, 16).numpy())).contiguous().cuda()
    dummy = torch.zeros(2, 1, 8, device='cuda')
    with _coefficients_for_audio(model, coeffs):
        rec, latents, trn, trn_rec, trn_scr, losses = model(dummy, True)
    assert losses == {} and rec.shape == (2, 2, 540, 16)
    _check_outputs(g, tag, (rec, latents, trn, trn_rec, trn_scr))
    act = model.to_activations(trn)
    np.testing.assert_allclose((act[:, ::2] if tag == 'mc1' else act[:, ::8, ::2]).detach().cpu().numpy(), g[f'{tag}_act'], rtol=1e-4, atol=1e-5)
    gt = stub_cqt.closed_form_targets(2, 540, 16).cuda()
    l_rec = compute_reconstruction_loss(rec, coeffs)
    l_trn = compute_transcription_loss(act, gt, True)
    l_sp, l_sc = compute_consistency_loss(trn_rec, trn_scr, trn)
    total = l_rec + l_trn + (l_sp + l_sc)
    np.testing.assert_allclose([float(v.detach()) for v in (l_rec, l_trn, l_sp, l_sc, total)], g[f'{tag}_losses'], rtol=1e-4)
    model.zero_grad()
    total.backward()
    full = 0
    for k, p in model.named_parameters():
        if f'{tag}_grad.{k}' in g.files:
            ref = g[f'{tag}_grad.{k}']
            np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=5e-3, atol=5e-4 * float(np.abs(ref).max() + 1e-6), err_msg=k)
            full += 1
        else:
            st = g[f'{tag}_gradstat.{k}']
            gg = p.grad.double().flatten().cpu()
            np.testing.assert_allclose(float(gg.norm()), st[1], rtol=2e-3, atol=1e-12, err_msg=k)
            np.testing.assert_allclose(gg[:6].numpy(), st[2:], rtol=1e-2, atol=2e-3 * st[1] + 1e-12, err_msg=k)
    assert full == 5                                       # film_layer.* and decoder.convin.0.bias are recorded in full
    # the layer alone: the recorded bits, whichever way the condition arrives
    x = torch.from_numpy(g[f'{tag}_film_in']).cuda()
    with torch.no_grad():
        for t in (False, True):
            want = torch.from_numpy(g[f'{tag}_film_out_t{int(t)}'])
            for cond in ((t, not t), torch.tensor([t, not t], dtype=torch.float32), torch.tensor([t, not t], dtype=torch.float32, device='cuda')):
                assert torch.equal(model.film_layer(x, cond).cpu(), want), (t, type(cond))
    # the route evaluate() takes: no grad, two decodes
    with torch.no_grad(), _coefficients_for_audio(model, coeffs):
        res = model(dummy, True)
    _check_outputs(g, tag, res[:5])


def test_film_inference_vs_composed_oracle():
    """chunked_inference for both switches, transcribe and inference at mc 2 / latent 128, one clip of one block, real transform (its
    coefficients taken from the HIP CQT, pinned on its own), against the oracle composed per chunk: 1e-4 of the maximum."""
    D = KW['mc2']['latent_size']
    sd = film_ref.fixture_overrides(oae.closed_form_state_dict(film_ref.film_shapes(oae.state_dict_shapes(540, **KW['mc2']), D)), D)
    model = _model(KW['mc2'], sd).eval()
    audio = torch.rand(1, 1, N, generator=torch.Generator().manual_seed(21)) * 2 - 1
    a = audio.cuda()
    trn = model.chunked_inference(a, True)
    rec = model.chunked_inference(a, False)
    assert trn.shape == rec.shape == (1, 2, 540, M)
    want = film_ref.oracle_chunked(audio, sd, lambda chunk: model.sliCQ(chunk.cuda()).cpu(), N, M)
    assert film_ref.separation(want[False], want[True]) >= 10          # a swapped or ignored condition cannot pass

    def rel(got, w):
        return float((got.cpu() - w).abs().max() / w.abs().max())
    for t, got in ((True, trn), (False, rec)):
        assert rel(got, want[t]) < 1e-4, (t, rel(got, want[t]))
    act = model.transcribe(a)
    assert act.shape == (1, 540, M)
    assert float((act.cpu() - oae.to_activations(want[True])).abs().max()) < 1e-4
    one = model.inference(a, True)
    want_one = film_ref.oracle_inference(model.sliCQ(a).cpu(), sd, (True,))[True]
    assert one.shape == (1, 2, 540, M) and rel(one, want_one) < 1e-4, rel(one, want_one)


# ---- the train step under autocast ---------------------------------------------------------------------------------------------------------

def _count(monkeypatch, cls, calls):
    orig = cls.apply
    monkeypatch.setattr(cls, 'apply', staticmethod(lambda *a: (calls.append((cls.__name__, a)), orig(*a))[1]))


def _bench_style_targets(n, n_bins, T, seed=4321):
    """Targets as bench.py draws them: Bernoulli(0.01) seeds blurred along frequency, seeds exactly 1, one frame without positives."""
    g2 = torch.Generator().manual_seed(seed)
    seeds = (torch.rand(n, n_bins, T, generator=g2) < 0.01).float()
    k = torch.exp(-0.5 * torch.arange(-4, 5, dtype=torch.float32) ** 2).view(1, 1, 9)
    blurred = torch.nn.functional.conv1d(seeds.permute(0, 2, 1).reshape(-1, 1, n_bins), k, padding=4)
    blurred = blurred.reshape(n, T, n_bins).permute(0, 2, 1)
    target = torch.maximum(blurred.clamp(0, 1), seeds).contiguous()
    target[:, :, 0] = 0.0
    return target


def _step(model, c, gt, dtype, zero=None):
    from timbre_trap.framework import compute_consistency_loss, compute_reconstruction_loss, compute_transcription_loss
    with _coefficients_for_audio(model, c), torch.autocast(device_type='cuda', dtype=dtype or torch.bfloat16, enabled=dtype is not None):
        rec, latents, trn, trn_rec, trn_scr, _ = model(torch.zeros(2, 1, 8, device='cuda'), True)
        l_sp, l_sc = compute_consistency_loss(trn_rec, trn_scr, trn)
        total = compute_reconstruction_loss(rec, c) + compute_transcription_loss(model.to_activations(trn), gt, True) + (l_sp + l_sc)
        (zero or model.zero_grad)()
        total.backward()
    torch.cuda.synchronize()
    return ([t.detach().float().clone() for t in (rec, latents, trn, trn_rec, trn_scr)],
            {k: p.grad.detach().double().clone() for k, p in model.named_parameters()})


def _inputs(T=256):
    g = torch.Generator().manual_seed(77)
    return (torch.randn(2, 2, 540, T, generator=g) * 0.5).cuda(), _bench_style_targets(2, 540, T).cuda()


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-300))


def _bias_like(k):
    # a film_layer entry is a sum over all B x T positions, like a bias gradient
    return k.endswith('.bias') or k.startswith('film_layer.')


@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float16), ids=('bf16', 'fp16'))
def test_film_autocast_step_against_the_fp32_route(monkeypatch, dtype):
    """model(audio, True) + the three losses + backward under autocast at mc 2 / latent 128 (default initialisation, two clips, T = 256,
    white-noise coefficients) against the same model on the exact-fp32 HIP route: outputs 3e-2 of their maximum, gradients relative L2
    5e-2 (biases and film_layer.* 8e-2), cosine >= 0.998; the route -- FilmFn in its pair form once per decode_pair, ConvOut16PairFn
    twice, no ConvFn, no LatentDecodeFn, no torch.cat inside decode_pair; and with PAIR_DECODE off the same values within the
    switch-to-switch bars (outputs 1e-2, gradients 4e-2 / 8e-2)."""
    from timbre_trap.framework import TimbreTrap, ops
    torch.manual_seed(2)
    model = _model(KW['mc2'])
    c, gt = _inputs()
    ref_outs, ref = _step(model, c, gt, None)
    calls, cats, inside = [], [], []
    for cls in (ops.FilmFn, ops.ConvOut16PairFn, ops.ConvFn, ops.LatentDecodeFn, ops.LatDec16Fn):
        _count(monkeypatch, cls, calls)
    cat, pair = torch.cat, type(model).decode_pair
    monkeypatch.setattr(torch, 'cat', lambda *a, **k: (cats.append(1) if inside else None, cat(*a, **k))[1])

    def decode_pair(self, *a, **k):
        inside.append(1)
        try:
            return pair(self, *a, **k)
        finally:
            inside.pop()
    monkeypatch.setattr(type(model), 'decode_pair', decode_pair)
    outs, grads = _step(model, c, gt, dtype)
    names = [n for n, _ in calls]
    film = [a for n, a in calls if n == 'FilmFn']
    assert len(film) == 2 and all(a[6] == 2 and tuple(a[5]) == (0.0, 1.0, 1.0, 0.0) for a in film), [(a[5], a[6]) for a in film]
    assert names.count('ConvOut16PairFn') == 2 and names.count('LatDec16Fn') == 2
    assert names.count('ConvFn') == 0 and names.count('LatentDecodeFn') == 0 and not cats
    for nm, a, b in zip(OUTPUTS, outs, ref_outs):
        assert float((a - b).abs().max() / b.abs().max()) < 3e-2, nm
    stats = sorted(((_rel(grads[k], want), k) for k, want in ref.items()), reverse=True)
    print('%s: gradient relative L2 worst %.3e (%s), film_layer: %s' % (dtype, stats[0][0], stats[0][1],
                                                                       {k[11:]: '%.2e' % r for r, k in stats if k.startswith('film_layer.')}))
    for k, want in ref.items():
        cos = float(torch.dot(grads[k].flatten(), want.flatten()) / (grads[k].norm() * want.norm() + 1e-300))
        assert _rel(grads[k], want) <= (8e-2 if _bias_like(k) else 5e-2) and cos >= 0.998, (k, _rel(grads[k], want), cos)
    assert all(float(ref[k].norm()) > 0 for k in ref if k.startswith('film_layer.'))
    # two decodes instead of the pair
    monkeypatch.setattr(TimbreTrap, 'PAIR_DECODE', False)
    del calls[:]
    outs2, grads2 = _step(model, c, gt, dtype)
    film = [a for n, a in calls if n == 'FilmFn']
    assert len(film) == 4 and all(a[6] == 1 for a in film) and [n for n, _ in calls].count('ConvOut16PairFn') == 0
    for nm, a, b in zip(OUTPUTS, outs2, outs):
        assert float((a - b).abs().max() / b.abs().max()) < 1e-2, nm
    for k in ref:
        assert _rel(grads2[k], grads[k]) <= (8e-2 if _bias_like(k) else 4e-2), (k, _rel(grads2[k], grads[k]))


def test_film_bf16_step_is_bit_reproducible_and_feeds_the_fused_optimiser():
    """Two bf16 train steps from the same state give bit-identical flat gradients; the film_layer gradients are views of FusedAdamW's
    flat buffer, filled by the kernels' own +=, and one optimiser step changes the four tensors."""
    from timbre_trap.utils import FusedAdamW
    torch.manual_seed(3)
    model = _model(KW['mc2'])
    opt = FusedAdamW(model.parameters(), lr=1e-3, max_norm=10.0)
    c, gt = _inputs()
    flats = []
    for _ in range(2):
        _step(model, c, gt, torch.bfloat16, zero=opt.zero_grad)
        flats.append(opt.flat_grad.clone())
    assert torch.equal(flats[0], flats[1])
    lo, hi = opt.flat_grad.data_ptr(), opt.flat_grad.data_ptr() + 4 * opt.flat_grad.numel()
    film = dict(model.film_layer.named_parameters())
    assert sorted(film) == ['beta.bias', 'beta.weight', 'gamma.bias', 'gamma.weight']
    for k, p in film.items():
        assert lo <= p.grad.data_ptr() < hi and float(p.grad.abs().sum()) > 0, k
    before = {k: p.detach().clone() for k, p in film.items()}
    opt.step()
    torch.cuda.synchronize()
    for k, p in film.items():
        assert not torch.equal(p.detach(), before[k]), k
