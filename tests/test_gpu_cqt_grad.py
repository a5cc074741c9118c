"""
Gradients of the constant-Q transform (tt_cqt_forward_bwd / tt_cqt_inverse_bwd / tt_cqt_forward_mag_bwd and their any-length twins, and
the autograd surface of timbre_trap.framework.CQT on top of them) against float64.

References, cases, bars and the constants K live in tests/cqt_grad_ref.py; tests/test_cqt_grad_restatement.py (CPU) checks them.  The
analysis gradient is held per block at K (N / 2M) decode_bar(g, adj, stages), the synthesis gradient per bin at K (2M / N) encode_bar(y,
adj, stages), ``adj`` the tables with window and dual exchanged and ``stages`` from nsgt_error.fft_stages.  Shapes: the specialised path
(N = 66150) at 2 clips x 2 blocks with every block different (the q -> (clip, block) map and the frame offset blk * M), the any-length
path at CQT(9, 60, 22050, 0.5) (N = 11025, M = 128, odd N) at the same 2 x 2, and N = 66150 forced onto the any-length kernels with one
clip per case on the edge cases.  Every check prints its ratio to the bar (pytest -rP).

The kernels' worst ratios, measured on an MI355X, in units of the bar (K = 1; N = 66150 / N = 11025 / N = 66150 forced onto the
any-length kernels; autograd and the direct C calls, planes and complex, agree bit for bit):
    analysis gradient    random 0.344 / 0.222, l2 0.437 / 0.234, single 2.227 / 0.569 / 1.287
    synthesis gradient   noise 0.331 / 0.220, impulses 0.316 / 0.318 / 0.244, dc_nyquist 0.577 / 1.036, tones 1.518 / 0.485 / 0.851
    magnitude gradient   fused 0.489, composed 0.464, fused against composed 0.488 / any-length (composed) 0.259
    through the model    waveform term: worst excess over the rtol part 0.54 of the atol part; bf16 flat-gradient cosine 1.00000
"""

import ctypes
import functools

import numpy as np
import pytest
import torch

import cqt_grad_ref as R
from oracle import autoencoder as oae
from oracle import nsgt
from oracle import objectives as oobj

pytestmark = pytest.mark.gpu
N, N_SMALL = R.N_FAST, R.N_SMALL

_worst = {}


def _note(key, ratio, k):
    _worst[key] = max(_worst.get(key, 0.0), ratio)
    print('ratio to bar: %-52s %.3f (worst so far %.3f, K %.2f)' % (key, ratio, _worst[key], k))


@pytest.fixture(scope='module')
def cqs():
    """'fast': the specialised kernels; 'small': the short odd block length only the any-length kernels serve; 'forced': N = 66150 on the
    any-length kernels"""
    from timbre_trap.framework import CQT, cqtwrapper
    mp = pytest.MonkeyPatch()
    mp.setattr(cqtwrapper, 'FORCE_GENERIC', True)
    try:
        forced = CQT(9, 60, R.SR, 3).to('cuda')
    finally:
        mp.undo()
    fast, small = CQT(9, 60, R.SR, 3).to('cuda'), CQT(9, 60, R.SR, 0.5).to('cuda')
    assert fast._fast and not forced._fast and not small._fast
    assert (forced.block_length, small.block_length, small.max_window_length) == (N, N_SMALL, 128)
    return dict(fast=fast, small=small, forced=forced)


def _n(path):
    return N_SMALL if path == 'small' else N


def _planes(c):
    return torch.stack([c[:, 0].real, c[:, 0].imag], 1).contiguous()


def _complex(p):
    return torch.complex(p[:, 0], p[:, 1])[:, None]


# ---- the C entries, called directly ---------------------------------------------------------------------------------------------------------

def _c_analysis_bwd(cq, g):
    """tt_cqt_forward_bwd / tt_cqt_generic_forward_bwd on g: contiguous complex64 (B, 1, F, T) or float32 planes (B, 2, F, T)"""
    from timbre_trap import _hip
    lib, ps = _hip.lib(), cq._plan_struct(g.device)
    B, nblk = g.size(0), g.size(-1) // cq.max_window_length
    src = torch.view_as_real(g) if g.is_complex() else g
    assert src.is_contiguous() and src.dtype == torch.float32
    out = torch.empty((B, 1, nblk * cq.block_length), dtype=torch.float32, device=g.device)
    scratch = cq._scratch(lib, ps, B * nblk, g.device)
    entry = lib.tt_cqt_forward_bwd if cq._fast else lib.tt_cqt_generic_forward_bwd
    _hip.check(entry(ctypes.byref(ps), _hip.ptr(src), _hip.ptr(out), _hip.ptr(scratch), B, nblk, int(g.is_complex()), _hip.stream_ptr()))
    return out


def _c_synthesis_bwd(cq, y, complex_out):
    from timbre_trap import _hip
    lib, ps = _hip.lib(), cq._plan_struct(y.device)
    B, nblk = y.size(0), y.size(-1) // cq.block_length
    T = nblk * cq.max_window_length
    assert y.is_contiguous() and y.dtype == torch.float32
    out = torch.empty((B, 1, cq.n_bins, T, 2) if complex_out else (B, 2, cq.n_bins, T), dtype=torch.float32, device=y.device)
    scratch = cq._scratch(lib, ps, B * nblk, y.device)
    entry = lib.tt_cqt_inverse_bwd if cq._fast else lib.tt_cqt_generic_inverse_bwd
    _hip.check(entry(ctypes.byref(ps), _hip.ptr(y), _hip.ptr(out), _hip.ptr(scratch), B, nblk, int(complex_out), _hip.stream_ptr()))
    return torch.view_as_complex(out) if complex_out else out


def _c_magnitude_bwd(cq, audio, dmag):
    from timbre_trap import _hip
    lib, ps = _hip.lib(), cq._plan_struct(audio.device)
    B, nblk = audio.size(0), audio.size(-1) // cq.block_length
    assert audio.is_contiguous() and dmag.is_contiguous()
    out = torch.empty_like(audio)
    scratch = cq._scratch(lib, ps, B * nblk, audio.device)
    _hip.check(lib.tt_cqt_forward_mag_bwd(ctypes.byref(ps), _hip.ptr(audio), _hip.ptr(dmag), _hip.ptr(out), _hip.ptr(scratch), B, nblk,
                                          _hip.stream_ptr()))
    return out


# ---- through autograd -----------------------------------------------------------------------------------------------------------------------

def _grad_encode(cq, g):
    """gradient w.r.t. the audio of encode for the complex grad_output g (the transform is linear: the audio's values do not matter)"""
    x = torch.zeros((g.size(0), 1, g.size(-1) // cq.max_window_length * cq.block_length), device='cuda', requires_grad=True)
    c = cq.encode(x)
    assert c.dtype == torch.complex64 and c.grad_fn is not None
    return torch.autograd.grad(c, x, g)[0]


def _grad_analyze(cq, gp):
    x = torch.zeros((gp.size(0), 1, gp.size(-1) // cq.max_window_length * cq.block_length), device='cuda', requires_grad=True)
    p = cq.analyze(x)
    assert p.dtype == torch.float32 and p.is_contiguous() and p.size(1) == 2 and p.grad_fn is not None
    return torch.autograd.grad(p, x, gp)[0]


def _grad_synthesize(cq, y, complex_in):
    T = y.size(-1) // cq.block_length * cq.max_window_length
    if complex_in:
        c = torch.zeros((y.size(0), 1, cq.n_bins, T), dtype=torch.complex64, device='cuda', requires_grad=True)
    else:
        c = torch.zeros((y.size(0), 2, cq.n_bins, T), device='cuda', requires_grad=True)
    a = cq.synthesize(c)
    assert a.shape == y.shape and a.grad_fn is not None
    d = torch.autograd.grad(a, c, y)[0]
    assert d.shape == c.shape and d.dtype == c.dtype
    return d


# ---- analysis gradient -------------------------------------------------------------------------------------------------------------------------

def _check_analysis(cq, family, n, generic, clips=2, tag=''):
    g_np, ref = R.analysis_case(family, n, clips)
    bar = R.analysis_bar(family, n, generic, clips)
    k = R.K_ANALYSIS[family][0]
    g = torch.tensor(g_np).cuda()
    gp = _planes(g)
    routes = dict(encode=_grad_encode(cq, g), analyze=_grad_analyze(cq, gp), c_complex=_c_analysis_bwd(cq, g), c_planes=_c_analysis_bwd(cq, gp))
    for route, got in routes.items():
        got = got.cpu().numpy()
        assert got.shape == ref.shape and np.isfinite(got).all()
        r = R.analysis_ratio(got, ref, bar)
        _note('analysis gradient %s%s %s' % (tag, family, route), r, k)
        assert r <= k, (route, r, k)
    assert torch.equal(routes['encode'], routes['c_complex']) and torch.equal(routes['analyze'], routes['c_planes'])
    return routes['c_complex'].cpu().numpy()


@pytest.mark.parametrize('family', ['random', 'l2', 'single'])
@pytest.mark.parametrize('path', ['fast', 'small'])
def test_analysis_gradient(cqs, path, family):
    n = _n(path)
    got = _check_analysis(cqs[path], family, n, path != 'fast')
    if family == 'single':
        # one non-zero coefficient in the second block of the second clip of each case: every other block is exactly zero
        blocks = got.reshape(R.N_SINGLE, 2, 2, n)
        for i in range(R.N_SINGLE):
            assert blocks[i, 1, 1].any() and not blocks[i, 0].any() and not blocks[i, 1, 0].any(), i


def test_analysis_gradient_forced_generic_edge_cases(cqs):
    got = _check_analysis(cqs['forced'], 'single', N, True, clips=1, tag='forced ')
    blocks = got.reshape(R.N_SINGLE, 2, N)
    assert all(blocks[i, 1].any() and not blocks[i, 0].any() for i in range(R.N_SINGLE))


# ---- synthesis gradient ------------------------------------------------------------------------------------------------------------------------

def _check_synthesis(cq, family, n, generic, tag=''):
    y_np, ref = R.synthesis_case(family, n)
    bar = R.synthesis_bar(family, n, generic)
    k = R.K_SYNTHESIS[family][0]
    y = torch.tensor(y_np).cuda()
    routes = dict(synthesize_complex=_grad_synthesize(cq, y, True), synthesize_planes=_complex(_grad_synthesize(cq, y, False)),
                  c_complex=_c_synthesis_bwd(cq, y, True), c_planes=_complex(_c_synthesis_bwd(cq, y, False)))
    for route, got in routes.items():
        got = got.cpu().numpy()
        assert got.shape == ref.shape and np.isfinite(got.real).all() and np.isfinite(got.imag).all()
        r = R.synthesis_ratio(got, ref, bar)
        _note('synthesis gradient %s%s %s' % (tag, family, route), r, k)
        assert r <= k, (route, r, k)
    assert torch.equal(torch.view_as_real(routes['synthesize_complex']), torch.view_as_real(routes['c_complex']))
    assert torch.equal(torch.view_as_real(routes['synthesize_planes']), torch.view_as_real(routes['c_planes']))


@pytest.mark.parametrize('family', list(R.K_SYNTHESIS))
@pytest.mark.parametrize('path', ['fast', 'small'])
def test_synthesis_gradient(cqs, path, family):
    _check_synthesis(cqs[path], family, _n(path), path != 'fast')


def test_synthesis_gradient_forced_generic_edge_cases(cqs):
    _check_synthesis(cqs['forced'], 'tones', N, True, tag='forced ')
    _check_synthesis(cqs['forced'], 'impulses', N, True, tag='forced ')


# ---- magnitude gradient ------------------------------------------------------------------------------------------------------------------------

def _grad_magnitude(cq, audio, dmag, composed):
    x = audio.clone().requires_grad_()
    mag = cq.to_real(cq.encode(x)).norm(p=2, dim=-3) if composed else cq.magnitude(x)
    assert mag.shape == dmag.shape and mag.grad_fn is not None
    return torch.autograd.grad(mag, x, dmag)[0]


@pytest.mark.parametrize('path', ['fast', 'small'])
def test_magnitude_gradient(cqs, path):
    """Upstream gradient dmag = h |c_ref| with h in [0.5, 1.5]: dc = h c is well conditioned, and the result is held at K times the
    adjoint's bar on that dc.  On the specialised path magnitude() is the fused route (tt_cqt_forward_mag_bwd); on the any-length path it
    composes encode with torch's norm, as the composed route here does on both."""
    cq, n = cqs[path], _n(path)
    a_np, dmag_np, _, ref = R.magnitude_case(n)
    bar, k = R.analysis_bar('magnitude', n, path != 'fast'), R.K_ANALYSIS['magnitude'][0]
    a, dmag = torch.tensor(a_np).cuda(), torch.tensor(dmag_np).cuda()
    fused, composed = _grad_magnitude(cq, a, dmag, False), _grad_magnitude(cq, a, dmag, True)
    for route, got in (('magnitude()', fused), ('composed', composed)):
        got = got.cpu().numpy()
        assert np.isfinite(got).all()
        r = R.analysis_ratio(got, ref, bar)
        _note('magnitude gradient %s %s' % (path, route), r, k)
        assert r <= k, (route, r, k)
    r = R.analysis_ratio(fused.cpu().numpy(), composed.cpu().numpy().astype(np.float64), bar)
    _note('magnitude gradient %s magnitude() against composed' % path, r, k)
    assert r <= k
    if path == 'fast':
        assert torch.equal(fused, _c_magnitude_bwd(cq, a, dmag))


@pytest.mark.parametrize('path', ['fast', 'small'])
def test_magnitude_gradient_of_silence_is_zero(cqs, path):
    """|c| == 0 everywhere: torch's norm backward gives 0 there, not 0 / 0"""
    cq, n = cqs[path], _n(path)
    x = torch.zeros((2, 1, 2 * n), device='cuda', requires_grad=True)
    mag = cq.magnitude(x)
    d, = torch.autograd.grad(mag, x, torch.ones_like(mag))
    assert bool(torch.isfinite(d).all()) and not bool(d.any())


# ---- autograd plumbing -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('path', ['fast', 'small'])
def test_gradient_through_to_real_equals_its_contiguous_copy(cqs, path):
    cq, n = cqs[path], _n(path)
    g = torch.tensor(R.analysis_case('random', n)[0]).cuda()
    gp = _planes(g)
    x = torch.tensor(R.noise_audio(n)).cuda().requires_grad_()
    r = cq.to_real(cq.encode(x))
    assert r.shape == gp.shape and not r.is_contiguous()
    through_view, = torch.autograd.grad(r, x, gp)
    assert torch.equal(through_view, _c_analysis_bwd(cq, g))
    # and a non-contiguous grad_output of analyze / synthesize
    gt = gp.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not gt.is_contiguous()
    assert torch.equal(torch.autograd.grad(cq.analyze(x), x, gt)[0], _c_analysis_bwd(cq, gp))


def test_inputs_that_need_no_gradient_get_none(cqs):
    cq = cqs['small']
    x = torch.tensor(R.noise_audio(N_SMALL)).cuda()
    for fn in (cq.encode, cq.analyze, cq.magnitude):
        out = fn(x)
        assert not out.requires_grad and out.grad_fn is None
    c = cq.encode(x)
    assert not cq.synthesize(c).requires_grad
    # a leaf that requires grad next to one that does not: only the first gets a gradient
    c1, c2 = c.clone().requires_grad_(), c.clone()
    (cq.synthesize(c1) + cq.synthesize(c2)).sum().backward()
    assert c1.grad is not None and c2.grad is None


@pytest.mark.parametrize('path', ['fast', 'small'])
def test_detached_routes_keep_their_bits_and_stay_detached(cqs, path):
    cq, n = cqs[path], _n(path)
    x = torch.tensor(R.noise_audio(n)).cuda()
    xg = x.clone().requires_grad_()
    want = cq._transform(x, True)
    with torch.no_grad():
        e = cq.encode(xg)
    assert not e.requires_grad and torch.equal(torch.view_as_real(e), torch.view_as_real(want))
    assert torch.equal(torch.view_as_real(cq.encode(xg)), torch.view_as_real(want))            # the differentiable route: the same bits
    assert torch.equal(cq.analyze(xg), cq(x)) and torch.equal(cq.magnitude(xg), cq.magnitude(x))
    # forward() and decode() are the two calls the reference wraps in no_grad
    planes = cq(xg)
    assert planes.grad_fn is None and not planes.requires_grad
    cg = planes.clone().requires_grad_()
    audio = cq.decode(cg)
    assert audio.grad_fn is None and not audio.requires_grad
    assert torch.equal(cq.synthesize(cg), cq._decode_raw(planes))


@pytest.mark.parametrize('path', ['fast', 'small'])
def test_backward_twice_gives_identical_bits(cqs, path):
    cq, n = cqs[path], _n(path)
    g = torch.tensor(R.analysis_case('random', n)[0]).cuda()
    y = torch.tensor(R.synthesis_case('noise', n)[0]).cuda()
    a, dmag = (torch.tensor(v).cuda() for v in R.magnitude_case(n)[:2])
    for fn in (lambda: _grad_encode(cq, g), lambda: _grad_synthesize(cq, y, False), lambda: _grad_synthesize(cq, y, True),
               lambda: _grad_magnitude(cq, a, dmag, False)):
        first, second = fn(), fn()
        first, second = (torch.view_as_real(t) if t.is_complex() else t for t in (first, second))
        assert torch.equal(first, second)


# ---- through the model -------------------------------------------------------------------------------------------------------------------------

KW = dict(latent_size=None, model_complexity=1, skip_connections=False)


@functools.lru_cache(maxsize=None)
def _model_reference():
    """float64 on the CPU: oracle/autoencoder.py, the spectral loss of oracle/objectives.py and a waveform loss through decode_t;
    (audio float32, gradients of the sum, gradients of the waveform term alone) per parameter name"""
    tab = R.tables(N)
    audio = R.noise_audio(N)[:1, :, :N]
    sd = oae.closed_form_state_dict(oae.state_dict_shapes(540, **KW), amplitude=0.12)
    params = {k: v.double().requires_grad_() for k, v in sd.items()}
    a64 = torch.from_numpy(audio.astype(np.float64))
    coeffs = torch.from_numpy(np.ascontiguousarray(nsgt.wrapper_forward(audio.astype(np.float64), tab)))
    rec = oae.forward(coeffs, params, consistency=False)[0]
    spectral = oobj.compute_reconstruction_loss(rec, coeffs)
    wave = ((R.decode_t(torch.complex(rec[:, 0], rec[:, 1])[:, None], tab) - a64) ** 2).mean()
    names = list(params)

    def grads(loss):
        gs = torch.autograd.grad(loss, [params[k] for k in names], retain_graph=True, allow_unused=True)
        return {k: (torch.zeros_like(params[k]) if g is None else g).numpy() for k, g in zip(names, gs)}
    return audio, sd, grads(spectral + wave), grads(wave)


def _model_step(model, a, wave_only=False, dtype=None):
    from timbre_trap.framework import compute_reconstruction_loss
    model.zero_grad(set_to_none=True)
    coeffs = model.sliCQ(a)
    with torch.autocast(device_type='cuda', dtype=dtype, enabled=dtype is not None):
        rec = model(a)[0]
        wave = ((model.sliCQ.synthesize(rec) - a) ** 2).mean()
        loss = wave if wave_only else compute_reconstruction_loss(rec, coeffs) + wave
        loss.backward()
    return {k: (torch.zeros_like(p) if p.grad is None else p.grad.detach().float().clone()) for k, p in model.named_parameters()}


def test_waveform_loss_trains_the_model(cqs):
    """Loss = compute_reconstruction_loss + mean((synthesize(reconstruction) - audio)^2) on TimbreTrap(22050, 9, 60, 3, latent_size=None,
    model_complexity=1), one clip, one block, fp32: every parameter gradient against the float64 restatement at the bar test_gpu_model.py
    holds fp32 parameter gradients to (rtol 5e-3, atol 5e-4 of the parameter's largest reference gradient) -- for the sum, and for the
    waveform term alone, which contributes no gradient at all without a differentiable synthesis.  Then the same step under bf16
    autocast: finite, and the flat gradient's cosine to the fp32 one at least 0.995 (the bar smoke() holds a 16-bit route to)."""
    from timbre_trap.framework import TimbreTrap
    audio, sd, ref_sum, ref_wave = _model_reference()
    model = TimbreTrap(R.SR, 9, 60, 3, **KW)
    model.load_state_dict(sd, strict=True)
    model = model.cuda()
    a = torch.tensor(audio).cuda()
    got_sum = _model_step(model, a)
    for what, got, ref in (('sum', got_sum, ref_sum), ('waveform term', _model_step(model, a, wave_only=True), ref_wave)):
        worst = 0.0
        for k in ref:
            top = float(np.abs(ref[k]).max())
            err = np.abs(got[k].cpu().numpy() - ref[k]) - 5e-3 * np.abs(ref[k])
            worst = max(worst, float(err.max()) / (5e-4 * (top + 1e-6)))
        print('parameter gradients of the %s: worst (|got - ref| - 5e-3 |ref|) / (5e-4 max |ref|) = %.3f' % (what, worst))
        assert any(np.abs(ref[k]).max() > 0 for k in ref if k.startswith('decoder.'))
        for k in ref:
            np.testing.assert_allclose(got[k].cpu().numpy(), ref[k], rtol=5e-3, atol=5e-4 * float(np.abs(ref[k]).max() + 1e-6), err_msg='%s: %s' % (what, k))
    got16 = _model_step(model, a, dtype=torch.bfloat16)
    flat32, flat16 = (torch.cat([g[k].flatten() for k in ref_sum]) for g in (got_sum, got16))
    cos = float(torch.dot(flat16, flat32) / (flat16.norm() * flat32.norm()))
    print('bf16 autocast: flat-gradient cosine to the fp32 step %.5f' % cos)
    assert bool(torch.isfinite(flat16).all()) and cos >= 0.995
