"""
GPU parity of the magnitude variants TimbreTrapMag / TimbreTrapMagDB (reference modules.py:892-1075): the fp32 route against values
recorded from the reference (tests/golden/variants.npz), inference against the CPU oracle composed from oracle.autoencoder's
shape-generic functions (encoder_forward with a (C0,1,3,3) convin, decode, then relu / sigmoid), the front-end kernels
(tt_cqt_forward_mag, tt_magnitude, tt_decibels) against torch / oracle.nsgt, the one-channel 16-bit edge kernels stage by stage through the
C ABI against float64 restatements, the autocast train step against the composed oracle, and its run-to-run determinism.
"""

import numpy as np
import pytest
import torch

import stub_cqt
from oracle import autoencoder as oae
from oracle import nsgt

pytestmark = pytest.mark.gpu
N, M, SR = 66150, 1024, 22050
LOGIT_TOL = dict(rtol=1e-4, atol=1e-4)
KW = dict(mc1=dict(latent_size=None, model_complexity=1, skip_connections=False),
          mc2=dict(latent_size=128, model_complexity=2, skip_connections=False),
          mc2skip=dict(latent_size=128, model_complexity=2, skip_connections=True))
ACT = dict(TimbreTrapMag=torch.relu, TimbreTrapMagDB=torch.sigmoid)


def _shapes(**kw):
    shapes = oae.state_dict_shapes(540, **kw)
    c0 = shapes['encoder.convin.0.weight'][0]
    shapes['encoder.convin.0.weight'] = (c0, 1, 3, 3)
    shapes['decoder.convout.weight'] = (1, c0, 3, 3)
    shapes['decoder.convout.bias'] = (1,)
    return shapes


def _model(name, kw, sd=None):
    import timbre_trap.framework as fw
    m = getattr(fw, name)(SR, 9, 60, 3, **kw)
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    return m.cuda()


class _features:
    """``with _features(model, f):`` -- model.sliCQ.magnitude(audio) returns ``f`` (B,F,T): the transform is pinned on its own, the
    autoencoder routes get recorded features (MagDB still takes them through its own CQT.to_decibels)."""

    def __init__(self, model, f):
        self.cqt, self.f = model.sliCQ, f

    def __enter__(self):
        self.cqt.magnitude = lambda audio: self.f
        return self

    def __exit__(self, *exc):
        del self.cqt.magnitude
        return False


def _oracle_features(name, mag):
    """The encoder input of the reference from magnitudes (B,F,T), float64 oracle arithmetic for the dB map."""
    if name == 'TimbreTrapMagDB':
        return torch.from_numpy(nsgt.to_decibels(mag.double().numpy())).float().unsqueeze(-3)
    return mag.unsqueeze(-3)


def _oracle_infer(name, feat, sd, transcribe):
    """TimbreTrapMag(DB).decode(encode(.)) after the transform, composed from oracle.autoencoder."""
    with torch.no_grad():
        latents, emb = oae.encoder_forward(feat, sd)
        return ACT[name](oae.decode(latents, sd, oae.apply_skip_connections(emb, sd), transcribe))


@pytest.mark.parametrize('name', ('TimbreTrapMag', 'TimbreTrapMagDB'))
@pytest.mark.parametrize('tag', ('mc1', 'mc2skip'))
def test_variant_forward_losses_gradients_golden(golden, name, tag):
    """model.forward (consistency) + the train.py losses + gradients, fp32 route, vs the reference on closed-form weights."""
    from timbre_trap.framework import CQT, compute_consistency_loss, compute_reconstruction_loss, compute_transcription_loss
    g = golden('variants')
    pre = '%s_%s' % (name, tag)
    sd = oae.closed_form_state_dict(_shapes(**KW[tag]))
    model = _model(name, KW[tag], sd)
    audio = stub_cqt.closed_form_audio(2, 64)
    mag = torch.from_numpy(nsgt.to_magnitude(nsgt.to_real(stub_cqt.stub_encode(audio, 540, 64, 16).numpy()))).float().contiguous().cuda()
    # the reconstruction target of train.py:406-413
    target = CQT.to_magnitude(torch.from_numpy(nsgt.to_real(stub_cqt.stub_encode(audio, 540, 64, 16).numpy())).contiguous().cuda()).unsqueeze(-3)
    if name == 'TimbreTrapMagDB':
        target = CQT.to_decibels(target)
    with _features(model, mag):
        rec, latents, trn, trn_rec, trn_scr, losses = model(torch.zeros(2, 1, 8, device='cuda'), True)
    assert losses == {} and rec.shape == (2, 1, 540, 16)
    for nm, t in (('reconstruction', rec), ('latents', latents), ('transcription', trn),
                  ('transcription_rec', trn_rec), ('transcription_scr', trn_scr)):
        np.testing.assert_allclose(t.detach().cpu().numpy(), g[f'{pre}_fwd_{nm}'], err_msg=nm, **LOGIT_TOL)
    act = model.to_activations(trn)
    assert act.shape == (2, 540, 16)
    np.testing.assert_allclose(act.detach().cpu().numpy(), g[f'{pre}_act'], rtol=1e-4, atol=1e-5)
    gt = stub_cqt.closed_form_targets(2, 540, 16).cuda()
    l_rec = compute_reconstruction_loss(rec, target)
    l_trn = compute_transcription_loss(act, gt, True)
    l_sp, l_sc = compute_consistency_loss(trn_rec, trn_scr, trn)
    total = l_rec + l_trn + (l_sp + l_sc)
    np.testing.assert_allclose([float(v.detach()) for v in (l_rec, l_trn, l_sp, l_sc, total)], g[f'{pre}_losses'], rtol=1e-4, atol=1e-9)
    model.zero_grad()
    total.backward()
    for k, p in model.named_parameters():
        if f'{pre}_grad.{k}' in g:
            ref = g[f'{pre}_grad.{k}']
            np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=5e-3, atol=5e-4 * float(np.abs(ref).max() + 1e-6), err_msg=k)
        else:
            st = g[f'{pre}_gradstat.{k}']
            gg = p.grad.double().flatten().cpu()
            np.testing.assert_allclose(float(gg.norm()), st[1], rtol=2e-3, atol=1e-12, err_msg=k)
            np.testing.assert_allclose(gg[:6].numpy(), st[2:], rtol=1e-2, atol=2e-3 * st[1] + 1e-12, err_msg=k)


@pytest.mark.parametrize('name', ('TimbreTrapMag', 'TimbreTrapMagDB'))
def test_variant_inference_vs_composed_oracle(name):
    """chunked_inference / transcribe / reconstruct / inference at mc 2 against the oracle composed per chunk, real transform (its
    magnitudes taken from the HIP CQT, pinned on its own): the reference's (B,2,F,T) broadcast of the 1-channel chunks included."""
    sd = oae.closed_form_state_dict(_shapes(**KW['mc2']), amplitude=0.08)
    sd['decoder.convout.bias'] = torch.full((1,), 0.05)           # logits on both sides of 0: the relu passes some, clips others
    model = _model(name, KW['mc2'], sd).eval()
    g = torch.Generator().manual_seed(21)
    audio = torch.rand(1, 1, N, generator=g) * 2 - 1
    a = audio.cuda()
    trn = model.chunked_inference(a, True)
    rec = model.chunked_inference(a, False)
    assert trn.shape == rec.shape == (1, 2, 540, M) and torch.equal(trn[:, 0], trn[:, 1])
    # the oracle: reference modules.py:204-269 with the chunk outputs added into zeros((B,2,F,T))
    hop = N // 2
    padded = torch.nn.functional.pad(audio, [hop] * 2)
    n_chunks = (padded.size(-1) - hop) // hop
    window = torch.signal.windows.hann(M, dtype=torch.float32)
    want = {t: torch.zeros(1, 2, 540, 2 * M) for t in (True, False)}
    for i in range(n_chunks):
        mag = model.sliCQ.magnitude(padded[..., i * hop: i * hop + N].cuda()).cpu()
        feat = _oracle_features(name, mag)
        for t in (True, False):
            want[t][..., i * M // 2: i * M // 2 + M] += window * _oracle_infer(name, feat, sd, t)

    def rel(got, w):                                              # (a relu output may be all zero: the bar is then absolute)
        return float((got.cpu() - w).abs().max()) / max(float(w.abs().max()), 1e-2)
    assert float(want[False].abs().max()) > 1e-2
    for t, got in ((True, trn), (False, rec)):
        w = want[t][..., M // 2: -M // 2]
        assert rel(got, w) < 1e-4, (t, rel(got, w))
    act = model.transcribe(a)
    assert act.shape == (1, 2, 540, M)
    want_act = torch.tanh(want[True][..., M // 2: -M // 2]) if name == 'TimbreTrapMag' else want[True][..., M // 2: -M // 2]
    assert float((act.cpu() - want_act).abs().max()) < 1e-4
    # reconstruct = the transform's inverse of the (B,2,F,T) reconstruction pinned above (re = im); the inverse itself is pinned on its
    # own, and its inf-norm division magnifies 1e-4 coefficient differences: the route is checked, not the inverse again
    audio_back = model.reconstruct(a)
    assert audio_back.shape == (1, 1, N) and torch.equal(audio_back, model.sliCQ.decode(rec))
    one = model.inference(a)
    assert one.shape == (1, 1, 540, M)
    want_one = _oracle_infer(name, _oracle_features(name, model.sliCQ.magnitude(a).cpu()), sd, False)
    assert rel(one, want_one) < 1e-4


def test_front_end_kernels():
    """tt_cqt_forward_mag and tt_magnitude = torch's norm of tt_cqt_forward's output (1e-6 relative); tt_decibels = oracle.nsgt.to_decibels
    (float64) on (B,F,T) and (B,1,F,T) inputs, an all-zero clip and exact zeros, rescale on and off; autograd inputs keep torch."""
    from timbre_trap.framework import CQT
    cqt = CQT(9, 60, SR, 3).cuda()
    g = torch.Generator().manual_seed(8)
    audio = (torch.rand(3, 1, 2 * N, generator=g) * 2 - 1).cuda()
    c = cqt(audio)
    ref = c.norm(p=2, dim=-3)
    for got in (cqt.magnitude(audio), CQT.to_magnitude(c)):
        assert got.shape == ref.shape == (3, 540, 2 * M)
        assert float(((got - ref).abs() / ref.abs().clamp_min(1e-30)).max()) < 1e-6
    m = ref.clone()
    m[1] = 0.0                                                   # an all-zero clip
    m[2, :, :100] = 0.0                                          # exact zeros beside non-zero values
    m[0] *= 1e-3
    for x in (m, m.unsqueeze(1)):
        for rescale in (True, False):
            got = CQT.to_decibels(x, rescale)
            want = nsgt.to_decibels(x.double().cpu().numpy(), rescale)
            assert got.shape == x.shape and got.dtype == torch.float32
            err = np.abs(got.cpu().numpy() - want)
            bar = 1e-6 if rescale else 1e-6 * max(1.0, float(np.abs(want).max()))   # dB values up to ~200: fp32's own spacing
            assert float(err.max()) < bar, (rescale, float(err.max()))
    # a NaN propagates to its whole clip, as in torch's clamp / max / maximum
    nan_in = m[:2].clone()
    nan_in[0, 5, 7] = float('nan')
    d = CQT.to_decibels(nan_in)
    assert bool(torch.isnan(d[0]).all()) and bool(torch.isfinite(d[1]).all())
    # the same clip twice gives the same bits (the item maxima meet in a fixed order)
    assert torch.equal(CQT.to_decibels(m), CQT.to_decibels(m))
    # an input that requires grad still gets autograd (the torch expression)
    x = m[:2].clone().requires_grad_(True)
    d = CQT.to_decibels(CQT.to_magnitude(torch.stack((x, x), dim=1)))
    d.sum().backward()
    assert x.grad is not None and d.grad_fn is not None



def test_front_end_takes_the_kernels_on_device_tensors(monkeypatch):
    """CQT.to_magnitude / CQT.to_decibels on CUDA fp32 tensors outside autograd go through tt_magnitude / tt_decibels (ops.magnitude /
    ops.decibels), not the torch expression that gives the same values."""
    from timbre_trap.framework import CQT, ops
    calls = []
    for name in ('magnitude', 'decibels'):
        orig = getattr(ops, name)
        monkeypatch.setattr(ops, name, (lambda o, n: lambda *a: (calls.append(n), o(*a))[1])(orig, name))
    c = torch.rand(2, 2, 540, 64, device='cuda')
    CQT.to_decibels(CQT.to_magnitude(c))
    assert calls == ['magnitude', 'decibels']
    CQT.to_decibels(CQT.to_magnitude(c.cpu()))
    CQT.to_magnitude(c.clone().requires_grad_(True))
    assert calls == ['magnitude', 'decibels']


# ---- the one-channel 16-bit channels-last edges, stage by stage -----------------------------------------------------------------------

def _e16(dtype):
    return dict(bf16=torch.bfloat16, fp16=torch.float16)[dtype]


def _cl16(t, dtype):
    from timbre_trap.framework import ops
    return ops._pack(t.float().contiguous(), dtype)


@pytest.mark.parametrize('dtype', ('bf16', 'fp16'))
@pytest.mark.parametrize('B,H,T', ((2, 37, 70), (1, 48, 128)), ids=('border-scalar', 'vector'))
def test_one_channel_edge_kernels_vs_float64(dtype, B, H, T):
    """tt_convin16_1_{fwd,bwd} and tt_convout16_1_{fwd,bwd} (bf16 and the _h fp16 build) against float64 restatements with the same
    roundings: B > 1, T % 4 != 0 (scalar staging) and H not a multiple of 16 (border tiles); convin backward with and without dx and
    pregated; convout with none / relu / sigmoid."""
    import torch.nn.functional as Fn
    from timbre_trap import _hip
    from timbre_trap.framework import ops
    from timbre_trap.framework.ops import ACT_NONE, ACT_RELU, ACT_SIGMOID
    et = _e16(dtype)
    lib = ops.lib16(et)
    P = _hip.ptr
    st = _hip.stream_ptr()
    g = torch.Generator().manual_seed(B * 1000 + H + T)
    ws = torch.empty(lib.tt_edge16_scratch_bytes(), dtype=torch.uint8, device='cuda')
    eps = 2.0 ** -8 if et == torch.bfloat16 else 2.0 ** -11

    def close(got, want, what, k=2.0):
        got, want = got.double().cpu(), want.double().cpu()
        err = float((got - want).abs().max())
        assert err <= k * eps * float(want.abs().max()) + 1e-6, (what, err, float(want.abs().max()))

    # ---- convin 1 -> 4 + ELU
    x = torch.randn(B, 1, H, T, generator=g).cuda()
    w = (torch.randn(4, 1, 3, 3, generator=g) * 0.5).cuda()
    b = (torch.randn(4, generator=g) * 0.1).cuda()
    y = ops.new_cl16(B, 4, H, T, 'cuda', et)
    _hip.check(lib.tt_convin16_1_fwd(P(x), P(w), P(b), P(y), B, H, T, st), 'tt_convin16_1_fwd')
    want = Fn.elu(Fn.conv2d(x.double(), w.double(), b.double(), padding=1))
    close(y.float(), want.to(et).double(), 'convin fwd', k=1.0)
    dy = _cl16(torch.randn(B, 4, H, T, generator=g).cuda(), et)
    gate = torch.clamp(y.double() + 1.0, max=1.0)                 # ELU' through the saved (rounded) output
    gd = dy.double() * gate
    xd = x.double().requires_grad_(True)
    wd = w.double().requires_grad_(True)
    bd = torch.zeros(4, dtype=torch.float64, device='cuda', requires_grad=True)
    Fn.conv2d(xd, wd, bd, padding=1).backward(gd)
    for with_dx in (True, False):
        for pre in (False, True):
            dx = torch.full_like(x, float('nan')) if with_dx else None
            dw, db = torch.zeros_like(w), torch.zeros_like(b)
            src = _cl16(gd.float(), et) if pre else dy                 # pregated: dy arrives multiplied by ELU'(y), y is not read
            _hip.check(lib.tt_convin16_1_bwd(P(x), None if pre else P(y), P(src), P(w), P(dx), P(dw), P(db), P(ws), B, H, T, st),
                       'tt_convin16_1_bwd')
            tag = 'convin bwd dx=%d pre=%d' % (with_dx, pre)
            k = 4.0 if pre else 1e-3                                  # (pregated: the gated dy is itself rounded to 16 bits once more)
            close(dw, wd.grad, tag + ' dw', k)
            close(db, bd.grad, tag + ' db', k)
            if with_dx:
                close(dx, xd.grad, tag + ' dx', k)

    # ---- convout 4 -> 1 + none / relu / sigmoid, single and pair form
    xc = _cl16(torch.randn(B, 4, H, T, generator=g).cuda(), et)
    wo = (torch.randn(1, 4, 3, 3, generator=g) * 0.5).cuda()
    bo = (torch.randn(1, generator=g) * 0.1).cuda()
    dyo = torch.randn(B, 1, H, T, generator=g).cuda()
    acts = {ACT_NONE: lambda t: t, ACT_RELU: torch.relu, ACT_SIGMOID: torch.sigmoid}
    for act, fn in acts.items():
        yo = torch.empty(B, 1, H, T, device='cuda')
        _hip.check(lib.tt_convout16_1_fwd(P(xc), P(wo), P(bo), P(yo), B, H, T, act, st), 'tt_convout16_1_fwd')
        xd = xc.double().requires_grad_(True)
        wd = wo.double().requires_grad_(True)
        bd = bo.double().requires_grad_(True)
        ref = fn(Fn.conv2d(xd, wd, bd, padding=1))
        close(yo, ref.detach(), 'convout fwd act %d' % act, k=1e-3)
        ref.backward(dyo.double())
        dx = ops.new_cl16(B, 4, H, T, 'cuda', et)
        dw, db = torch.zeros_like(wo), torch.zeros_like(bo)
        _hip.check(lib.tt_convout16_1_bwd(P(xc), P(yo) if act != ACT_NONE else None, P(dyo), P(wo), P(dx), P(dw), P(db), P(ws), B, H, T, act,
                                          st), 'tt_convout16_1_bwd')
        close(dx.float(), xd.grad.to(et).double(), 'convout bwd dx act %d' % act, k=1.0)
        close(dw, wd.grad, 'convout bwd dw act %d' % act, k=1e-3)
        close(db, bd.grad, 'convout bwd db act %d' % act, k=1e-3)
        # the pair form (TimbreTrap.decode_pair): the same numbers per half
        if B % 2 == 0:
            xp = xc.detach()
            w_ = wo.clone().requires_grad_(True)
            b_ = bo.clone().requires_grad_(True)
            y0, y1 = ops.ConvOut16x1PairFn.apply(xp, w_, b_, act)
            assert torch.equal(torch.cat((y0, y1)), yo)
            (y0 * dyo[:B // 2]).sum().backward(retain_graph=True)
            (y1 * dyo[B // 2:]).sum().backward()
            close(w_.grad, wd.grad, 'pair dw act %d' % act, k=1e-3)


# ---- the train step under autocast against the composed oracle ------------------------------------------------------------------------

_ORACLE = {}


def _mag_oracle_run(name, tag):
    """The fp32 CPU oracle of one TimbreTrapMag(DB) train step (reference train.py:404-464 with the :406-413 target) at mc 2 / latent 128,
    default initialisation under seed 2, two clips of one 3-s block, features = the HIP transform's magnitudes (pinned on its own)."""
    key = (name, tag)
    if key in _ORACLE:
        return _ORACLE[key]
    from oracle import objectives as oobj
    torch.manual_seed(2)
    model = _model(name, KW[tag])
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if not k.startswith('sliCQ.')}
    if 'skip_weights' in sd:
        sd['skip_weights'] = torch.tensor([0.7, 1.1, 0.9, 1.3, 0.8])
    audio = torch.rand(2, 1, N, generator=torch.Generator().manual_seed(1234)) * 2 - 1
    with torch.no_grad():
        mag = model.sliCQ.magnitude(audio.cuda()).cpu()
    del model
    feat = _oracle_features(name, mag)
    gt = stub_cqt.closed_form_targets(2, 540, M)
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}

    def decode(latents, emb, transcribe):
        return ACT[name](oae.decode(latents, params, emb, transcribe))
    latents, emb = oae.encoder_forward(feat, params)
    emb = oae.apply_skip_connections(emb, params)
    rec, trn = decode(latents, emb, False), decode(latents, emb, True)
    lat2, emb2 = oae.encoder_forward(trn, params)
    emb2 = oae.apply_skip_connections(emb2, params)
    trn_rec, trn_scr = decode(lat2, emb2, False), decode(lat2, emb2, True)
    act = torch.tanh(trn.squeeze(-3)) if name == 'TimbreTrapMag' else trn.squeeze(-3)
    parts = dict(reconstruction=oobj.compute_reconstruction_loss(rec, feat), transcription=oobj.compute_transcription_loss(act, gt, True))
    parts['consistency_spectral'], parts['consistency_score'] = oobj.compute_consistency_loss(trn_rec, trn_scr, trn)
    total = parts['reconstruction'] + parts['transcription'] + (parts['consistency_spectral'] + parts['consistency_score'])
    total.backward()
    run = dict(sd=sd, mag=mag, feat=feat, gt=gt, outputs=[t.detach() for t in (rec, latents, trn, trn_rec, trn_scr)],
               parts={k: float(v.detach()) for k, v in parts.items()}, total=float(total.detach()),
               grads={k: v.grad.detach().clone() for k, v in params.items()})
    _ORACLE[key] = run
    return run


def _count(monkeypatch, cls):
    calls = []
    orig = cls.apply
    monkeypatch.setattr(cls, 'apply', staticmethod(lambda *a: (calls.append(1), orig(*a))[1]))
    return calls


ROUTES16 = [('TimbreTrapMag', 'mc2', True), ('TimbreTrapMag', 'mc2', False), ('TimbreTrapMagDB', 'mc2', True),
            ('TimbreTrapMagDB', 'mc2', False), ('TimbreTrapMag', 'mc2skip', True), ('TimbreTrapMagDB', 'mc2skip', True)]


@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float16), ids=('bf16', 'fp16'))
@pytest.mark.parametrize('name,tag,pair', ROUTES16, ids=['-'.join((n[9:], t, 'pair' if p else 'two')) for n, t, p in ROUTES16])
def test_autocast_step_matches_composed_oracle(monkeypatch, name, tag, pair, dtype):
    """model.forward + the train.py losses + backward under torch.autocast (the 16-bit channels-last path, both edges on the one-channel
    kernels) against the fp32 CPU oracle: five outputs, four losses and every parameter gradient at the bars of the complex model's
    autocast tests (outputs 3e-2 of their maximum, losses 1e-2, gradient relative L2 3e-2 / biases 6e-2, cosine 0.999, median 2e-2)."""
    from timbre_trap.framework import CQT, TimbreTrap, compute_consistency_loss, compute_reconstruction_loss, compute_transcription_loss, ops
    from timbre_trap.utils import FusedAdamW
    run = _mag_oracle_run(name, tag)
    model = _model(name, KW[tag])
    model.load_state_dict(run['sd'], strict=False)
    opt = FusedAdamW(model.parameters(), lr=1e-3, max_norm=10.0)
    monkeypatch.setattr(TimbreTrap, 'PAIR_DECODE', pair)
    n_in, n_pair, n_out, n_fp32 = (_count(monkeypatch, c) for c in (ops.ConvIn16x1Fn, ops.ConvOut16x1PairFn, ops.ConvOut16x1Fn, ops.ConvFn))
    mag, gt = run['mag'].cuda(), run['gt'].cuda()
    target = mag.unsqueeze(-3)
    if name == 'TimbreTrapMagDB':
        target = CQT.to_decibels(target)
    with _features(model, mag), torch.autocast(device_type='cuda', dtype=dtype):
        rec, latents, trn, trn_rec, trn_scr, _ = model(torch.zeros(2, 1, 8, device='cuda'), True)
        l_sp, l_sc = compute_consistency_loss(trn_rec, trn_scr, trn)
        losses = (compute_reconstruction_loss(rec, target), compute_transcription_loss(model.to_activations(trn), gt, True), l_sp, l_sc)
        total = losses[0] + losses[1] + (losses[2] + losses[3])
        opt.zero_grad()
        total.backward()
    torch.cuda.synchronize()
    # both edges on the one-channel 16-bit kernels, no edge layer (nor anything else) on the fp32 ConvFn
    assert (len(n_in), len(n_pair), len(n_out), len(n_fp32)) == (2, 2 if pair else 0, 0 if pair else 4, 0), \
        (len(n_in), len(n_pair), len(n_out), len(n_fp32))
    out_bar, loss_bar, grad_bar, bias_bar, cos_bar, median_bar = 3e-2, 1e-2, 3e-2, 6e-2, 0.999, 2e-2
    for nm, got, want in zip(('reconstruction', 'latents', 'transcription', 'transcription_rec', 'transcription_scr'),
                             (rec, latents, trn, trn_rec, trn_scr), run['outputs']):
        assert got.shape == want.shape, nm
        err = float((got.detach().float().cpu() - want).abs().max() / want.abs().max())
        assert err < out_bar, (nm, err)
    for nm, got in zip(('reconstruction', 'transcription', 'consistency_spectral', 'consistency_score'), losses):
        want = run['parts'][nm]
        assert abs(float(got.detach()) - want) <= loss_bar * abs(want) + 1e-5 * abs(run['total']), (nm, float(got.detach()), want)
    stats = []
    for k, p in model.named_parameters():
        gq, wq = p.grad.detach().double().cpu().flatten(), run['grads'][k].double().flatten()
        stats.append((float((gq - wq).norm() / (wq.norm() + 1e-30)), float(torch.dot(gq, wq) / (gq.norm() * wq.norm() + 1e-30)), k))
    stats.sort(reverse=True)
    print('%s %s %s pair=%d: gradient relative L2 median %.3e, worst %.3e (%s), worst cosine %.6f'
          % (name, tag, str(dtype), pair, sorted(r for r, _, _ in stats)[len(stats) // 2], stats[0][0], stats[0][2], min(c for _, c, _ in stats)))
    for rel, cos, k in stats:
        assert rel <= (bias_bar if k.endswith('.bias') else grad_bar) and cos >= cos_bar, (k, rel, cos)
    assert sorted(r for r, _, _ in stats)[len(stats) // 2] <= median_bar


def test_mag_bf16_step_is_bit_reproducible():
    """Two TimbreTrapMag bf16 train steps from the same state give bit-identical flat gradients (the edge weight / bias gradients are
    reduced in a fixed order, like every other backward of the 16-bit path)."""
    from timbre_trap.framework import compute_consistency_loss, compute_reconstruction_loss, compute_transcription_loss
    from timbre_trap.utils import FusedAdamW
    torch.manual_seed(3)
    model = _model('TimbreTrapMag', KW['mc2'])
    opt = FusedAdamW(model.parameters(), lr=1e-3, max_norm=10.0)
    g = torch.Generator().manual_seed(9)
    mag = (torch.randn(2, 540, 512, generator=g) * 0.5).abs().cuda()
    gt = (torch.rand(2, 540, 512, generator=g) < 0.02).float().cuda()
    flats = []
    for _ in range(2):
        with _features(model, mag), torch.autocast(device_type='cuda', dtype=torch.bfloat16):
            rec, _, trn, trn_rec, trn_scr, _ = model(torch.zeros(2, 1, 8, device='cuda'), True)
            l_sp, l_sc = compute_consistency_loss(trn_rec, trn_scr, trn)
            total = compute_reconstruction_loss(rec, mag.unsqueeze(1)) + compute_transcription_loss(model.to_activations(trn), gt, True) + (l_sp + l_sc)
            opt.zero_grad()
            total.backward()
        torch.cuda.synchronize()
        flats.append(opt.flat_grad.clone())
    assert torch.equal(flats[0], flats[1])
