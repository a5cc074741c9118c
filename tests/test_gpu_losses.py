"""
The objectives of csrc/losses.hip through the C ABI against float64 on the CPU, computed from the same fp32 inputs: the squared
differences (two-pass, fused, rescaled; one and two terms), the transcription loss (weighted and not) and to_activations.

The fused and the two-pass kernels share loops, partial sums and tail code, so comparing them with each other (tests/test_gpu_model.py)
cannot see a fault they share.  The shapes here take every path of those loops: lengths below four and with an n % 4 tail, a length
twice past the grid cap (a workgroup takes more than one stride), F < 4 (empty quarters of the frame kernel), B T no multiple of 64,
and B T > 65536 (workgroups loop over blocks of frames with barriers inside the loop).  Every output lies in a NaN-filled buffer and
must come back finite: a kernel that skipped the n % 4 tail (n = 1, 2, 3, 5, 1023, 4099 and the capped-grid length all have one)
would leave NaN there, and its loss would lack the tail's terms -- a third of the sum at n = 3, all of it at n = 1.

Every check prints its ratio to the bar (pytest -rP).  Worst ones measured on an MI355X: squared differences -- loss 0.07 (one term)
and 0.14 (two terms), gradients 0.38 (fused), 0.39 (tt_sqdiff_bwd), 0.48 (two terms fused), 0.51 (tt_sqdiff2_bwd); transcription --
loss 0.02, frame scale 0.22, gradient 0.11; activations -- forward 0.08, backward 0.05, one-channel forward 0.07, backward 0.03.

tt_sqdiff_sum and tt_sqdiff_sum_grad are documented to return the same bits (include/ttrap.h).  They did not: the compiler contracted
d0 d0 + d1 d1 into a fused multiply-add in one kernel and not in the other, and at n = 4 the two losses came out an fp32 ulp apart.
Both now sum the squares through one helper that spells the operations out, and test_sqdiff_one_term_matches_float64 asserts equality.
"""

import ctypes

import pytest
import torch

from oracle import objectives as oobj

pytestmark = pytest.mark.gpu

MAXP = 1024                                          # csrc/losses.hip: the grid cap of the reductions, and the stride of the second partial row
BADARG = -1
PAD = 8                                              # NaN sentinel behind every output


def _api():
    from timbre_trap import _hip
    return _hip.lib(), _hip.ptr, _hip.check, _hip.stream_ptr()


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def _out(n):
    return torch.full((n + PAD,), float('nan'), device='cuda')


def _scalar(v):
    return None if v is None else torch.tensor([v], dtype=torch.float32, device='cuda')


_worst = {}


def _note(key, ratio):
    _worst[key] = max(_worst.get(key, 0.0), ratio)
    print('ratio to bar: %-28s %.3f (worst so far %.3f)' % (key, ratio, _worst[key]))


def _check_elem(key, got, n, want, bar, what):
    """got: an output of n + PAD floats on the GPU; want, bar: float64 on the CPU.  Elementwise |got - want| <= bar, sentinel untouched."""
    torch.cuda.synchronize()
    assert bool(torch.isnan(got[n:]).all()), '%s: wrote past the end' % what
    e = (got[:n].double() - want.reshape(-1).cuda()).abs()
    bar = bar.reshape(-1).cuda()
    assert bool(torch.isfinite(got[:n]).all()), '%s: not finite' % what
    ratio = float((e / bar.clamp_min(1e-300)).max())
    _note(key, ratio)
    assert bool((e <= bar).all()), '%s: %.3f of the bar' % (what, ratio)


def _check_loss(key, got, want, rel, what):
    torch.cuda.synchronize()
    got = float(got)
    _note(key, abs(got - want) / (rel * abs(want)) if want else float(got != 0))
    assert abs(got - want) <= rel * abs(want), '%s: %r vs %r' % (what, got, want)


# ---- squared differences --------------------------------------------------------------------------------------------------------------
SQ_SIZES = [1, 2, 3, 4, 5, 1023, 4099, MAXP * 256 * 16 * 2 + 5]     # the last: twice past the cap of tt_sqdiff_sum's grid, with a tail
G_REL = 4e-7                                         # three fp32 roundings (difference, 2 scale g, product), the bar of tests/test_gpu_model.py


def _sq_inputs(n, close):
    gen = torch.Generator().manual_seed(1000 + n % 997 + int(close))
    b = torch.randn(n, generator=gen)
    if close:                                        # differences small against the operands
        a1, a2 = b + 1e-4 * torch.randn(n, generator=gen), b + 1e-4 * torch.randn(n, generator=gen)
    else:
        a1, a2 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    return a1, a2, b


@pytest.mark.parametrize('n,close', [(n, False) for n in SQ_SIZES] + [(4099, True), (5, True)])
def test_sqdiff_one_term_matches_float64(n, close):
    """tt_sqdiff_sum, tt_sqdiff_sum_grad + tt_sqdiff_rescale, tt_sqdiff_bwd: loss within 1e-6 relative (every term positive, at most
    three fp32 roundings each, summed in double), gradients 2 scale g (a - b) and their negative within 4e-7 |want| elementwise."""
    lib, ptr, check, st = _api()
    a, _, b = _sq_inputs(n, close)
    scale = _f32(1.0 / 37)
    d = a.double() - b.double()
    want_loss = float((d * d).sum()) * scale
    ad, bd = a.cuda(), b.cuda()
    partials = torch.full((2 * MAXP,), float('nan'), dtype=torch.float64, device='cuda')
    loss = torch.full((1,), float('nan'), device='cuda')
    check(lib.tt_sqdiff_sum(ptr(ad), ptr(bd), ptr(loss), ptr(partials), n, scale, st), 'tt_sqdiff_sum')
    _check_loss('sqdiff_sum loss', loss, want_loss, 1e-6, 'tt_sqdiff_sum n %d' % n)
    two_pass = float(loss)

    # the NULL-output and scalar variants run the same loops whatever the length: at the capped-grid length one of each is enough
    big = n > 1 << 20
    for has_da, has_db in ((True, True),) if big else ((True, True), (True, False), (False, True)):
        da, db = _out(n), _out(n)
        loss.fill_(float('nan'))
        check(lib.tt_sqdiff_sum_grad(ptr(ad), ptr(bd), ptr(loss), ptr(partials), n, scale, ptr(da) if has_da else None,
                                     ptr(db) if has_db else None, st), 'tt_sqdiff_sum_grad')
        _check_loss('sqdiff_sum_grad loss', loss, want_loss, 1e-6, 'tt_sqdiff_sum_grad n %d' % n)
        assert float(loss) == two_pass                     # the same loops and partial sums (csrc/losses.hip)
        for g in (0.3,) if big else (1.0, 0.5, 0.3):
            # the stored gradient is for an incoming 1; rescaling it by g1 then g2 gives g1 g2: apply each g to a fresh copy
            ca, cb = da.clone(), db.clone()
            gs = _scalar(g)
            check(lib.tt_sqdiff_rescale(ptr(ca) if has_da else None, ptr(cb) if has_db else None, ptr(gs), n, st), 'tt_sqdiff_rescale')
            want = 2.0 * scale * _f32(g) * d
            for t, w, used in ((ca, want, has_da), (cb, -want, has_db)):
                if used:
                    _check_elem('sqdiff fused gradient', t, n, w, G_REL * w.abs(), 'fused n %d g %g' % (n, g))
                else:
                    torch.cuda.synchronize()
                    assert bool(torch.isnan(t).all()), 'a NULL output was written'
            da2, db2 = _out(n), _out(n)
            check(lib.tt_sqdiff_bwd(ptr(ad), ptr(bd), ptr(gs), scale, ptr(da2) if has_da else None, ptr(db2) if has_db else None, n, st),
                  'tt_sqdiff_bwd')
            for t, w, used in ((da2, want, has_da), (db2, -want, has_db)):
                if used:
                    _check_elem('sqdiff_bwd gradient', t, n, w, G_REL * w.abs(), 'bwd n %d g %g' % (n, g))
                else:
                    torch.cuda.synchronize()
                    assert bool(torch.isnan(t).all()), 'a NULL output was written'
    assert torch.equal(ad.cpu(), a) and torch.equal(bd.cpu(), b)


@pytest.mark.parametrize('n,close', [(n, False) for n in SQ_SIZES] + [(4099, True), (5, True)])
def test_sqdiff_two_terms_match_float64(n, close):
    """tt_sqdiff2_sum_grad + tt_sqdiff2_rescale and tt_sqdiff2_bwd: both losses within 1e-6 relative; da1 = 2 s g1 (a1 - b) and
    da2 = 2 s g2 (a2 - b) within 4e-7 |want|; a NULL g counts as 0.
    db = -(da1 + da2) is a SUM of two rounded terms of either sign: each carries its three roundings relative to ITSELF and the
    sum one more, so its bar is 4e-7 (|da1| + |da2|), not 4e-7 |da1 + da2| -- where the terms cancel, no fp32 evaluation of this
    expression can meet the latter."""
    lib, ptr, check, st = _api()
    a1, a2, b = _sq_inputs(n, close)
    scale = _f32(1.0 / 37)
    d1, d2 = a1.double() - b.double(), a2.double() - b.double()
    a1d, a2d, bd = a1.cuda(), a2.cuda(), b.cuda()
    partials = torch.full((2 * MAXP,), float('nan'), dtype=torch.float64, device='cuda')
    l1, l2 = torch.full((1,), float('nan'), device='cuda'), torch.full((1,), float('nan'), device='cuda')
    # the NULL-output and scalar variants run the same loops whatever the length: at the capped-grid length one of each is enough
    big = n > 1 << 20
    pairs = ((0.5, 0.3),) if big else ((1.0, 1.0), (0.5, 0.3), (0.3, 1.0), (None, 0.5), (0.3, None))

    def wants(g1, g2):
        u = 2.0 * scale * (_f32(g1) if g1 is not None else 0.0) * d1
        v = 2.0 * scale * (_f32(g2) if g2 is not None else 0.0) * d2
        return u, v

    def check_three(key, outs, used, g1, g2, what):
        u, v = wants(g1, g2)
        for t, w, bar, on in ((outs[0], u, G_REL * u.abs(), used[0]), (outs[1], v, G_REL * v.abs(), used[1]),
                              (outs[2], -(u + v), G_REL * (u.abs() + v.abs()), used[2])):
            if on:
                _check_elem(key, t, n, w, bar, what)
            else:
                torch.cuda.synchronize()
                assert bool(torch.isnan(t).all()), 'a NULL output was written'

    # the fused forward (gradients for incoming scalars of 1) and its rescale; the rescale needs da1 and da2, db may be NULL
    for has_db in (True,) if big else (True, False):
        outs = [_out(n), _out(n), _out(n)]
        check(lib.tt_sqdiff2_sum_grad(ptr(a1d), ptr(a2d), ptr(bd), ptr(l1), ptr(l2), ptr(partials), n, scale, ptr(outs[0]), ptr(outs[1]),
                                      ptr(outs[2]) if has_db else None, st), 'tt_sqdiff2_sum_grad')
        _check_loss('sqdiff2_sum_grad loss', l1, float((d1 * d1).sum()) * scale, 1e-6, 'l1 n %d' % n)
        _check_loss('sqdiff2_sum_grad loss', l2, float((d2 * d2).sum()) * scale, 1e-6, 'l2 n %d' % n)
        check_three('sqdiff2 fused gradient', outs, (True, True, has_db), 1.0, 1.0, 'fused2 n %d' % n)
        for g1, g2 in pairs:
            cp = [t.clone() for t in outs]
            s1, s2 = _scalar(g1), _scalar(g2)
            check(lib.tt_sqdiff2_rescale(ptr(cp[0]), ptr(cp[1]), ptr(cp[2]) if has_db else None, ptr(s1), ptr(s2), n, st), 'tt_sqdiff2_rescale')
            check_three('sqdiff2 fused gradient', cp, (True, True, has_db), g1, g2, 'rescale2 n %d g %s %s' % (n, g1, g2))
    # the forward alone with every output NULL but one
    for k in () if big else range(3):
        outs = [_out(n), _out(n), _out(n)]
        used = tuple(i == k for i in range(3))
        check(lib.tt_sqdiff2_sum_grad(ptr(a1d), ptr(a2d), ptr(bd), ptr(l1), ptr(l2), ptr(partials), n, scale,
                                      *[ptr(t) if on else None for t, on in zip(outs, used)], st), 'tt_sqdiff2_sum_grad')
        check_three('sqdiff2 fused gradient', outs, used, 1.0, 1.0, 'fused2 n %d only %d' % (n, k))
    # the two-pass backward
    for g1, g2 in pairs:
        for used in ((True, True, True),) if big else ((True, True, True), (True, False, False), (False, True, False), (False, False, True)):
            outs = [_out(n), _out(n), _out(n)]
            s1, s2 = _scalar(g1), _scalar(g2)
            check(lib.tt_sqdiff2_bwd(ptr(a1d), ptr(a2d), ptr(bd), ptr(s1), ptr(s2), scale, *[ptr(t) if on else None for t, on in zip(outs, used)],
                                     n, st), 'tt_sqdiff2_bwd')
            check_three('sqdiff2_bwd gradient', outs, used, g1, g2, 'bwd2 n %d g %s %s' % (n, g1, g2))
    assert torch.equal(a1d.cpu(), a1) and torch.equal(a2d.cpu(), a2) and torch.equal(bd.cpu(), b)


def test_sqdiff_vector_entry_points_refuse_misaligned_pointers(n=64):
    """tt_sqdiff_sum_grad and tt_sqdiff2_bwd make 16-byte accesses: a pointer off by one float is the bad-argument code, and nothing is
    launched (the outputs keep their NaN)."""
    lib, ptr, check, st = _api()
    gen = torch.Generator().manual_seed(3)
    bufs = [torch.randn(n + 4, generator=gen).cuda() for _ in range(3)]
    outs = [_out(n + 4) for _ in range(3)]
    loss = torch.full((1,), float('nan'), device='cuda')
    partials = torch.zeros(2 * MAXP, dtype=torch.float64, device='cuda')
    g = _scalar(1.0)

    def off(t, on):
        return ctypes.c_void_p(t.data_ptr() + (4 if on else 0))
    for bad in range(4):                               # a, b, da, db in turn
        o = [bad == i for i in range(4)]
        rc = lib.tt_sqdiff_sum_grad(off(bufs[0], o[0]), off(bufs[1], o[1]), ptr(loss), ptr(partials), n, 1.0, off(outs[0], o[2]),
                                    off(outs[1], o[3]), st)
        assert rc == BADARG, (bad, rc)
    for bad in range(6):                               # a1, a2, b, da1, da2, db
        o = [bad == i for i in range(6)]
        rc = lib.tt_sqdiff2_bwd(off(bufs[0], o[0]), off(bufs[1], o[1]), off(bufs[2], o[2]), ptr(g), ptr(g), 1.0, off(outs[0], o[3]),
                                off(outs[1], o[4]), off(outs[2], o[5]), n, st)
        assert rc == BADARG, (bad, rc)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs) and bool(torch.isnan(loss).all())
    # aligned, the same calls go through
    check(lib.tt_sqdiff_sum_grad(ptr(bufs[0]), ptr(bufs[1]), ptr(loss), ptr(partials), n, 1.0, ptr(outs[0]), ptr(outs[1]), st), 'aligned')
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all())


# ---- transcription loss ---------------------------------------------------------------------------------------------------------------
TRN_SHAPES = [(1, 1, 1), (2, 3, 5), (1, 2, 64),      # F < 4: quarters of the frame kernel stay empty
              (3, 37, 50),                            # B T no multiple of 64
              (2, 540, 7),
              (2, 3, 40000)]                          # B T = 80000 > 65536: workgroups loop over more than one block of frames


def _trn_inputs(B, F, T):
    gen = torch.Generator().manual_seed(7 * B + 13 * F + T)
    est = torch.rand(B, F, T, generator=gen)
    tgt = 0.02 + 0.96 * torch.rand(B, F, T, generator=gen)          # fractional, as the blurred targets are
    ones = torch.rand(B, F, T, generator=gen) < 0.2
    tgt[ones] = 1.0
    if T >= 3:
        b = B - 1
        tgt[b, :, T - 1] = 1.0                                        # all ones: the scale is 0 and the weights fall back to 1
        tgt[b, :, T - 2] = 0.0                                        # all zeros
        frac = 0.02 + 0.96 * torch.rand(F, generator=gen)
        frac[::2] = 0.0 if F > 1 else frac[0]
        tgt[b, :, T - 3] = frac                                       # the only non-zero entries are fractional
    return est, tgt


@pytest.mark.parametrize('weighted', [0, 1])
@pytest.mark.parametrize('B,F,T', TRN_SHAPES)
def test_transcription_loss_matches_float64(B, F, T, weighted):
    """tt_transcription_loss_fwd / _fwd_grad / _bwd against oracle.objectives.compute_transcription_loss on float64 inputs (it keeps
    finfo(float32).eps) and its autograd gradient: loss within 2e-6 relative; the frame scale, an fp32 quotient of fp32 sums, within
    1e-6 relative where the frame has a positive target; the gradient within 1e-6 |want| + 1e-6 max |want|."""
    lib, ptr, check, st = _api()
    est, tgt = _trn_inputs(B, F, T)
    e64 = est.double().requires_grad_(True)
    want_loss = oobj.compute_transcription_loss(e64, tgt.double(), bool(weighted))
    want_grad, = torch.autograd.grad(want_loss, e64)
    want_loss = float(want_loss.detach())
    n = B * F * T
    ed, td = est.cuda(), tgt.cuda()
    partials = torch.full((2 * MAXP,), float('nan'), dtype=torch.float64, device='cuda')
    loss = torch.full((1,), float('nan'), device='cuda')

    def scale_buffer():
        return torch.full((B * T + PAD,), float('nan'), device='cuda') if weighted else None

    def check_scale(fs, what):
        if not weighted:
            return
        t64 = tgt.double()
        pos = t64.sum(-2)
        want = (1 - t64).sum(-2) / (pos + torch.finfo(torch.float32).eps)
        has = (pos > 0).reshape(-1)
        _check_elem('transcription frame scale', fs, B * T, torch.where(has, want.reshape(-1), fs[:B * T].double().cpu()),
                    torch.where(has, 1e-6 * want.reshape(-1).abs(), torch.zeros(B * T, dtype=torch.float64)), what)

    def grad_bar(w):
        return 1e-6 * w.abs() + 1e-6 * float(w.abs().max())

    fs = scale_buffer()
    check(lib.tt_transcription_loss_fwd(ptr(ed), ptr(td), ptr(loss), ptr(fs), ptr(partials), B, F, T, weighted, st), 'fwd')
    _check_loss('transcription loss', loss, want_loss, 2e-6, 'fwd %s' % ((B, F, T),))
    check_scale(fs, 'fwd frame scale')
    for g in (1.0, 0.5, 0.3):
        dest = _out(n)
        gs = _scalar(g)
        check(lib.tt_transcription_loss_bwd(ptr(ed), ptr(td), ptr(fs), ptr(gs), ptr(dest), B, F, T, weighted, st), 'bwd')
        w = _f32(g) * want_grad
        _check_elem('transcription gradient', dest, n, w, grad_bar(w), 'bwd g %g' % g)

    fs2 = scale_buffer()
    dest = _out(n)
    loss.fill_(float('nan'))
    check(lib.tt_transcription_loss_fwd_grad(ptr(ed), ptr(td), ptr(loss), ptr(fs2), ptr(partials), ptr(dest), B, F, T, weighted, st), 'fwd_grad')
    _check_loss('transcription loss', loss, want_loss, 2e-6, 'fwd_grad %s' % ((B, F, T),))
    check_scale(fs2, 'fwd_grad frame scale')
    _check_elem('transcription gradient', dest, n, want_grad, grad_bar(want_grad), 'fwd_grad')
    for g in (0.5, 0.3):                               # its backward: the stored gradient times the incoming scalar
        c = dest.clone()
        gs = _scalar(g)
        check(lib.tt_sqdiff_rescale(ptr(c), None, ptr(gs), n, st), 'tt_sqdiff_rescale')
        w = _f32(g) * want_grad
        _check_elem('transcription gradient', c, n, w, grad_bar(w), 'fwd_grad rescaled g %g' % g)
    assert torch.equal(ed.cpu(), est) and torch.equal(td.cpu(), tgt)


# ---- to_activations -------------------------------------------------------------------------------------------------------------------
ACT_SHAPES = [(2, 5, 7), (1, 37, 50), (3, 540, 9)]


def _act_inputs(B, F, T):
    """(B, 2, F, T) with magnitudes log-uniform in [1e-6, 20] (below 1e-18 the fp32 square underflows on any fp32 path), exact (0, 0)
    pairs and pairs with one component 0."""
    gen = torch.Generator().manual_seed(B + 3 * F + 5 * T)
    lo, hi = torch.log(torch.tensor(1e-6)), torch.log(torch.tensor(20.0))
    mag = torch.exp(lo + (hi - lo) * torch.rand(B, F, T, generator=gen))
    ph = 6.283185307179586 * torch.rand(B, F, T, generator=gen)
    c = torch.stack([mag * torch.cos(ph), mag * torch.sin(ph)], dim=1).contiguous()
    flat = c.view(B, 2, F * T)
    flat[:, :, 0::11] = 0.0                                            # the origin
    flat[:, 0, 1::11] = 0.0                                            # real part 0
    flat[:, 1, 2::11] = 0.0                                            # imaginary part 0
    return c, torch.randn(B, F, T, generator=gen)


@pytest.mark.parametrize('B,F,T', ACT_SHAPES)
def test_activations_match_float64(B, F, T):
    """tanh |c| within 1e-6 absolute; its gradient dact (1 - act^2) c / |c| within 2e-6 max |dact| absolute and exactly 0 at the origin."""
    lib, ptr, check, st = _api()
    c, dact = _act_inputs(B, F, T)
    c64 = c.double()
    mag = (c64[:, 0] ** 2 + c64[:, 1] ** 2).sqrt()
    want = torch.tanh(mag)
    k = torch.where(mag > 0, dact.double() * (1 - want ** 2) / mag.clamp_min(1e-300), torch.zeros_like(mag))
    want_dc = torch.stack([k * c64[:, 0], k * c64[:, 1]], dim=1)
    n = B * F * T
    cd, dd = c.cuda(), dact.cuda()
    act = _out(n)
    check(lib.tt_activations_fwd(ptr(cd), ptr(act), B, F, T, st), 'tt_activations_fwd')
    _check_elem('activations forward', act, n, want, torch.full_like(want, 1e-6), 'forward')
    dc = _out(2 * n)
    check(lib.tt_activations_bwd(ptr(cd), ptr(act), ptr(dd), ptr(dc), B, F, T, st), 'tt_activations_bwd')
    _check_elem('activations backward', dc, 2 * n, want_dc, torch.full_like(want_dc, 2e-6 * float(dact.abs().max())), 'backward')
    origin = ((c[:, 0] == 0) & (c[:, 1] == 0)).unsqueeze(1).expand(B, 2, F, T)
    assert int(origin.sum()) > 0
    assert bool((dc[:2 * n].cpu().view(B, 2, F, T)[origin] == 0).all())
    assert torch.equal(cd.cpu(), c)


@pytest.mark.parametrize('B,F,T', ACT_SHAPES)
def test_activations1_match_float64(B, F, T):
    """The one-channel form (magnitude variants): tanh c within 1e-6 absolute, dact (1 - act^2) within 2e-6 max |dact|."""
    lib, ptr, check, st = _api()
    c2, dact = _act_inputs(B, F, T)
    c = (c2[:, 0] + c2[:, 1]).contiguous()                             # signed, log-uniform size, exact zeros at the origin
    n = B * F * T
    want = torch.tanh(c.double())
    want_dc = dact.double() * (1 - want ** 2)
    cd, dd = c.cuda(), dact.cuda()
    act = _out(n)
    check(lib.tt_activations1_fwd(ptr(cd), ptr(act), n, st), 'tt_activations1_fwd')
    _check_elem('activations1 forward', act, n, want, torch.full_like(want, 1e-6), 'forward')
    dc = _out(n)
    check(lib.tt_activations1_bwd(ptr(act), ptr(dd), ptr(dc), n, st), 'tt_activations1_bwd')
    _check_elem('activations1 backward', dc, n, want_dc, torch.full_like(want_dc, 2e-6 * float(dact.abs().max())), 'backward')
