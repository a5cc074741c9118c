"""
Pins tests/x3_ref.py -- the float64 restatements the split-operand (x3) kernels are held to by tests/test_gpu_x3_parity.py -- against
torch on the CPU: float64 conv2d / conv_transpose2d / autograd for the block, the strided pair and the latent heads; torch.half
arithmetic for the pair model (subnormal halves, +-0, the edge of fp16's range); the bounds of the error model on the pair itself; and
the expected S of tt_x3_grad_scale.  No GPU.
"""

import math
import zlib

import pytest
import torch
import torch.nn.functional as F

import x3_ref as X


def _gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ---- the pair ---------------------------------------------------------------------------------------------------------------------
def _split_by_hand(v):
    """The kernel's steps one by one in torch arithmetic: hi = half(v); sc = v * 2048 (fp32); lo = half(fma(hi, -2048, sc)).  The fma is
    evaluated exactly in float64 (a half times 2048 and an fp32 value: far fewer than 53 bits apart wherever both are finite)."""
    hi = v.to(torch.float16)
    sc = v * torch.tensor(2048.0, dtype=torch.float32)
    lo = (hi.double() * -2048.0 + sc.double()).to(torch.float16)
    return hi, lo


def _edge_values():
    f = lambda bits: torch.tensor(bits, dtype=torch.int32).view(torch.float32)
    vals = [0.0, -0.0, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -26, 3 * 2.0 ** -24, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -30, 2.0 ** -15, 2.0 ** -13,
            1.0, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 65504.0, 65519.0, 65519.996, 65520.0, 65536.0, 1e5, -65504.0, -65520.0, 3e38, float('inf'),
            2.0 ** -40, 2.0 ** -149, 2.0 ** -126]
    v = torch.tensor(vals, dtype=torch.float32)
    return torch.cat([v, -v, f([0x7f7fffff, 0x00000001, 0x007fffff, 0x33800000, 0x33800001, 0x337fffff])])


def test_split_is_the_kernels_arithmetic():
    g = _gen('split')
    v = torch.cat([_edge_values(), X.pm32(g, 4096), X.pm32(g, 4096) * 2.0 ** -14, X.pm32(g, 4096) * 2.0 ** -20, X.pm32(g, 4096) * 40000,
                   torch.randn(4096, generator=g) * 2.0 ** -26])
    hi, lo = X.split(v)
    hh, hl = _split_by_hand(v)
    assert torch.equal(hi.view(torch.int16), hh.view(torch.int16))
    same = (lo.view(torch.int16) == hl.view(torch.int16)) | (lo.isnan() & hl.isnan())
    assert bool(same.all())
    # (v - hi) 2^11 is exact in fp32 wherever hi is finite: the fp32 fma of the kernel rounds once, to half
    fin = hi.isfinite()
    r = (v.double() - hi.double())[fin] * 2048
    assert torch.equal(r.float().double(), r)


def test_range_edges_of_the_pair():
    for v, finite in ((65504.0, True), (65519.996, True), (65520.0, False), (1e5, False), (-65520.0, False), (float('inf'), False)):
        hi, lo = X.split(torch.tensor([v], dtype=torch.float32))
        j = X.join(hi, lo)
        assert bool(j.isfinite()) == finite, v
        if finite:
            assert abs(float(j) - float(torch.tensor(v, dtype=torch.float32))) <= 2.0 ** -23 * abs(v)
        else:
            assert bool(j.isnan()) or bool(hi.isinf())                  # hi = inf; lo = -inf or NaN: the join is never finite
    z = torch.tensor([0.0, -0.0], dtype=torch.float32)
    hi, lo = X.split(z)
    assert torch.equal(hi.view(torch.int16), z.half().view(torch.int16))            # the sign of zero stays in hi
    assert torch.equal(X.join(hi, lo), z.double())


def test_pair_error_bound_and_where_2_pow_minus_23_holds():
    """|v - join(split(v))| <= max(2^-23 |v|, 2^-36) on every finite value in range; the relative 2^-23 is reached to within a few per cent
    (so 2^-24 would be wrong), 2^-22 is never exceeded down to 2^-14, and at 2^-15 the error is absolute: up to 2^-21 relative."""
    g = _gen('pairerr')
    worst = 0.0
    for e in range(-30, 16):
        v = (X.pm32(g, 20000) * 2.0 ** (e + 1)).clamp(-65519.996, 65519.996)      # the last binade ends at fp16's range
        err = (v.double() - X.join(*X.split(v))).abs()
        assert bool((err <= X.pair_err(v.double())).all()), e
        if e >= -13:
            worst = max(worst, float((err / v.double().abs()).max()))
    assert 0.8 * 2.0 ** -23 < worst <= 2.0 ** -23
    v = X.pm32(g, 200000) * 2.0 ** -14                                   # [2^-15, 2^-14]
    rel = float(((v.double() - X.join(*X.split(v))).abs() / v.double().abs()).max())
    assert 2.0 ** -23 < rel <= 2.0 ** -21
    v = _edge_values()
    v = v[v.abs() <= 65519.996]
    assert bool(((v.double() - X.join(*X.split(v))).abs() <= X.pair_err(v.double())).all())


def test_join_is_exact_in_fp32_and_exact_pairs_are_exact():
    g = _gen('join')
    v = torch.cat([X.pm32(g, 50000) * 2.0 ** k for k in (-20, -14, -13, -3, 0, 7, 15)])
    j = X.join(*X.split(v))
    assert torch.equal(j.float().double(), j)
    for scale in (1.0, 1 / math.sqrt(288), 2.0 ** -12):
        w = X.exact_pairs(g, 3000, scale=scale)
        assert X.is_exact(w) and bool((w.abs() >= 0.5 * 2.0 ** round(math.log2(scale))).all())
    assert not X.is_exact(X.general(g, 3000))
    with pytest.raises(AssertionError):
        X.exact_pairs(g, 8, scale=2.0 ** -14)


def test_x3_layout_round_trip():
    g = _gen('layout')
    x = X.general(g, 2, 16, 3, 5)
    t = X.to_x3(x)
    assert t.shape == (2, 3, 5, 2, 16) and t.dtype == torch.float16 and t.is_contiguous()
    hi, lo = X.split(x)
    assert torch.equal(t[1, 2, 4, 0], hi[1, :, 2, 4]) and torch.equal(t[1, 2, 4, 1], lo[1, :, 2, 4])
    assert torch.equal(X.from_x3(t), X.join(hi, lo))
    assert torch.equal(X.pack(x).view(torch.int16), t.view(torch.int16))
    assert torch.equal(X.unpack(t).double(), X.from_x3(t))
    sc = (2.0 ** 20, 2.0 ** -20)
    xs = x * 1e-7
    t2 = X.pack(xs, sc)
    assert torch.equal(t2.view(torch.int16), X.to_x3(xs * 2.0 ** 20).view(torch.int16))
    assert torch.equal(X.unpack(t2, sc).double(), X.from_x3(t2) * 2.0 ** -20)


# ---- tt_x3_grad_scale -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('amax,S', [
    (1.0, 2.0 ** 8), (1.0 - 2.0 ** -24, 2.0 ** 9), (1.0 + 2.0 ** -23, 2.0 ** 8), (2.0, 2.0 ** 7), (2.0 - 2.0 ** -23, 2.0 ** 8),
    (256.0, 1.0), (511.9, 1.0), (512.0, 0.5), (255.99, 2.0), (2.0 ** -20, 2.0 ** 28), (1e-7, 2.0 ** 32),
    (2.0 ** -126, 2.0 ** 120), (2.0 ** -127, 2.0 ** 120), (2.0 ** -149, 2.0 ** 120), (2.0 ** -112, 2.0 ** 120), (2.0 ** -111, 2.0 ** 119),
    (3.4e38, 2.0 ** -119), (2.0 ** 127, 2.0 ** -119), (0.0, 1.0), (float('inf'), 1.0), (float('nan'), 1.0)])
def test_grad_scale(amax, S):
    dy = torch.full((37,), 0.25, dtype=torch.float32) * (0.0 if amax == 0 else min(1.0, abs(amax)) if math.isfinite(amax) else 1.0) * 0.5
    dy[11] = -amax
    s, inv = X.grad_scale(dy)
    assert (s, inv) == (S, 1.0 / S)
    if math.isfinite(amax) and amax >= 2.0 ** -112 and amax < 2.0 ** 127:
        assert 2.0 ** 8 <= amax * s < 2.0 ** 9
    # both are fp32 numbers (the kernel builds them from the exponent field)
    assert float(torch.tensor(s, dtype=torch.float32)) == s and float(torch.tensor(inv, dtype=torch.float32)) == inv


def test_grad_scale_nan_beats_inf_and_sign_is_ignored():
    assert X.grad_scale(torch.tensor([1.0, float('inf'), float('nan')])) == (1.0, 1.0)
    assert X.grad_scale(torch.tensor([-300.0, 2.0])) == (1.0, 1.0)
    assert X.grad_scale(torch.tensor([-0.0, 0.0])) == (1.0, 1.0)


# ---- the block --------------------------------------------------------------------------------------------------------------------
def _block(C, d, B, H, T):
    g = _gen('block', C, d, H, T)
    x = X.from_x3(X.to_x3(X.general(g, B, C, H, T)))
    w1 = X.general(g, C, C, 3, 3, scale=1 / math.sqrt(9 * C))
    w2 = X.general(g, C, C, 1, 1, scale=1 / math.sqrt(C))
    b1, b2 = X.general(g, C, scale=0.3), X.general(g, C, scale=0.3)
    dy = X.from_x3(X.to_x3(X.general(g, B, C, H, T)))
    return x, w1, b1, w2, b2, dy


@pytest.mark.parametrize('C,d,H,T', [(4, 1, 1, 1), (8, 2, 2, 3), (16, 3, 3, 4), (16, 1, 5, 9), (32, 2, 4, 7)])
def test_block_forward_and_backward_against_autograd(C, d, H, T, B=2):
    x, w1, b1, w2, b2, dy = _block(C, d, B, H, T)
    xr = x.clone().requires_grad_(True)
    p = [t.double().requires_grad_(True) for t in (w1, b1, w2, b2)]
    h1t = F.elu(F.conv2d(xr, p[0], p[1], padding=d, dilation=d))
    yt = F.elu(F.conv2d(h1t, p[2], p[3])) + xr
    h1, a1, bh = X.rb_stage1(x, w1, b1, d)
    _close(h1, h1t.detach())
    y, a2, by = X.rb_stage2(h1, x, w2, b2)
    _close(y, yt.detach())
    y2, by2 = X.rb_fwd(x, w1, b1, w2, b2, d)
    assert torch.equal(y2, y) and bool((by2 >= by).all()) and bool((bh > 0).all())
    _close(X.level_fwd(x, [(w1, b1, w2, b2, d)] * 2), X.rb_fwd(y, w1, b1, w2, b2, d)[0])
    gx, gw1, gb1, gw2, gb2 = torch.autograd.grad(yt, [xr] + p, dy)
    for g1_used in (None, 'own'):
        out = X.rb_bwd(x, h1, dy, w1, w2, b2, d)
        if g1_used:
            out = X.rb_bwd(x, h1, dy, w1, w2, b2, d, g1_used=out['g1'][0])
        for name, want in (('dx', gx), ('dw1', gw1), ('db1', gb1), ('dw2', gw2.reshape(C, C)), ('db2', gb2)):
            _close(out[name][0], want)
            bar = out[name][1] + torch.zeros_like(want)
            # a tap with no pixel inside the image sums nothing: value and bar are exactly 0 there
            assert bool((bar[want != 0] > 0).all()) and bool((bar[want == 0] == 0).all()) and bool((bar < 1e-3 * (1 + want.abs().max())).all()), name
    # the bar of a sum counts only taps inside the image: one pixel has one tap
    if (H, T) == (1, 1):
        assert float(X.conv3(x, w1, b1, d)[2].max()) == C


# ---- the strided pair and the latent heads ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,H,T', [(8, 4, 1), (16, 5, 3), (32, 7, 2), (16, 6, 5)])
def test_sconv_against_torch(C, H, T, B=2):
    g = _gen('sconv', C, H, T)
    x, w, b = X.general(g, B, C, H, T).double(), X.general(g, 2 * C, C, 4, 1, scale=0.1), X.general(g, 2 * C, scale=0.3)
    y, v, beta = X.stride_fwd('sconv', C, x, w, b)
    want = F.elu(F.conv2d(x, w.double(), b.double(), stride=(2, 1)))
    _close(y, want)
    assert y.shape == (B, 2 * C, (H - 4) // 2 + 1, T) and bool((beta > 0).all())


@pytest.mark.parametrize('C,H,T,op', [(16, 1, 3, 0), (16, 2, 1, 1), (32, 2, 5, 1), (32, 1, 2, 0)])
def test_tconv_against_torch(C, H, T, op, B=2):
    g = _gen('tconv', C, H, T, op)
    x, w, b = X.general(g, B, 2 * C, H, T).double(), X.general(g, 2 * C, C, 4, 1, scale=0.1), X.general(g, C, scale=0.3)
    y, v, beta = X.stride_fwd('tconv', C, x, w, b, out_pad=op)
    want = F.elu(F.conv_transpose2d(x, w.double(), b.double(), stride=(2, 1), output_padding=(op, 0)))
    _close(y, want)
    assert y.shape == (B, C, 2 * H + 2 + op, T)


@pytest.mark.parametrize('C,D,E,T', [(32, 32, 1, 3), (32, 32, 3, 5), (64, 128, 2, 2)])
@pytest.mark.parametrize('bias', [True, False])
def test_latent_heads_against_torch(C, D, E, T, bias, B=2):
    g = _gen('lat', C, D, E, T)
    x = X.general(g, B, C, E, T).double()
    w = X.general(g, D, C, E, 1, scale=1 / math.sqrt(C * E))
    b = X.general(g, D, scale=0.3) if bias else None
    z, beta = X.lat_encode(x, w, b)
    want = F.conv2d(x, w.double(), None if b is None else b.double())[:, :, 0]
    _close(z, want)
    wd = X.general(g, D + 1, C, E, 1, scale=1 / math.sqrt(D))
    bd = X.general(g, C, scale=0.3) if bias else None
    zz = X.general(g, B, D + 1, T)
    for Dz, fill in ((D + 1, 0.0), (D, 0.75)):
        zin = zz[:, :Dz].contiguous()
        y, v, beta = X.lat_decode(zin, Dz, fill, wd, bd)
        full = zz.double().clone()
        if Dz == D:
            full[:, D] = fill
        want = F.elu(F.conv_transpose2d(full.unsqueeze(2), wd.double(), None if bd is None else bd.double()))
        _close(y, want)
        assert y.shape == (B, C, E, T) and bool((beta > 0).all())


def test_prod_bar_terms():
    """The bar of a product sum shrinks by exactly n 2^-23 S (1 + 2^-10) per operand that is a pair, and never below the dropped lo x lo term."""
    v, S = torch.tensor([0.5], dtype=torch.float64), torch.tensor([3.0], dtype=torch.float64)
    b2, b1, b0 = (float(X.prod_bar(v, S, 10, n)) for n in (2, 1, 0))
    assert abs((b2 - b1) - (1 + 2.0 ** -10) * 2.0 ** -23 * 3.0) < 1e-20 and abs((b1 - b0) - (b2 - b1)) < 1e-20
    assert b0 > 2.0 ** -22 * 3.0 + 10 * 2.0 ** -24 * 3.0
