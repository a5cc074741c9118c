"""
Float64 restatements of the split-operand ("x3") entry points of include/ttrap.h (csrc/conv_x3.hip) and the error model their kernels are
held to.  tests/test_x3_restatement.py pins this file against torch where no GPU is needed; tests/test_gpu_x3_parity.py holds the kernels
to it.  Built on tests/conv_ref.py (gather + einsum: every value comes with S, the sum of absolute products, and K, the number of
products that land in the image); the guarded arena is tests/cl16_ref.py's.

Restated: tt_x3_pack / _unpack / _pack_scaled / _unpack_scaled (pack, unpack), tt_x3_grad_scale (grad_scale), tt_x3_rb_fwd /
tt_x3_rb_fwd_train / tt_x3n_rb_fwd (rb_stage1, rb_stage2: the narrow block is the same function of its operands), tt_x3_level_fwd /
tt_x3n_level_fwd (level_fwd: the blocks in sequence), tt_x3_rb_bwd (rb_bwd), tt_x3_sconv_fwd / tt_x3_tconv_fwd (stride_fwd),
tt_x3_latent_encode / _decode (lat_encode, lat_decode).

The pair.  An fp32 value v is held as two IEEE halves
    hi = fp16(v)            lo = fp16((v - hi) 2^11)            v ~ hi + lo 2^-11
(round to nearest even both times; (v - hi) 2^11 is exact in fp32, so the kernels' fma form rounds once).  ``split`` / ``join``
restate that bit for bit, subnormal halves included.  Layout "x3": [B][H][T][2][C] halves (``to_x3`` / ``from_x3``).

How exact a pair is (the header said 2^-23 relative, tests/test_gpu_x3.py asserts 2^-22).  Let 2^e <= |v| < 2^(e+1), e >= -14.  hi is v
rounded to 11 bits: |v - hi| <= 2^(e-11), so |(v - hi) 2^11| <= 2^e.  If that value equals 2^e it is a half; otherwise it lies below 2^e,
where halves are spaced 2^(e-11) or closer, and rounding it moves it by at most 2^(e-12).  Back in units of v: 2^(e-23) <= 2^-23 |v|.
lo is a NORMAL half only while its own spacing 2^(e-11) is at least that of the subnormals, 2^-24, i.e. e >= -13; below, rounding lo
moves it by up to 2^-25 whatever its size, 2^-36 in units of v -- and for |v| < 2^-14 hi is subnormal too, |v - hi| <= 2^-25,
lo <= 2^-14 and the same 2^-36 holds.  So
    |v - (hi + lo 2^-11)|  <=  max(2^-23 |v|, 2^-36)                                      (``pair_err``)
2^-23 relative holds from |v| = 2^-13 upwards, 2^-22 relative from 2^-14, and below that the error is absolute.  The header's 2^-23 is
right for a correctly rounded split and stays; what it said about the lower end ("2^-22 relative only above ~2^-15") was off by one
binade and is corrected there.  A value with at most 22 significant bits (the two lowest of fp32's 24 zero) and |v| >= 2^-13 is held
EXACTLY: (v - hi) 2^11 then has at most 11 bits.  ``exact_pairs`` draws such values.  The join hi + lo 2^-11 is exact in fp32 (its bits
span at most 2^e .. 2^(e-23)), so an x3 tensor handed to a kernel IS a tensor of exactly known fp32 values: the restatements take
``from_x3`` of the bytes the kernel reads, and only operands the kernels split themselves -- weights, fp32 planar inputs, their own
intermediates -- carry a split term.

A product sum (``prod_bar``).  The kernels evaluate W x = Whi xhi + 2^-11 (Whi xlo + Wlo xhi) on the 16-bit matrix pipe with fp32
accumulators: ``am`` takes the bias and the K products Whi xhi, ``al`` the 2 K cross products (in units of 2^11), and the result is one
fma, al 2^-11 + am.  Products of two halves are exact in fp32.  With u = 2^-24 and S = sum |W| |x| (+ |bias|), to first order:
    K u S                      the accumulation of am, in any order (matrix instruction, partial sums of workgroups, a reduce)
    2^-9 K u S                 the accumulation of al: 2 K terms, sum of magnitudes <= 2 S 2^11 because |lo| <= 2^e <= |v|; times 2^-11
    u |v|                      the final fma
    2^-22 S                    the dropped term Wlo xlo 2^-22, |lo| <= |v| on both sides
    n 2^-23 S                  n = how many of the two operands are split by the kernel from values that are not exactly pairs
second-order terms are covered by a factor (1 + 2^-10) on the whole.  On top, exactly as tests/test_gpu_conv_parity.py:
    ELU                        + 4 u max(1, |a|)        (__expf(a) - 1)
    ELU' through exp           dy min(exp(a2), 1) with a2 known to beta: |dy| (beta + 2 u) (exp is 1-Lipschitz for a <= 0) + u |g|
    ELU' through the output    t min(h + 1, 1): u |t| for the h + 1, u |g| for the product
    residual / incoming add    + u |result|
    a stored pair              + pair_err(|want| + beta)
ELU, both ELU' forms and the split are continuous: no element is excluded anywhere.
"""

import torch

import conv_ref as R
from cl16_ref import Arena, FILL_BIG, FILL_NAN, GUARD, U, elu, elu_gate, pm32      # noqa: F401  (the GPU file takes them from here)

LO = 2048.0
EP, EABS = 2.0 ** -23, 2.0 ** -36
F16_MAX = 65504.0


# ---- the pair ---------------------------------------------------------------------------------------------------------------------
def split(v):
    """fp32 tensor -> (hi, lo) halves, bit for bit what ``split`` of csrc/conv_x3.hip gives: hi = fp16(v), lo = fp16(fma(hi, -2^11, v 2^11)).
    v 2^11 is an fp32 product (inf beyond FLT_MAX / 2^11), the fma is exact for every finite hi and rounds once to half."""
    v = v.float()
    hi = v.half()
    sc = (v * LO).double()                                   # fp32 product, exact unless it overflows
    with torch.no_grad():
        lo = (sc - hi.double() * LO).half()                  # inf - inf = NaN like the fma
    return hi, lo


def join(hi, lo):
    """(hi, lo) halves -> float64 hi + lo 2^-11: exact, and exactly what the kernels' fp32 fma returns for every pair ``split`` makes."""
    return hi.double() + lo.double() / LO


def pair_err(v):
    """Bound on |v - join(split(v))| for |v| <= 65504 (module docstring)."""
    return (EP * v.abs()).clamp_min(EABS)


def to_x3(v):
    """(B, C, H, T) fp32 -> the x3 tensor [B][H][T][2][C] of halves."""
    hi, lo = split(v)
    return torch.stack([hi.permute(0, 2, 3, 1), lo.permute(0, 2, 3, 1)], 3).contiguous()


def from_x3(t):
    """x3 tensor (B, H, T, 2, C) -> (B, C, H, T) float64: the fp32 value every pixel's pair holds."""
    return join(t[:, :, :, 0], t[:, :, :, 1]).permute(0, 3, 1, 2).contiguous()


def exact_pairs(gen, *shape, scale=1.0):
    """fp32 values in +-[0.5, 1) times the power of two nearest ``scale`` that a pair holds EXACTLY: the two lowest significand bits are
    zero (22 significant bits) and |v| >= 2^-13 -- the constraint; asserted here.  With such operands every input-side split term of
    prod_bar vanishes, and a lost lo plane or cross term (2^-11 relative per product) is far outside the bar."""
    import math
    m = (0.5 + 0.5 * torch.rand(*shape, generator=gen)).float()
    m = (m.view(torch.int32) & ~3).view(torch.float32)
    sign = (torch.randint(0, 2, shape, generator=gen) * 2 - 1).float()
    v = m * sign * 2.0 ** round(math.log2(scale))
    assert float(v.abs().min()) >= 2.0 ** -13
    return v


def general(gen, *shape, scale=1.0):
    """General fp32 values, uniform in +-[0.5, 1] times ``scale`` (weights: scale = 1 / sqrt(K), as in the fp32 file)."""
    return pm32(gen, *shape) * scale


def is_exact(v):
    """Whether every element of the fp32 tensor is held exactly by its pair."""
    hi, lo = split(v)
    return bool((join(hi, lo) == v.double()).all())


def pack(x, scale=None):
    """tt_x3_pack / tt_x3_pack_scaled: x3 = split(x * scale[0]) (an fp32 product)."""
    x = x.float()
    return to_x3(x if scale is None else x * torch.tensor(scale[0], dtype=torch.float32))


def unpack(t, scale=None):
    """tt_x3_unpack / tt_x3_unpack_scaled: y = join(x3) * scale[1] as fp32."""
    y = from_x3(t).float()
    return y if scale is None else y * torch.tensor(scale[1], dtype=torch.float32)


def grad_scale(dy):
    """tt_x3_grad_scale: (S, 1 / S) with S = 2^se the power of two that puts abs-max(dy) into [2^8, 2^9): se = 8 - e for abs-max in
    [2^e, 2^(e+1)), e read from the exponent field (a subnormal abs-max reads e = -127), clamped to +-120; S = 1 for an all-zero dy and
    for one with an inf or a NaN (|v| as bits: NaN sorts above inf)."""
    m = int((dy.float().contiguous().view(torch.int32) & 0x7fffffff).max())
    se = 0
    if m != 0 and m < 0x7f800000:
        se = max(-120, min(120, 8 - ((m >> 23) - 127)))
    return 2.0 ** se, 2.0 ** -se


# ---- bars -------------------------------------------------------------------------------------------------------------------------
def prod_bar(v, S, K, nsplit):
    """Bar of one three-term product sum (module docstring).  S includes |bias| where the bias is the accumulator's initial value."""
    return (1 + 2.0 ** -10) * ((K * (1 + 2.0 ** -9)) * U * S + (2.0 ** -22 + nsplit * EP) * S) + U * v.abs()


def elu_bar(a):
    return 4 * U * a.abs().clamp_min(1.0)


def stored(v, beta):
    """Bar of a value that leaves as a pair when its fp32 form is known to beta."""
    return beta + pair_err(v.abs() + beta)


# ---- the residual block -----------------------------------------------------------------------------------------------------------
def conv3(x, w, b, d):
    """W (*)_d x + b, x (B, C, H, T), w (Co, C, 3, 3): (v, S incl. |b|, K (H, T))."""
    B, Cn, H, T = x.shape
    fa = R.forward_args('conv', Cn, w.size(0), 3, 3, 1, d, d, d)
    _, v, S = R.conv2d(x, w.reshape(-1), b, None, Hout=H, **fa)
    if b is not None:
        S = S + b.double().abs().view(1, -1, 1, 1)
    return v, S, Cn * R.tap_count(H, H, T, 3, 3, 1, d, d, d, d, 0)


def rb_stage1(x, w1, b1, d, nsplit=1):
    """h1 = ELU(W1 (*)_d x + b1) -> (h1, a1, beta): beta the bar of the fp32 h1 (``stored(h1, beta)`` that of the pair).  nsplit: 1 for an
    x3 input (only W1 is split by the kernel), 2 for a general fp32 planar input; one less with exact_pairs weights."""
    a1, S, K = conv3(x, w1, b1, d)
    return elu(a1), a1, prod_bar(a1, S, K, nsplit) + elu_bar(a1)


def rb_stage2(h1, x, w2, b2, carry=None, nsplit=1):
    """y = ELU(W2 h1 + b2) + x, w2 (C, C) -> (y, a2, beta of the fp32 y).  carry: the bar of the h1 the kernel used where that is not
    observable (taken through |W2|)."""
    w2 = w2.double().reshape(w2.size(0), -1)
    a2 = torch.einsum('oc,bcht->boht', w2, h1) + b2.double().view(1, -1, 1, 1)
    S = torch.einsum('oc,bcht->boht', w2.abs(), h1.abs()) + b2.double().abs().view(1, -1, 1, 1)
    beta = prod_bar(a2, S, h1.size(1), nsplit)
    if carry is not None:
        beta = beta + torch.einsum('oc,bcht->boht', w2.abs(), carry)
    y = elu(a2) + x
    return y, a2, beta + elu_bar(a2) + U * y.abs()


def rb_fwd(x, w1, b1, w2, b2, d, nsplit_x=0, nsplit_w=1):
    """tt_x3_rb_fwd / tt_x3n_rb_fwd: (y, beta of the fp32 y); h1 is not observable, its pair's bar is carried."""
    h1, _, bh = rb_stage1(x, w1, b1, d, nsplit_x + nsplit_w)
    y, _, by = rb_stage2(h1, x, w2, b2, carry=stored(h1, bh), nsplit=nsplit_w)
    return y, by


def level_fwd(x, blocks):
    """tt_x3_level_fwd / tt_x3n_level_fwd in float64: blocks = [(w1, b1, w2, b2, d), ...] (the value only; the GPU file holds the level
    calls bit for bit to block-by-block calls, which it holds to rb_fwd)."""
    for w1, b1, w2, b2, d in blocks:
        x = rb_fwd(x, w1, b1, w2, b2, d)[0]
    return x


def rb_bwd(x, h1, dy, w1, w2, b2, d, g1_used=None, nsplit_w=1):
    """tt_x3_rb_bwd on the values the three x3 tensors hold (dy still carrying the factor S: every result here carries it too, the caller
    multiplies value and bar by 1 / S, exact).  g1_used: the g1 the kernel stored in ws (from_x3), fed to dx and dW1 in place of the
    restatement's own; None: the restatement's own with its bar carried.
    The sums over pixels (K = B H T, for dW1 restricted by the tap): db1 and db2 add K fp32 values in a tree of lanes, waves, dumps and the
    reduce -- at most K - 1 roundings on any path whatever its shape (an empty lane or dump adds an exact zero): K u S.  dW2 and dW1 are
    product sums (prod_bar) in which EVERY wave ends with its own fma al 2^-11 + am before the dumps are added: the fmas together round by
    at most u times the sum of the |partials| <= u S, one more than the single fma prod_bar counts: K + 1.  The 1 / S factor is exact.
    -> dict name -> (value, bar): g1 (fp32 form; ``stored`` for the pair in ws), dx (fp32 form), dw1, db1, dw2, db2 (before the +=: add
    U (|previous| + |result|) for it)."""
    B, Cn, H, T = x.shape
    npix = B * H * T
    w2 = w2.double().reshape(Cn, Cn)
    aw2 = w2.abs()
    b2 = b2.double().view(1, -1, 1, 1)
    a2 = torch.einsum('oc,bcht->boht', w2, h1) + b2
    ba2 = prod_bar(a2, torch.einsum('oc,bcht->boht', aw2, h1.abs()) + b2.abs(), Cn, nsplit_w)
    g2 = dy * torch.exp(a2.clamp(max=0.0))
    bg2 = dy.abs() * (ba2 + 2 * U) + U * g2.abs()
    out = {}
    # db2 sums the fp32 g2; dW2 and W2^T g2 take its pair
    out['db2'] = (g2.sum((0, 2, 3)), bg2.sum((0, 2, 3)) + npix * U * g2.abs().sum((0, 2, 3)))
    bg2p = stored(g2, bg2)
    dw2 = torch.einsum('boht,bcht->oc', g2, h1)
    S2 = torch.einsum('boht,bcht->oc', g2.abs(), h1.abs())
    out['dw2'] = (dw2, prod_bar(dw2, S2, npix + 1, 0) + torch.einsum('boht,bcht->oc', bg2p, h1.abs()))
    t = torch.einsum('oc,boht->bcht', w2, g2)
    bt = prod_bar(t, torch.einsum('oc,boht->bcht', aw2, g2.abs()), Cn, nsplit_w) + torch.einsum('oc,boht->bcht', aw2, bg2p)
    gate = elu_gate(h1)
    g1 = t * gate
    bg1 = bt * gate + U * t.abs() + U * g1.abs()
    out['g1'] = (g1, bg1)
    out['db1'] = (g1.sum((0, 2, 3)), bg1.sum((0, 2, 3)) + npix * U * g1.abs().sum((0, 2, 3)))
    if g1_used is None:
        g1_used, carry = g1, stored(g1, bg1)
    else:
        carry = None
    da = R.dgrad_args('conv', Cn, Cn, 3, 3, 1, d, d, d)
    _, c, Sx = R.conv2d(g1_used, w1.reshape(-1), None, None, Hout=H, **da)
    Kx = Cn * R.tap_count(H, H, T, 3, 3, 1, d, d, d, d, 0)
    dx = dy + c
    bdx = prod_bar(c, Sx, Kx, nsplit_w) + U * dx.abs()
    dw1, S1, K1, _, _ = R.conv2d_wgrad(x, g1_used, KH=3, KW=3, stride_h=1, dil_h=d, dil_w=d, pad_h=d, pad_w=d)
    bdw1 = prod_bar(dw1, S1, (K1 + 1).view(1, 1, 3, 3).double(), 0)
    if carry is not None:
        aw1 = w1.double().abs()
        bdx = bdx + R.conv2d(carry, aw1.reshape(-1), None, None, Hout=H, **da)[1]
        bdw1 = bdw1 + R.conv2d_wgrad(x.abs(), carry, KH=3, KW=3, stride_h=1, dil_h=d, dil_w=d, pad_h=d, pad_w=d)[0]
    out['dx'] = (dx, bdx)
    out['dw1'] = (dw1, bdw1)
    return out


# ---- the strided pair -------------------------------------------------------------------------------------------------------------
def stride_layer(kind, C):
    """sconv: Conv2d(C, 2C, (4,1), stride (2,1)); tconv: ConvTranspose2d(2C, C, (4,1), stride (2,1)) -- C as the entry points take it."""
    return ('conv', C, 2 * C, 4, 1, 2, 1, 0, 0) if kind == 'sconv' else ('tconv', 2 * C, C, 4, 1, 2, 1, 0, 0)


def stride_fwd(kind, C, x, w, b, out_pad=0, nsplit=1):
    """tt_x3_sconv_fwd / tt_x3_tconv_fwd on x (B, Cin, H, T): (y = ELU(v), v, beta of the fp32 y)."""
    layer = stride_layer(kind, C)
    H, T = x.size(2), x.size(3)
    Hout = R.out_rows(layer[0], H, 4, 2, 1, 0, out_pad)
    fa = R.forward_args(*layer)
    y, v, S = R.conv2d(x, w.reshape(-1), b, None, Hout=Hout, act=R.ACT_ELU, **fa)
    S = S + b.double().abs().view(1, -1, 1, 1)
    K = layer[1] * R.tap_count(H, Hout, T, 4, 1, 2, 1, 1, 0, 0, fa['transposed'])
    return y, v, prod_bar(v, S, K, nsplit) + elu_bar(v)


# ---- the latent heads -------------------------------------------------------------------------------------------------------------
def lat_encode(x, w, b, nsplit=1):
    """tt_x3_latent_encode: x (B, C, E, T) the values of the x3 embedding, w (D, C, E, 1) -> (z (B, D, T), beta)."""
    wd = w.double()[..., 0]
    z = torch.einsum('dce,bcet->bdt', wd, x)
    S = torch.einsum('dce,bcet->bdt', wd.abs(), x.abs())
    if b is not None:
        z = z + b.double().view(1, -1, 1)
        S = S + b.double().abs().view(1, -1, 1)
    return z, prod_bar(z, S, w.size(1) * w.size(2), nsplit)


def lat_decode(z, Dz, fill, w, b, nsplit=2):
    """tt_x3_latent_decode: z (B, Dz, T) fp32 (split by the kernel), w (D + 1, C, E, 1) -> (y = ELU(v) (B, C, E, T), v, beta of the fp32 y).
    The extra input channel D (z's own where Dz = D + 1, else the constant ``fill``) enters as ONE fp32 fma on the finished sum."""
    D = w.size(0) - 1
    wd = w.double()[..., 0]
    zd = z.double()
    v = torch.einsum('dce,bdt->bcet', wd[:D], zd[:, :D])
    S = torch.einsum('dce,bdt->bcet', wd[:D].abs(), zd[:, :D].abs())
    if b is not None:
        v = v + b.double().view(1, -1, 1, 1)
        S = S + b.double().abs().view(1, -1, 1, 1)
    beta = prod_bar(v, S, D, nsplit)
    zx = zd[:, D] if Dz > D else torch.full((z.size(0), z.size(2)), float(torch.tensor(fill, dtype=torch.float32)), dtype=torch.float64)
    v = v + torch.einsum('ce,bt->bcet', wd[D], zx)
    beta = beta + U * v.abs()
    return elu(v), v, beta + elu_bar(v)
