"""
Float64 restatements of the 16-bit channels-last ("cl16") entry points of include/ttrap.h, and the guarded arena their operands are
handed over in.  tests/test_cl16_restatement.py pins this file against torch (and tests the arena) where no GPU is needed;
tests/test_gpu_cl16_parity.py holds the kernels to it.  Built on tests/conv_ref.py: the convolutions are its gather + einsum, so every
value comes with S, the sum of absolute products, and K, the number of products restricted to the taps that land in the image.

Restated here: tt_wide_pack / tt_wide_unpack, tt_gate16, tt_skip_join16_fwd / _bwd, tt_scaled_add16, tt_dot16, the eight edge
convolutions tt_convin16[_1]_* / tt_convout16[_1]_*, the strided pair tt_sconv16_* / tt_tconv16_*, and the latent heads tt_latent16_*.
The residual block's two stages are restated here (rb_stage1, rb_stage2); its backward is a chain of einsums and conv_ref calls written
out in the GPU file next to the bars it carries (dA2, dA1 and a recomputed h1 are rounded inside the kernels from sums that are only
known to within a bar: boundary_spread).

Layout.  A cl16 tensor is [B][H][T][C] in memory; the restatements work on the logical (B, C, H, T) float64 values, ``to_cl`` / ``from_cl``
convert.  Rounding points: 16-bit round-to-nearest-even where the header says a value is stored or used as a matrix operand -- every
cl16 output, the operand z of the latent heads, the gated input of tt_latent16_contract / _wgrad with gy, the gated gradient of the
strided layers.  With the operands of the GPU
file (16-bit values in +-[0.5, 1]) the gate g * min(y + 1, 1) is exact in fp32 (y + 1 and the product fit 24 bits), and z is an input:
both roundings are therefore applied to exactly known values, ``round16`` reproduces them bit for bit and no restatement of this file
has to mark elements near a rounding boundary.
"""

import ctypes
import math

import torch

import conv_ref as R

U = 2.0 ** -24                       # unit roundoff of fp32
GUARD = 128                          # bytes of guard in front of and behind every window
FILL_NAN, FILL_BIG = 0xFF, 0x46      # every byte 0xFF: NaN in bf16, fp16 and fp32; 0x46: 12672 (bf16), 6.27 (fp16), 12689.6 (fp32)
ACT_NONE, ACT_ELU, ACT_RELU, ACT_SIGMOID = R.ACT_NONE, R.ACT_ELU, R.ACT_RELU, R.ACT_SIGMOID


def roundoff16(dtype):
    """Unit roundoff of the element type: round-to-nearest of a value v to p significant bits moves it by at most 2^-p |v| (bf16: p = 8,
    fp16: p = 11)."""
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11


def round16(v, dtype):
    """Round-to-nearest-even to the element type, back in float64.  Through fp32, like the kernels: exact for every value that fp32
    holds exactly, which is all this file rounds."""
    return v.float().to(dtype).double()


def half_spacing16(dtype):
    """Half the spacing of the element type's subnormals, 2^(emin - p): what round-to-nearest moves a value below the smallest normal
    number by (fp16: below 2^-14 = 6.1e-5, where a gate close to 0 times a cancelling sum lands; bf16: below 2^-126, never reached)."""
    return 2.0 ** -134 if dtype == torch.bfloat16 else 2.0 ** -25


def bar16(want, beta, dtype):
    """Bar of a stored 16-bit result whose fp32 value carries the bar beta: beta + e (|want| + beta), e the unit roundoff -- or, in the
    subnormal range where the spacing no longer shrinks with the value, beta + half that spacing."""
    return beta + (roundoff16(dtype) * (want.abs() + beta)).clamp_min(half_spacing16(dtype))


def to_cl(v, dtype):
    """(B, C, H, T) values -> the [B][H][T][C] tensor of the element type."""
    return v.permute(0, 2, 3, 1).contiguous().to(dtype)


def from_cl(t):
    """[B][H][T][C] tensor -> (B, C, H, T) float64."""
    return t.double().permute(0, 3, 1, 2).contiguous()


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def pm32(gen, *shape):
    """fp32, uniform in +-[0.5, 1]"""
    return (0.5 + 0.5 * torch.rand(*shape, generator=gen)) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1).float()


def pm16(gen, dtype, *shape):
    """uniform in +-[0.5, 1], rounded to the element type"""
    return pm32(gen, *shape).to(dtype)


def exact_weights(gen, K, *shape):
    """+-[0.5, 1) with a 4-bit significand times the power of two nearest 1 / sqrt(K): exact in bf16 and fp16, so a kernel's own rounding
    of its weights is the identity and a product with a 16-bit operand is exact in fp32.  One dropped, doubled or mis-addressed product
    moves a sum by at least 0.25 / sqrt(K) in these units."""
    m = torch.randint(8, 16, shape, generator=gen).float() / 16
    sign = (torch.randint(0, 2, shape, generator=gen) * 2 - 1).float()
    return m * sign * 2.0 ** round(math.log2(1 / math.sqrt(K)))


# ---- the arena --------------------------------------------------------------------------------------------------------------------
class Arena:
    """The operands of one call as windows of ONE flat byte buffer filled with ``fill``.  A window starts on a 16-byte boundary plus
    ``shift`` bytes and has at least GUARD bytes of the fill in front of it and behind it.  kinds: 'in' (bit-unchanged afterwards), 'out'
    (the fill before; written and finite afterwards), 'acc' (a non-zero pattern before -- the += contract -- finite afterwards), 'scratch'
    (anything afterwards).  An 'out' element counts as written when its bytes differ from the fill: a kernel that legitimately stored
    exactly the fill's value (12672 in bf16, 6.27 in fp16 under 0x46) would be reported as unwritten -- out of reach of operands in
    +-[0.5, 1] with scaled weights, to be remembered with other operands.  Device-agnostic: tests/test_cl16_restatement.py runs it on the CPU with torch writes in place of a kernel."""

    def __init__(self, fill=FILL_NAN, device='cpu'):
        self.fill, self.device = fill, device
        self.win = {}
        self.pos = GUARD

    def _add(self, name, kind, dtype, shape, vals, shift, align=16):
        item = torch.empty((), dtype=dtype).element_size()
        assert shift % item == 0 and align % 16 == 0
        nbytes = int(math.prod(shape)) * item
        start = (self.pos + align - 1) // align * align + shift
        if vals is not None:
            assert vals.dtype == dtype and tuple(vals.shape) == tuple(shape)
            vals = vals.contiguous().reshape(-1).view(torch.uint8).clone()
        self.win[name] = dict(start=start, nbytes=nbytes, kind=kind, dtype=dtype, shape=tuple(shape), vals=vals, item=item)
        self.pos = start + nbytes + GUARD

    def inp(self, name, vals, shift=0):
        self._add(name, 'in', vals.dtype, vals.shape, vals, shift)

    def out(self, name, shape, dtype, shift=0):
        self._add(name, 'out', dtype, shape, None, shift)

    def acc(self, name, vals, shift=0):
        self._add(name, 'acc', vals.dtype, vals.shape, vals, shift)

    def scratch(self, name, nbytes, shift=0, align=16):
        """``align``: the boundary (a multiple of 16 bytes, counted from the start of the buffer) the window starts on before ``shift``"""
        self._add(name, 'scratch', torch.uint8, (int(nbytes),), None, shift, align)

    def build(self):
        total = (self.pos + 15) // 16 * 16
        self.dev = torch.full((total,), self.fill, dtype=torch.uint8, device=self.device)
        assert self.dev.data_ptr() % 16 == 0
        self.inside = torch.zeros(total, dtype=torch.bool, device=self.device)
        for w in self.win.values():
            if w['kind'] != 'in':
                self.inside[w['start']:w['start'] + w['nbytes']] = True
            if w['vals'] is not None:
                self.dev[w['start']:w['start'] + w['nbytes']] = w['vals'].to(self.device)
        self.before = self.dev.clone()
        return self

    def ptr(self, name, offset=0):
        """C pointer to element ``offset`` of a window; None (NULL) for a window that was not added."""
        if name not in self.win:
            return None
        w = self.win[name]
        return ctypes.c_void_p(self.dev.data_ptr() + w['start'] + offset * w['item'])

    def view(self, name):
        """The window as a tensor of its type and shape, on the arena's device (shares the buffer)."""
        w = self.win[name]
        return self.dev[w['start']:w['start'] + w['nbytes']].view(w['dtype']).view(w['shape'])

    def get(self, name):
        return self.view(name).cpu().clone()

    def untouched(self, what):
        """After a refused call: not one byte of the buffer changed, outputs and scratch included."""
        if self.dev.is_cuda:
            torch.cuda.synchronize()
        same = self.dev == self.before
        if not bool(same.all()):
            i = int((~same).nonzero()[0])
            owner = [n for n, w in self.win.items() if w['start'] <= i < w['start'] + w['nbytes']]
            raise AssertionError('%s: a refused call wrote byte %d of the buffer (%s)' % (what, i, owner[0] if owner else 'a guard band'))

    def verify(self, what, finite=True):
        """Every byte outside the out / acc / scratch windows is unchanged (guard bands, inputs); every out element was written; out and acc
        are finite (finite=False: a case whose outputs are non-finite by design keeps the other checks)."""
        if self.dev.is_cuda:
            torch.cuda.synchronize()
        same = (self.dev == self.before) | self.inside
        if not bool(same.all()):
            i = int((~same).nonzero()[0])
            owner = [n for n, w in self.win.items() if w['start'] <= i < w['start'] + w['nbytes']]
            if owner:
                raise AssertionError('%s: input %s was changed (byte %d of the window)' % (what, owner[0], i - self.win[owner[0]]['start']))
            near = min(self.win.items(), key=lambda kv: min(abs(i - kv[1]['start']), abs(i - kv[1]['start'] - kv[1]['nbytes'] + 1)))
            raise AssertionError('%s: byte %d of the buffer, in the guard band next to %s (window %d..%d), was written' % (
                what, i, near[0], near[1]['start'], near[1]['start'] + near[1]['nbytes'] - 1))
        for name, w in self.win.items():
            if w['kind'] == 'out':
                raw = self.dev[w['start']:w['start'] + w['nbytes']].view(-1, w['item'])
                untouched = (raw == self.fill).all(1)
                if bool(untouched.any()):
                    raise AssertionError('%s: output %s was not written everywhere (element %d of %d still holds the fill)' % (
                        what, name, int(untouched.nonzero()[0]), raw.size(0)))
            if finite and w['kind'] in ('out', 'acc') and not bool(torch.isfinite(self.view(name)).all()):
                raise AssertionError('%s: non-finite element in %s' % (what, name))


# ---- pointwise helpers ------------------------------------------------------------------------------------------------------------
def elu(v):
    return torch.where(v > 0, v, torch.expm1(v))


def elu_gate(y):
    """ELU' through the output y = ELU(a): min(y + 1, 1)."""
    return torch.clamp(y + 1, max=1.0)


def act_grad(dy, y, act):
    """dy * act'(a) through the saved output y = act(a), as tt_convout16_1_bwd gates dy; -> (g, r): the value and the number of fp32
    roundings its kernel form takes (relu: a select; sigmoid: (dy (1 - y)) y)."""
    if act == ACT_RELU:
        return torch.where(y > 0, dy, torch.zeros_like(dy)), 0
    if act == ACT_SIGMOID:
        return dy * (1 - y) * y, 3
    return dy, 0


def gate16(g, y):
    """tt_gate16: g * ELU'(y) on 16-bit g, y -> (v, S, K) with one product."""
    v = g * elu_gate(y)
    return v, v.abs(), 1


def skip_join_fwd(y, e, s, reps):
    """tt_skip_join16_fwd: y (reps, n), e (n) -> y[r] + s e as one fma: (v, S, K)."""
    v = y + s * e.unsqueeze(0)
    return v, y.abs() + abs(s) * e.abs().unsqueeze(0), 1


def skip_join_bwd(g, e, s, gate, prev_de=None):
    """tt_skip_join16_bwd: g (reps, n), e (n).  -> (de, bar factor of de in units of u, ds, S of ds, K of ds): t = sum_r g[r] (exact in
    fp32 for 16-bit g), de = s t [* ELU'(e)] [+ what de held], ds = <t, e>."""
    t = g.sum(0)
    de = s * t
    n_round = 1
    if gate & 1:
        de = de * elu_gate(e)
        n_round += 2                                 # e + 1 and the product
    S = de.abs()
    if gate & 2:
        de = de + prev_de
        S = S + prev_de.abs()
        n_round += 1
    return de, n_round * S, (t * e).sum(), (t * e).abs().sum(), t.numel()


def scaled_add(a, b, s):
    """tt_scaled_add16: a + s b as one fma (a may be None): (v, S, K)."""
    v = s * b + (a if a is not None else 0.0)
    return v, (abs(s) * b.abs() + (a.abs() if a is not None else 0.0)), 1


def dot(a, b):
    """tt_dot16: (v, S, K)."""
    return (a * b).sum(), (a * b).abs().sum(), a.numel()


# ---- the 3x3 edge convolutions ----------------------------------------------------------------------------------------------------
def _edge_geom():
    return dict(KH=3, KW=3, stride_h=1, dil_h=1, dil_w=1, pad_h=1, pad_w=1)


def edge_fwd(x, w, b, act):
    """3x3 'same' convolution, x (B, Cin, H, T), w (Cout, Cin, 3, 3): tt_convin16[_1]_fwd (Cin 2 / 1 -> 4, ELU) and tt_convout16[_1]_fwd
    (4 -> 2 / 1; act none / relu / sigmoid).  -> (y, v, S, K): activation applied, pre-activation, sum of absolute products, and
    K (H, T) = Cin x the taps that land in the image."""
    B, Cin, H, T = x.shape
    Cout = w.size(0)
    y, v, S = R.conv2d(x, w.reshape(-1), b, None, Hout=H, act=act, **R.forward_args('conv', Cin, Cout, 3, 3, 1, 1, 1, 1))
    return y, v, S, Cin * R.tap_count(H, H, T, 3, 3, 1, 1, 1, 1, 1, 0)


def edge_bwd(x, g, w):
    """The three gradients of the same layer from x (B, Cin, H, T) and g (B, Cout, H, T) = the gradient at the pre-activation.
    -> dict: 'dw' (v, S, K (3, 3)), 'db' (v, S, K), 'dx' (v, S, K (H, T))."""
    B, Cin, H, T = x.shape
    Cout = g.size(1)
    dw, S, K, db, Sb = R.conv2d_wgrad(x, g, **_edge_geom())
    da = R.dgrad_args('conv', Cin, Cout, 3, 3, 1, 1, 1, 1)
    dx, _, Sx = R.conv2d(g, w.reshape(-1), None, None, Hout=H, **da)
    return dict(dw=(dw, S, K), db=(db, Sb, B * H * T), dx=(dx, Sx, Cout * R.tap_count(H, H, T, 3, 3, 1, 1, 1, 1, 1, 0)))


def edge_carry(x_abs, bar_g, w_abs):
    """A bar on g carried to first order through the three sums of edge_bwd: -> (dw, db, dx) bars."""
    H = x_abs.size(2)
    da = R.dgrad_args('conv', x_abs.size(1), bar_g.size(1), 3, 3, 1, 1, 1, 1)
    return (R.conv2d_wgrad(x_abs, bar_g, **_edge_geom())[0], bar_g.sum((0, 2, 3)),
            R.conv2d(bar_g, w_abs.reshape(-1), None, None, Hout=H, **da)[0])


# ---- the residual block, forward ---------------------------------------------------------------------------------------------------
def ulp16(v, dtype):
    """Spacing of the element type at |v| (that of the subnormals below the smallest normal number)."""
    p, emin = (8, -126) if dtype == torch.bfloat16 else (11, -14)
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** emin)))
    return 2.0 ** (e - (p - 1))


def boundary_spread(v, beta, dtype):
    """What a 16-bit rounding inside a kernel can differ by from round16(v) when the kernel's fp32 value is only known to within beta of
    v: 0 wherever v - beta and v + beta round to the same element (the kernel then holds exactly round16(v)), else the distance of those
    two roundings -- one spacing (ulp16) for an element within its bar of a rounding boundary, more only where beta itself exceeds the
    spacing (small |v| in fp16).  An output that depends on such an element through a weight w has its bar grown by |w| times this."""
    return round16(v + beta, dtype) - round16(v - beta, dtype)


def rb_stage1(x, w1, b1, d):
    """a1 = W1 (*)_d x + b1 of the residual block, x (B, C, H, T), w1 (C, C, 3, 3): (ELU(a1), a1, S, K (H, T))."""
    B, Cn, H, T = x.shape
    fa = R.forward_args('conv', Cn, Cn, 3, 3, 1, d, d, d)
    h, a1, S = R.conv2d(x, w1.reshape(-1), b1, None, Hout=H, act=ACT_ELU, **fa)
    return h, a1, S, Cn * R.tap_count(H, H, T, 3, 3, 1, d, d, d, d, 0)


def rb_stage2(h, w2, b2):
    """a2 = W2 h + b2, w2 (C, C): (ELU(a2), a2, S)."""
    a2 = torch.einsum('oc,bcht->boht', w2, h) + b2.view(1, -1, 1, 1)
    return elu(a2), a2, torch.einsum('oc,bcht->boht', w2.abs(), h.abs())


# ---- the strided pair --------------------------------------------------------------------------------------------------------------
# EncoderBlock.sconv C -> 2C, (4, 1) stride (2, 1); DecoderBlock.tconv 2C -> C with output_padding.  Both weights are (2C, C, 4, 1) arrays.
def stride_layer(kind, C):
    """The layer description conv_ref takes."""
    return ('conv', C, 2 * C, 4, 1, 2, 1, 0, 0) if kind == 'sconv' else ('tconv', 2 * C, C, 4, 1, 2, 1, 0, 0)


def stride_fwd(kind, C, x, w, b, out_pad=0):
    """tt_sconv16_fwd / tt_tconv16_fwd on x (B, Cin, H, T): (y = ELU(v), v, S, K (Hout, T))."""
    layer = stride_layer(kind, C)
    H, T = x.size(2), x.size(3)
    Hout = R.out_rows(layer[0], H, 4, 2, 1, 0, out_pad)
    fa = R.forward_args(*layer)
    y, v, S = R.conv2d(x, w.reshape(-1), b, None, Hout=Hout, act=ACT_ELU, **fa)
    return y, v, S, layer[1] * R.tap_count(H, Hout, T, 4, 1, 2, 1, 1, 0, 0, fa['transposed'])


def stride_bwd(kind, C, x, g, w, gsum=None):
    """The gradients of the same layer from x and g (B, Cout, Hout, T), the gradient at the pre-activation as the matrix products take it
    (rounded to 16 bits); ``gsum``: what the bias gradient sums where that differs (the unrounded gated gradient of the forms that gate
    on the fly).  -> dict: 'dw' (v (2C, C, 4, 1), S, K (1, 1, 4, 1)), 'db' (v, S, K), 'dx' (v, S, K (H, T))."""
    layer = stride_layer(kind, C)
    B, _, H, T = x.shape
    Hout = g.size(2)
    swap, wg, _ = R.wgrad_args(*layer)
    p, q = (g, x) if swap else (x, g)
    dw, S, K, _, _ = R.conv2d_wgrad(p, q, **wg)
    da = R.dgrad_args(*layer)
    dx, _, Sx = R.conv2d(g, w.reshape(-1), None, None, Hout=H, **da)
    gs = g if gsum is None else gsum
    return dict(dw=(dw, S, K.view(1, 1, 4, 1)), db=(gs.sum((0, 2, 3)), gs.abs().sum((0, 2, 3)), B * Hout * T),
                dx=(dx, Sx, layer[2] * R.tap_count(Hout, H, T, 4, 1, 2, 1, 1, 0, 0, da['transposed'])))


# ---- the latent heads -------------------------------------------------------------------------------------------------------------
# w (D, CT, E): index (d CT + c) E + h.  Embeddings (B, CT, E, T) logical (cl16 [B][E][T][CT] in memory), latents (B, D, T) fp32.
def lat_z(z, Dz, D, fill, dtype):
    """The operand the kernels make of z (B, Dz, T): channel D - 1 = the constant ``fill`` where Dz = D - 1, rounded to the element type."""
    if Dz < D:
        z = torch.cat([z, torch.full((z.size(0), 1, z.size(2)), fill, dtype=z.dtype)], 1)
    return round16(z.double(), dtype)


def lat_contract(x, w, Dout):
    """out[b, d, t] = sum_{c, h} w[d, c, h] x[b, c, h, t] for d < Dout: (v, S, K = CT E)."""
    wd = w.double()[:Dout]
    return torch.einsum('dch,bcht->bdt', wd, x), torch.einsum('dch,bcht->bdt', wd.abs(), x.abs()), w.size(1) * w.size(2)


def lat_expand(z, w):
    """out[b, c, h, t] = sum_d w[d, c, h] z[b, d, t]: (v, S, K = D)."""
    wd = w.double()
    return torch.einsum('dch,bdt->bcht', wd, z), torch.einsum('dch,bdt->bcht', wd.abs(), z.abs()), w.size(0)


def lat_wgrad(z, g):
    """dw[d, c, h] = sum_{b, t} z[b, d, t] g[b, c, h, t]; db[c] = sum g: (dw, S, K = B T, db, Sb, Kb = B E T)."""
    B, _, E, T = g.shape
    return (torch.einsum('bdt,bcht->dch', z, g), torch.einsum('bdt,bcht->dch', z.abs(), g.abs()), B * T,
            g.sum((0, 2, 3)), g.abs().sum((0, 2, 3)), B * E * T)
