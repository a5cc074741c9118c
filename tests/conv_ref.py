"""
Float64 restatement of the general convolution of include/ttrap.h (tt_conv2d / tt_conv2d_wgrad), written with gather and einsum over
the SAME arguments the C entry points take: signed weight strides, the weight base as an element offset into a flat buffer,
``transposed``, ``stride_h``, dilations, pads, ``res`` and ``act``.  No F.conv2d: tests/test_conv_restatement.py pins this file against
torch, tests/test_gpu_conv_parity.py holds the kernels to it.

    y[b,co,ho,t] = act(bias[co] + sum_{ci,kh,kw} w[base + co ws_co + ci ws_ci + kh ws_kh + kw ws_kw] x[b,ci,hi,ti]) + res[b,co,ho,t]
    ti = t + kw dil_w - pad_w
    transposed == 0:  hi = ho stride_h + kh dil_h - pad_h
    transposed == 1:  hi = (ho + pad_h - kh dil_h) / stride_h   when divisible (else no term)
    dw[...] += sum_{b,ho,t} g[b,co,ho,t] x[b,ci,hi,ti]          (transposed == 0 form),   dbias[co] += sum g[b,co,:,:]

Next to every value comes S = sum |w| |x| (the sum of absolute products): a length-K sum of products computed in fp32 in ANY order is
within K 2^-24 S of the exact one, which is the bar the GPU tests use.

The ``*_args`` functions build the argument sets of timbre_trap/framework/ops/fp32.py (ConvFn.forward / .backward) for a layer geometry.
"""

import torch

ACT_NONE, ACT_ELU, ACT_RELU, ACT_SIGMOID = 0, 1, 2, 3


def act64(v, act):
    if act == ACT_ELU:
        return torch.where(v > 0, v, torch.expm1(v))
    if act == ACT_RELU:
        return torch.relu(v)
    if act == ACT_SIGMOID:
        return torch.sigmoid(v)
    return v


def weight_index(Cout, Cin, KH, KW, ws_co, ws_ci, ws_kh, ws_kw, base=0):
    """Element index of w[co][ci][kh][kw] in the flat weight buffer, (Cout, Cin, KH, KW) int64."""
    co = torch.arange(Cout).view(-1, 1, 1, 1)
    ci = torch.arange(Cin).view(1, -1, 1, 1)
    kh = torch.arange(KH).view(1, 1, -1, 1)
    kw = torch.arange(KW).view(1, 1, 1, -1)
    return base + co * ws_co + ci * ws_ci + kh * ws_kh + kw * ws_kw


def tap_rows(Hin, Hout, KH, stride_h, dil_h, pad_h, transposed):
    """(hi, valid), both (Hout, KH): the input row of tap kh of output row ho, and whether the term exists."""
    ho = torch.arange(Hout).view(-1, 1)
    kh = torch.arange(KH).view(1, -1)
    if transposed:
        num = ho + pad_h - kh * dil_h
        hi = torch.div(num, stride_h, rounding_mode='floor')
        ok = (num >= 0) & (hi * stride_h == num) & (hi < Hin)
    else:
        hi = ho * stride_h + kh * dil_h - pad_h
        ok = (hi >= 0) & (hi < Hin)
    return hi.clamp(0, Hin - 1), ok


def tap_cols(T, KW, dil_w, pad_w):
    t = torch.arange(T).view(-1, 1)
    kw = torch.arange(KW).view(1, -1)
    ti = t + kw * dil_w - pad_w
    return ti.clamp(0, T - 1), (ti >= 0) & (ti < T)


def gather_taps(x, Hout, KH, KW, stride_h, dil_h, dil_w, pad_h, pad_w, transposed):
    """x (B, Cin, Hin, T) float64 -> (B, Cin, Hout, KH, T, KW): x[b, ci, hi, ti] of every (output pixel, tap), 0 where no term exists."""
    B, Cin, Hin, T = x.shape
    hi, hok = tap_rows(Hin, Hout, KH, stride_h, dil_h, pad_h, transposed)
    ti, tok = tap_cols(T, KW, dil_w, pad_w)
    g = x[:, :, hi][:, :, :, :, ti]                                  # (B, Cin, Hout, KH, T, KW)
    ok = hok.view(1, 1, Hout, KH, 1, 1) & tok.view(1, 1, 1, 1, T, KW)
    return torch.where(ok, g, torch.zeros((), dtype=x.dtype)), hok, tok


def tap_count(Hin, Hout, T, KH, KW, stride_h, dil_h, dil_w, pad_h, pad_w, transposed):
    """(Hout, T): how many taps (kh, kw) of an output pixel land in the image -- times Cin, the number of products its sum has."""
    _, hok = tap_rows(Hin, Hout, KH, stride_h, dil_h, pad_h, transposed)
    _, tok = tap_cols(T, KW, dil_w, pad_w)
    return hok.sum(1).view(Hout, 1) * tok.sum(1).view(1, T)


def conv2d(x, wbuf, bias, res, Cout, Hout, KH, KW, stride_h, dil_h, dil_w, pad_h, pad_w, transposed, ws_co, ws_ci, ws_kh, ws_kw, act=ACT_NONE,
           base=0):
    """tt_conv2d in float64.  x (B, Cin, Hin, T), wbuf the flat weight buffer, ``base`` the element offset of the pointer handed to the
    library.  Returns (y, v, S): the result, the pre-activation bias + sum, and the sum of absolute products (same shape)."""
    x = x.double()
    Cin = x.size(1)
    w = wbuf.double()[weight_index(Cout, Cin, KH, KW, ws_co, ws_ci, ws_kh, ws_kw, base)]
    taps, _, _ = gather_taps(x, Hout, KH, KW, stride_h, dil_h, dil_w, pad_h, pad_w, transposed)
    v = torch.einsum('oikl,bihktl->boht', w, taps)
    S = torch.einsum('oikl,bihktl->boht', w.abs(), taps.abs())
    if bias is not None:
        v = v + bias.double().view(1, -1, 1, 1)
    y = act64(v, act)
    if res is not None:
        y = y + res.double()
    return y, v, S


def conv2d_wgrad(x, g, KH, KW, stride_h, dil_h, dil_w, pad_h, pad_w):
    """The sums of tt_conv2d_wgrad in float64 as dense arrays (place them with ``weight_index``).  x (B, Cin, Hin, T), g (B, Cout, Hout, T).
    Returns (dw, S, K, db, Sb): dw / S (Cout, Cin, KH, KW) the sum and the sum of absolute products, K (KH, KW) the number of summed
    products of a tap (B Hout T restricted to the taps that land in the image), db / Sb (Cout) the bias sum and sum |g|."""
    x, g = x.double(), g.double()
    B, _, Hout, T = g.shape
    taps, hok, tok = gather_taps(x, Hout, KH, KW, stride_h, dil_h, dil_w, pad_h, pad_w, 0)
    dw = torch.einsum('boht,bihktl->oikl', g, taps)
    S = torch.einsum('boht,bihktl->oikl', g.abs(), taps.abs())
    K = B * hok.sum(0).view(KH, 1) * tok.sum(0).view(1, KW)
    return dw, S, K, g.sum((0, 2, 3)), g.abs().sum((0, 2, 3))


# ---- the argument sets of ops/fp32.py ---------------------------------------------------------------------------------------------------
# A layer: kind 'conv' (weight (Cout, Cin, KH, KW)) or 'tconv' (weight (Cin, Cout, KH, KW)), stride / dilation / pads as ConvCfg.

def out_rows(kind, Hin, KH, stride, dil, pad_h, out_pad):
    if kind == 'conv':
        return (Hin + 2 * pad_h - dil * (KH - 1) - 1) // stride + 1
    return (Hin - 1) * stride + KH + out_pad


def forward_args(kind, Cin, Cout, KH, KW, stride, dil, pad_h, pad_w):
    """ConvFn.forward: keyword arguments of ``conv2d`` (without x, wbuf, bias, res, Hout, act)."""
    if kind == 'conv':
        return dict(Cout=Cout, KH=KH, KW=KW, stride_h=stride, dil_h=dil, dil_w=dil, pad_h=pad_h, pad_w=pad_w, transposed=0,
                    ws_co=Cin * KH * KW, ws_ci=KH * KW, ws_kh=KW, ws_kw=1, base=0)
    return dict(Cout=Cout, KH=KH, KW=KW, stride_h=stride, dil_h=1, dil_w=1, pad_h=0, pad_w=0, transposed=1,
                ws_co=KH * KW, ws_ci=Cout * KH * KW, ws_kh=KW, ws_kw=1, base=0)


def dgrad_args(kind, Cin, Cout, KH, KW, stride, dil, pad_h, pad_w):
    """ConvFn.backward, data gradient: dx = conv2d(g, w, ...) with Cout := Cin of the layer and Hout := Hin of the layer.  The three forms:
    unit-stride conv (both kernel axes flipped: negative strides, base at the last tap), strided conv (the transposed form), transposed
    conv (the plain strided conv with the channel roles swapped)."""
    if kind == 'conv' and stride == 1:
        return dict(Cout=Cin, KH=KH, KW=KW, stride_h=1, dil_h=dil, dil_w=dil, pad_h=(KH - 1) * dil - pad_h, pad_w=(KW - 1) * dil - pad_w,
                    transposed=0, ws_co=KH * KW, ws_ci=Cin * KH * KW, ws_kh=-KW, ws_kw=-1, base=(KH - 1) * KW + (KW - 1))
    if kind == 'conv':
        return dict(Cout=Cin, KH=KH, KW=KW, stride_h=stride, dil_h=1, dil_w=1, pad_h=pad_h, pad_w=(KW - 1) - pad_w, transposed=1,
                    ws_co=KH * KW, ws_ci=Cin * KH * KW, ws_kh=KW, ws_kw=-1, base=KW - 1)
    return dict(Cout=Cin, KH=KH, KW=KW, stride_h=stride, dil_h=1, dil_w=1, pad_h=0, pad_w=0, transposed=0,
                ws_co=Cout * KH * KW, ws_ci=KH * KW, ws_kh=KW, ws_kw=1, base=0)


def wgrad_args(kind, Cin, Cout, KH, KW, stride, dil, pad_h, pad_w):
    """ConvFn.backward, weight gradient: (swap, geometry, strides).  swap = False: tt_conv2d_wgrad(x, g, ...); True (transposed layer):
    tt_conv2d_wgrad(g, x, ...) -- the same sum with the roles swapped, so the dense result has the layout of the layer's own weight,
    (layer Cin, layer Cout, KH, KW)."""
    if kind == 'conv':
        return False, dict(KH=KH, KW=KW, stride_h=stride, dil_h=dil, dil_w=dil, pad_h=pad_h, pad_w=pad_w), \
            dict(ws_co=Cin * KH * KW, ws_ci=KH * KW, ws_kh=KW, ws_kw=1)
    return True, dict(KH=KH, KW=KW, stride_h=stride, dil_h=1, dil_w=1, pad_h=0, pad_w=0), \
        dict(ws_co=Cout * KH * KW, ws_ci=KH * KW, ws_kh=KW, ws_kw=1)
