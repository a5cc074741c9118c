"""
The yardstick of tests/test_gpu_conv_parity.py, checked where no GPU is needed: tests/conv_ref.py (gather + einsum over the arguments of
tt_conv2d / tt_conv2d_wgrad) against float64 F.conv2d, F.conv_transpose2d and autograd, for every argument set that
timbre_trap/framework/ops/fp32.py builds: forward, transposed forward, the three data-gradient forms (flipped kernel through negative
strides and an offset base; the transposed form of a strided conv; the role-swapped strided conv of a transposed one) and both
weight-gradient forms.  Agreement: 1e-12 of the sum of absolute products S that conv_ref returns next to each value.
"""

import pytest
import torch
import torch.nn.functional as F

import conv_ref as R

TOL = 1e-12

# kind, Cin, Cout, KH, KW, stride, dil, pad_h, pad_w, out_pad, H, T  -- the layer shapes of the autoencoder plus ragged relatives
LAYERS = [
    ('conv', 2, 4, 3, 3, 1, 1, 1, 1, 0, 7, 9),         # Encoder.convin
    ('conv', 4, 2, 3, 3, 1, 1, 1, 1, 0, 1, 1),         # a plane smaller than the halo
    ('conv', 3, 6, 3, 3, 1, 3, 3, 3, 0, 2, 3),         # dilation 3 on a plane inside the halo: only the centre tap lands
    ('conv', 8, 8, 3, 3, 1, 2, 2, 2, 0, 6, 11),
    ('conv', 5, 7, 1, 1, 1, 1, 0, 0, 0, 4, 6),
    ('conv', 4, 8, 4, 1, 2, 1, 0, 0, 0, 9, 5),         # EncoderBlock.sconv, odd height: the last row is unused
    ('conv', 4, 8, 4, 1, 2, 1, 0, 0, 0, 10, 5),
    ('conv', 3, 5, 3, 3, 2, 1, 1, 1, 0, 8, 6),         # strided with a kernel along time: the kw flip of the transposed data gradient
    ('tconv', 8, 4, 4, 1, 2, 1, 0, 0, 0, 5, 6),        # DecoderBlock.tconv
    ('tconv', 8, 4, 4, 1, 2, 1, 0, 0, 1, 5, 6),        # ... with the extra output row
    ('tconv', 6, 3, 4, 1, 2, 1, 0, 0, 1, 1, 2),
]


def _close(got, want, scale, what):
    e = (got - want).abs()
    assert bool((e <= TOL * scale).all()), '%s: off by %.3e where the scale is %.3e' % (what, float(e.max()), float(scale.max()))


def _torch_forward(kind, x, w, b, stride, dil, pad_h, pad_w, out_pad):
    if kind == 'conv':
        return F.conv2d(x, w, b, stride=(stride, 1), padding=(pad_h, pad_w), dilation=(dil, dil))
    return F.conv_transpose2d(x, w, b, stride=(stride, 1), output_padding=(out_pad, 0))


@pytest.mark.parametrize('layer', LAYERS, ids=['%s-%dto%d-k%dx%d-s%d-d%d-p%d-H%d-T%d' % (l[0], l[1], l[2], l[3], l[4], l[5], l[6], l[9], l[10], l[11])
                                               for l in LAYERS])
def test_restatement_against_torch(layer):
    kind, Cin, Cout, KH, KW, stride, dil, pad_h, pad_w, out_pad, H, T = layer
    gen = torch.Generator().manual_seed(H * 100 + T)
    B = 2
    x = torch.randn(B, Cin, H, T, generator=gen, dtype=torch.float64, requires_grad=True)
    wshape = (Cout, Cin, KH, KW) if kind == 'conv' else (Cin, Cout, KH, KW)
    w = torch.randn(*wshape, generator=gen, dtype=torch.float64, requires_grad=True)
    b = torch.randn(Cout, generator=gen, dtype=torch.float64, requires_grad=True)
    Hout = R.out_rows(kind, H, KH, stride, dil, pad_h, out_pad)
    geom = (kind, Cin, Cout, KH, KW, stride, dil, pad_h, pad_w)

    v_t = _torch_forward(kind, x, w, b, stride, dil, pad_h, pad_w, out_pad)
    assert v_t.shape == (B, Cout, Hout, T)
    res = torch.randn(B, Cout, Hout, T, generator=gen, dtype=torch.float64)
    wflat = w.detach().reshape(-1)

    # forward, every activation, with and without bias / residual
    for act, fn in ((R.ACT_NONE, lambda v: v), (R.ACT_ELU, F.elu), (R.ACT_RELU, torch.relu), (R.ACT_SIGMOID, torch.sigmoid)):
        y, v, S = R.conv2d(x.detach(), wflat, b.detach(), res, Hout=Hout, act=act, **R.forward_args(*geom))
        _close(v, v_t.detach(), S + b.detach().abs().view(1, -1, 1, 1), 'pre-activation')
        _close(y, fn(v_t.detach()) + res, S + b.detach().abs().view(1, -1, 1, 1) + res.abs() + 1.0, 'act %d' % act)
    y, v, S = R.conv2d(x.detach(), wflat, None, None, Hout=Hout, **R.forward_args(*geom))
    _close(y, v_t.detach() - b.detach().view(1, -1, 1, 1), S + b.detach().abs().view(1, -1, 1, 1), 'no bias')
    assert torch.equal(y, v)

    # the gradients of <g, conv(x)> by autograd
    g = torch.randn(B, Cout, Hout, T, generator=gen, dtype=torch.float64)
    dx_t, dw_t, db_t = torch.autograd.grad(v_t, (x, w, b), g)

    # data gradient: tt_conv2d on g with the layer's channel counts swapped and the weight read through other strides
    a = R.dgrad_args(*geom)
    wbuf = torch.cat([wflat, torch.full((4,), float('nan'), dtype=torch.float64)])      # reading past the weight shows as NaN
    dx, _, S = R.conv2d(g, wbuf, None, None, Hout=H, **a)
    assert dx.shape == x.shape
    _close(dx, dx_t, S, 'data gradient')
    if kind == 'conv' and stride == 1 and KH * KW > 1:
        assert a['ws_kh'] < 0 and a['ws_kw'] < 0 and a['base'] == KH * KW - 1         # the flipped-kernel form is what ran
    if kind == 'conv' and KH == 4 and H % 2 == 1:
        assert bool((dx[:, :, -1] == 0).all()) and bool((S[:, :, -1] == 0).all())     # the unused last row: no term at all

    # weight and bias gradient
    swap, wg, strides = R.wgrad_args(*geom)
    if swap:
        dw, S, K, _, _ = R.conv2d_wgrad(g, x.detach(), **wg)
    else:
        dw, S, K, db, Sb = R.conv2d_wgrad(x.detach(), g, **wg)
        _close(db, db_t, Sb, 'bias gradient')
    assert dw.shape == w.shape
    _close(dw, dw_t, S, 'weight gradient')
    # the strides address the layer's own weight layout, every element once
    idx = R.weight_index(w.size(0), w.size(1), KH, KW, **strides)
    assert torch.equal(idx.reshape(-1), torch.arange(w.numel()))
    assert int(K.max()) <= B * max(H, Hout) * T and int(K.min()) >= 0
    # a tap that never lands in the image sums nothing
    assert bool((dw[:, :, K == 0] == 0).all())


def test_weight_index_of_the_flipped_form():
    """Negative strides from a base at the last tap read the kernel back to front, in bounds."""
    Cin, Cout, KH, KW = 3, 5, 3, 3
    a = R.dgrad_args('conv', Cin, Cout, KH, KW, 1, 2, 2, 2)
    idx = R.weight_index(a['Cout'], Cout, KH, KW, a['ws_co'], a['ws_ci'], a['ws_kh'], a['ws_kw'], a['base'])
    assert int(idx.min()) == 0 and int(idx.max()) == Cout * Cin * KH * KW - 1
    w = torch.arange(Cout * Cin * KH * KW).view(Cout, Cin, KH, KW)
    assert torch.equal(w.reshape(-1)[idx], w.flip(2, 3).transpose(0, 1))


def test_transposed_rows_without_a_term():
    """transposed: output row ho takes tap kh only where ho + pad - kh is a non-negative multiple of the stride inside the input."""
    hi, ok = R.tap_rows(Hin=2, Hout=7, KH=4, stride_h=2, dil_h=1, pad_h=0, transposed=1)
    want = [[(0, 0)], [(1, 0)], [(0, 1), (2, 0)], [(1, 1), (3, 0)], [(2, 1)], [(3, 1)], []]        # (kh, hi) per output row
    for ho in range(7):
        got = [(kh, int(hi[ho, kh])) for kh in range(4) if bool(ok[ho, kh])]
        assert got == want[ho], ho
