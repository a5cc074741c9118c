"""The fp32 channel-planar bindings: general convolution, fused residual block, strided layers, latent heads (GEMMs), elementwise joins."""

import torch

from .. import ops as _ops
from ... import _hip
from ..._hip import check, ptr, stream_ptr
from ._common import ACT_ELU, ACT_NONE, _channel_sum, _f32c, _grad_target, _off, instrumented

@instrumented('conv', lambda x, w, b, cfg: '%dto%d' % ((x.size(1), w.size(0)) if cfg.kind == 'conv' else (x.size(1), w.size(1))))
class ConvFn(torch.autograd.Function):
    """y = act(conv(x, w) + b) for every non-fused layer of the autoencoder."""

    @staticmethod
    def forward(ctx, x, w, b, cfg):
        _hip.require_cuda(x, w)
        params = (w, b)                                          # as given: _grad_target finds the flat gradient views through them
        x, w, b = _f32c(x), _f32c(w), _f32c(b)                   # what the kernels read: contiguous fp32 (a no-op for the model's own tensors)
        B, Cin, Hin, T = x.shape
        KH, KW = cfg.KH, cfg.KW
        lib = _hip.lib()
        if cfg.kind == 'conv':
            Cout = w.size(0)
            Hout = (Hin + 2 * cfg.pad_h - cfg.dil * (KH - 1) - 1) // cfg.stride + 1
            y = torch.empty((B, Cout, Hout, T), dtype=torch.float32, device=x.device)
            check(lib.tt_conv2d(ptr(x), ptr(w), ptr(b), None, ptr(y), B, Cin, Hin, T, Cout, Hout, KH, KW,
                                cfg.stride, cfg.dil, cfg.dil, cfg.pad_h, cfg.pad_w, 0,
                                Cin * KH * KW, KH * KW, KW, 1, cfg.act, stream_ptr()), 'tt_conv2d')
        else:
            Cout = w.size(1)
            Hout = (Hin - 1) * cfg.stride + KH + cfg.out_pad
            y = torch.empty((B, Cout, Hout, T), dtype=torch.float32, device=x.device)
            check(lib.tt_conv2d(ptr(x), ptr(w), ptr(b), None, ptr(y), B, Cin, Hin, T, Cout, Hout, KH, KW,
                                cfg.stride, 1, 1, 0, 0, 1,
                                KH * KW, Cout * KH * KW, KW, 1, cfg.act, stream_ptr()), 'tt_conv2d(T)')
        ctx.cfg = cfg
        ctx.has_bias = b is not None
        ctx.params = params
        ctx.save_for_backward(x, w, y if cfg.act != ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        cfg = ctx.cfg
        lib = _hip.lib()
        st = stream_ptr()
        dy = _f32c(dy)
        B, Cin, Hin, T = x.shape
        _, Cout, Hout, _ = dy.shape
        KH, KW = cfg.KH, cfg.KW
        if cfg.act == ACT_ELU:
            g = torch.empty_like(dy)
            check(lib.tt_elu_bwd(ptr(dy), ptr(y), ptr(g), dy.numel(), st), 'tt_elu_bwd')
        elif cfg.act != ACT_NONE:                                # relu / sigmoid through the saved output (16-byte aligned operands)
            dy = dy if dy.data_ptr() % 16 == 0 else dy.clone()
            g = torch.empty_like(dy)
            check(lib.tt_act_bwd(ptr(dy), ptr(y), ptr(g), dy.numel(), cfg.act, st), 'tt_act_bwd')
        else:
            g = dy
        dx = dw = db = rw = rb = None
        want_w, want_b = ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            if cfg.kind == 'conv' and cfg.stride == 1:
                # data gradient of a unit-stride conv = the same conv with both kernel axes flipped
                check(lib.tt_conv2d(ptr(g), _off(w, (KH - 1) * KW + (KW - 1)), None, None, ptr(dx),
                                    B, Cout, Hout, T, Cin, Hin, KH, KW, 1, cfg.dil, cfg.dil,
                                    (KH - 1) * cfg.dil - cfg.pad_h, (KW - 1) * cfg.dil - cfg.pad_w, 0,
                                    KH * KW, Cin * KH * KW, -KW, -1, ACT_NONE, st), 'tt_conv2d(dgrad)')
            elif cfg.kind == 'conv':
                # strided conv: gradient is the transposed form (only KW == 1 / dil == 1 layers are strided)
                check(lib.tt_conv2d(ptr(g), _off(w, KW - 1), None, None, ptr(dx),
                                    B, Cout, Hout, T, Cin, Hin, KH, KW, cfg.stride, 1, 1,
                                    cfg.pad_h, (KW - 1) - cfg.pad_w, 1,
                                    KH * KW, Cin * KH * KW, KW, -1, ACT_NONE, st), 'tt_conv2d(dgradT)')
            else:
                # transposed conv: gradient is the plain strided conv with the roles of the channel dims swapped
                check(lib.tt_conv2d(ptr(g), ptr(w), None, None, ptr(dx),
                                    B, Cout, Hout, T, Cin, Hin, KH, KW, cfg.stride, 1, 1, 0, 0, 0,
                                    Cout * KH * KW, KH * KW, KW, 1, ACT_NONE, st), 'tt_conv2d(dgrad of T)')
        # weight and bias gradients are requested independently (a frozen weight with a trainable bias still gets db)
        if want_w:
            dw, rw = _grad_target(ctx.params[0])
        if want_b:
            db, rb = _grad_target(ctx.params[1])
        if want_w:
            if cfg.kind == 'conv':
                check(lib.tt_conv2d_wgrad(ptr(x), ptr(g), ptr(dw), ptr(db), B, Cin, Hin, T, Cout, Hout, KH, KW,
                                          cfg.stride, cfg.dil, cfg.dil, cfg.pad_h, cfg.pad_w,
                                          Cin * KH * KW, KH * KW, KW, 1, st), 'tt_conv2d_wgrad')
                db = None                                   # produced by the same launch
            else:
                # dW[ci][co][kh] = sum x[ci][hi] * g[co][stride*hi + kh]: same kernel, roles swapped
                check(lib.tt_conv2d_wgrad(ptr(g), ptr(x), ptr(dw), None, B, Cout, Hout, T, Cin, Hin, KH, KW,
                                          cfg.stride, 1, 1, 0, 0,
                                          Cout * KH * KW, KH * KW, KW, 1, st), 'tt_conv2d_wgrad(T)')
        if db is not None:
            _channel_sum(g, db, B, Cout, Hout * T, st)
        return dx, rw, rb, None


class AddFn(torch.autograd.Function):
    """y = a + b (residual / skip joins)."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = _f32c(a), _f32c(b)
        y = torch.empty_like(a)
        check(_hip.lib().tt_scaled_add(ptr(a), ptr(b), None, 0, ptr(y), a.numel(), stream_ptr()), 'tt_scaled_add')
        return y

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


class ScaleFn(torch.autograd.Function):
    """y = s[idx] * e  (TimbreTrap.apply_skip_connections, reference modules.py:112)."""

    @staticmethod
    def forward(ctx, e, s, idx):
        e, s = _f32c(e), _f32c(s)
        y = torch.empty_like(e)
        check(_hip.lib().tt_scaled_add(None, ptr(e), ptr(s), idx, ptr(y), e.numel(), stream_ptr()), 'tt_scaled_add')
        ctx.idx = idx
        ctx.save_for_backward(e, s)
        return y

    @staticmethod
    def backward(ctx, dy):
        e, s = ctx.saved_tensors
        dy = _f32c(dy)
        lib, st = _hip.lib(), stream_ptr()
        de = ds = None
        if ctx.needs_input_grad[0]:
            de = torch.empty_like(e)
            check(lib.tt_scaled_add(None, ptr(dy), ptr(s), ctx.idx, ptr(de), e.numel(), st), 'tt_scaled_add')
        if ctx.needs_input_grad[1]:
            ds = torch.zeros_like(s)
            check(lib.tt_dot(ptr(dy), ptr(e), _off(ds, ctx.idx), e.numel(), st), 'tt_dot')
        return de, ds, None


@instrumented('rb', lambda x, *a: 'C%d' % x.size(1))
class ResBlockFn(torch.autograd.Function):
    """Fused ResidualConv2dBlock (reference modules.py:755-777); hidden activations recomputed in backward."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, dilation):
        _hip.require_cuda(x, w1)
        params = (w1, b1, w2, b2)
        x, w1, b1, w2, b2 = (_f32c(t) for t in (x, w1, b1, w2, b2))
        B, C, H, T = x.shape
        y = torch.empty_like(x)
        needs_grad = any(ctx.needs_input_grad[:5])
        h1 = torch.empty_like(x) if (needs_grad and _ops.SAVE_HIDDEN) else None
        with _hip.timed('resblock_fwd_C%d' % C):          # the kernel launch alone (bench.py: roofline of the dominant kernel)
            check(_hip.lib().tt_resblock_fwd(ptr(x), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(y), ptr(h1), B, C, H, T, dilation,
                                             _ops._flags(), stream_ptr()), 'tt_resblock_fwd')
        ctx.dilation = dilation
        ctx.flags = _ops._flags()
        ctx.params = params
        ctx.save_for_backward(x, w1, b1, w2, b2, h1)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w1, b1, w2, b2, h1 = ctx.saved_tensors
        dy = _f32c(dy)
        B, C, H, T = x.shape
        dx = torch.empty_like(x)
        (dw1, r1), (db1, r2), (dw2, r3), (db2, r4) = (_grad_target(t) for t in ctx.params)
        ws = torch.empty(x.numel() + _hip.lib().tt_wgrad_scratch_floats(), dtype=torch.float32, device=x.device)
        with _hip.timed('resblock_bwd_C%d' % C):
            check(_hip.lib().tt_resblock_bwd(ptr(x), ptr(h1), ptr(dy), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(dx), ptr(dw1),
                                             ptr(db1), ptr(dw2), ptr(db2), ptr(ws), B, C, H, T, ctx.dilation,
                                             ctx.flags, stream_ptr()), 'tt_resblock_bwd')
        return dx, r1, r2, r3, r4, None


def _stride_forward(ctx, entry, x, w, b, C, Cout, Hout, *extra):
    """StridedConvFn / TransposedConvFn forward on the MFMA strided kernels: C = channels of the narrow side; ``extra``: the out_pad of tt_tconv_*."""
    _hip.require_cuda(x, w)
    params = (w, b)
    x, w, b = _f32c(x), _f32c(w), _f32c(b)
    B, _, H, T = x.shape
    y = torch.empty((B, Cout, Hout, T), dtype=torch.float32, device=x.device)
    check(getattr(_hip.lib(), entry + '_fwd')(ptr(x), ptr(w), ptr(b), ptr(y), B, C, H, T, *extra, stream_ptr()), entry + '_fwd')
    ctx.params, ctx.geom = params, (C, extra)
    ctx.save_for_backward(x, w, y)
    return y


def _stride_backward(ctx, entry, dy):
    x, w, y = ctx.saved_tensors
    dy = _f32c(dy)
    B, _, H, T = x.shape
    C, extra = ctx.geom
    dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
    (dw, rw), (db, rb) = (_grad_target(t) for t in ctx.params)
    scratch = torch.empty(_hip.lib().tt_wgrad_scratch_floats() + dy.numel(), dtype=torch.float32, device=x.device)
    check(getattr(_hip.lib(), entry + '_bwd')(ptr(x), ptr(y), ptr(dy), ptr(w), ptr(dx), ptr(dw), ptr(db), ptr(scratch), B, C, H, T, *extra,
                                              stream_ptr()), entry + '_bwd')
    return dx, rw, rb


@instrumented('sconv', lambda x, *a: 'C%d' % x.size(1))
class StridedConvFn(torch.autograd.Function):
    """EncoderBlock.sconv: ELU(Conv2d(C, 2C, (4,1), stride (2,1))) on the MFMA strided kernel."""

    @staticmethod
    def forward(ctx, x, w, b):
        C, H = x.size(1), x.size(2)
        return _stride_forward(ctx, 'tt_sconv', x, w, b, C, 2 * C, (H - 4) // 2 + 1)

    @staticmethod
    def backward(ctx, dy):
        return _stride_backward(ctx, 'tt_sconv', dy)


@instrumented('tconv', lambda x, w, *a: 'C%d' % w.size(1))
class TransposedConvFn(torch.autograd.Function):
    """DecoderBlock.tconv: ELU(ConvTranspose2d(2C, C, (4,1), stride (2,1), output_padding)) on the MFMA kernel."""

    @staticmethod
    def forward(ctx, x, w, b, out_pad):
        C, H = x.size(1) // 2, x.size(2)
        return _stride_forward(ctx, 'tt_tconv', x, w, b, C, C, 2 * H + 2 + out_pad, out_pad)

    @staticmethod
    def backward(ctx, dy):
        return (*_stride_backward(ctx, 'tt_tconv', dy), None)


@instrumented('latenc', lambda x, *a: 'C%d' % x.size(1))
class LatentEncodeFn(torch.autograd.Function):
    """Encoder.convlat: Conv2d(C, D, (E,1)) collapsing the frequency axis = per-clip GEMM (D x C*E)(C*E x T)."""

    @staticmethod
    def forward(ctx, x, w, b):
        x, w = _f32c(x), _f32c(w)
        B, C, E, T = x.shape
        D, K = w.size(0), C * E
        y = torch.empty((B, D, T), dtype=torch.float32, device=x.device)
        check(_hip.lib().tt_gemm(ptr(w), ptr(x), ptr(y), ptr(b), D, T, K, 0, 0, K, T, T, B, 0, K * T, D * T, 0,
                                 1.0, 0.0, 1 if b is not None else 0, 1, ACT_NONE, stream_ptr()), 'tt_gemm(convlat)')
        ctx.has_bias = b is not None
        ctx.params = (w, b)
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _f32c(dy)
        B, C, E, T = x.shape
        D, K = w.size(0), C * E
        lib, st = _hip.lib(), stream_ptr()
        dx = dw = db = rw = rb = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            check(lib.tt_gemm(ptr(w), ptr(dy), ptr(dx), None, K, T, D, 1, 0, K, T, T, B, 0, D * T, K * T, 0,
                              1.0, 0.0, 0, 1, ACT_NONE, st), 'tt_gemm(convlat dgrad)')
        if ctx.needs_input_grad[1]:
            dw, rw = _grad_target(ctx.params[0])
            check(lib.tt_gemm(ptr(dy), ptr(x), ptr(dw), None, D, K, T, 0, 1, T, T, K, B, D * T, K * T, 0, 1,
                              1.0, 1.0, 0, 1, ACT_NONE, st), 'tt_gemm(convlat wgrad)')
            if ctx.has_bias:
                db, rb = _grad_target(ctx.params[1])
                _channel_sum(dy, db, B, D, T, st)
        return dx, rw, rb


@instrumented('latdec', lambda z, w, *a: 'C%d' % w.size(1))
class LatentDecodeFn(torch.autograd.Function):
    """Decoder.convin: ConvTranspose2d(D+1, C, (E,1)) + ELU = per-clip GEMM (C*E x D+1)(D+1 x T)."""

    @staticmethod
    def forward(ctx, z, w, b):
        z, w = _f32c(z), _f32c(w)
        B, K, T = z.shape
        C, E = w.size(1), w.size(2)
        Mo = C * E
        y = torch.empty((B, C, E, T), dtype=torch.float32, device=z.device)
        check(_hip.lib().tt_gemm(ptr(w), ptr(z), ptr(y), ptr(b), Mo, T, K, 1, 0, Mo, T, T, B, 0, K * T, Mo * T, 0,
                                 1.0, 0.0, 2 if b is not None else 0, E, ACT_ELU, stream_ptr()), 'tt_gemm(dec convin)')
        ctx.has_bias = b is not None
        ctx.params = (w, b)
        ctx.save_for_backward(z, w, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        z, w, y = ctx.saved_tensors
        dy = _f32c(dy)
        B, K, T = z.shape
        C, E = w.size(1), w.size(2)
        Mo = C * E
        lib, st = _hip.lib(), stream_ptr()
        g = torch.empty_like(dy)
        check(lib.tt_elu_bwd(ptr(dy), ptr(y), ptr(g), dy.numel(), st), 'tt_elu_bwd')
        dz = dw = db = rw = rb = None
        if ctx.needs_input_grad[0]:
            dz = torch.empty_like(z)
            check(lib.tt_gemm(ptr(w), ptr(g), ptr(dz), None, K, T, Mo, 0, 0, Mo, T, T, B, 0, Mo * T, K * T, 0,
                              1.0, 0.0, 0, 1, ACT_NONE, st), 'tt_gemm(dec convin dgrad)')
        if ctx.needs_input_grad[1]:
            dw, rw = _grad_target(ctx.params[0])
            check(lib.tt_gemm(ptr(z), ptr(g), ptr(dw), None, K, Mo, T, 0, 1, T, T, Mo, B, K * T, Mo * T, 0, 1,
                              1.0, 1.0, 0, 1, ACT_NONE, st), 'tt_gemm(dec convin wgrad)')
            if ctx.has_bias:
                db, rb = _grad_target(ctx.params[1])
                _channel_sum(g, db, B, C, E * T, st)
        return dz, rw, rb
