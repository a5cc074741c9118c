"""The layers on cl16 tensors: residual levels (csrc/conv_wide_bf16.hip, conv_level_bf16.hip), strided layers (conv_stride_bf16.hip), latent heads."""

import ctypes

import torch

from .. import ops as _ops
from ... import _hip
from ..._hip import check, ptr, stream_ptr
from . import skip as _skip
from ._common import _channel_sum, _f32c, _grad_target, instrumented, lib16, loss_scaled_backward
from .cl16 import _as_cl16, new_cl16

# TTRAP_LEVEL_RECOMPUTE=1: the residual blocks of the wide levels (C = 16, 32) run their backward as ONE fused pass that
# recomputes the hidden activation per tile (csrc/conv_level_bf16.hip, tt_wide_rb_bwd_fused): the forward stores no h1 and
# dL/d(conv1 pre-activation) never reaches HBM -- 5 tensor passes per block (x, y | x, dy, dx) instead of 11, and a third less saved
# activation memory at those levels (52.6 -> 42.7 GB peak for the 64-clip step).  Measured (round 3): the fused pass is bound by
# vector-ALU issue, not by HBM (0.52-1.1 ms per block against 0.47-0.52 ms for the three per-stage kernels; step 69.3 -> 76.6 ms),
# so it is the memory-saving option, not the default.


def _level16_forward(ctx, x, dilations, link, join, params):
    """Level16Fn / Level16JoinFn forward.  ``join`` = None or (e, weights, idx, link of e): the level's LAST block adds weights[idx] * e[b mod Be]
    in its epilogue (tt_wide_rb_fwd_join)."""
    B, C, H, T = x.shape
    lib, st = lib16(x), stream_ptr()
    needs_grad = any(ctx.needs_input_grad)
    recompute = C in _ops.RECOMPUTE_CHANNELS
    # the promise to gate: only where backward will take the one-call path below (all of it known now)
    ctx.gate = bool(link is not None and link.producer and ctx.needs_input_grad[0] and _ops.LEVEL_BWD and not recompute and len(dilations) <= 4)
    if ctx.gate:
        link.gated = True
    ctx.link = link
    if link is not None and ctx.needs_input_grad[0]:
        link.accumulates = True             # this level's backward folds parked skip-join backwards into its dx (flush_pending)
    nb = len(dilations)
    outs = [new_cl16(B, C, H, T, x.device, x.dtype) for _ in range(nb)]
    hids = [new_cl16(B, C, H, T, x.device, x.dtype) if (needs_grad and not recompute) else None for _ in range(nb)]
    cur = x
    for i, d in enumerate(dilations):
        w1, b1_, w2, b2 = params[4 * i: 4 * i + 4]
        with _hip.timed('wide_rb_fwd_C%d' % C, clips=B):
            if join is not None and i == nb - 1:
                je, jw, jidx = join[:3]
                check(lib.tt_wide_rb_fwd_join(ptr(cur), ptr(w1), ptr(b1_), ptr(w2), ptr(b2), ptr(outs[i]), ptr(hids[i]), ptr(je), ptr(jw), jidx,
                                              je.size(0), B, C, H, T, d, st), 'tt_wide_rb_fwd_join')
            else:
                check(lib.tt_wide_rb_fwd(ptr(cur), ptr(w1), ptr(b1_), ptr(w2), ptr(b2), ptr(outs[i]), ptr(hids[i]), B, C, H, T, d, st), 'tt_wide_rb_fwd')
        cur = outs[i]
    ctx.dilations = tuple(dilations)
    ctx.params = params
    ctx.recompute = recompute
    ctx.join = None if join is None else (join[2], join[3], join[1], join[4])        # idx, link, the weights parameter object, defer
    if needs_grad:
        saved = []
        for i in range(nb):
            saved += [x if i == 0 else outs[i - 1]] + ([] if recompute else [hids[i]])
        ctx.save_for_backward(*params, *(() if join is None else join[:2]), *saved)
    return outs[-1]


def _level16_backward(ctx, dy):
    """-> (dx, [values returned to autograd for the parameters], de, value returned for the skip weights)."""
    nb = len(ctx.dilations)
    tensors = ctx.saved_tensors
    nj = 0 if ctx.join is None else 2
    params, saved = tensors[:4 * nb], tensors[4 * nb + nj:]
    B, C, H, T = saved[0].shape
    dt = saved[0].dtype
    lib, st = lib16(dt), stream_ptr()
    g_all = _as_cl16(dy, dt)
    de = rs = None
    if ctx.join is not None:
        # the folded join's backward: de = w * (sum over the halves of dy) [* ELU'(e)], dw += <sum, e> -- dy itself goes on into the blocks
        je, jw = tensors[4 * nb: 4 * nb + 2]
        jidx, jlink, jparam, jdefer = ctx.join
        de, rs = _skip._join_backward(g_all, je, jw, jidx, B // je.size(0), jlink, jparam, ctx.needs_input_grad[3], ctx.needs_input_grad[4], jdefer)
    recompute = ctx.recompute
    targets = [_grad_target(t) for t in ctx.params]
    dx = new_cl16(B, C, H, T, g_all.device, dt)
    tmp = [new_cl16(B, C, H, T, g_all.device, dt) for _ in range(2)] if nb > 1 else []
    if _ops.LEVEL_BWD and not recompute and nb <= 4:
        # the whole level in one call: the partial-sum reduces of its blocks are one launch at the end (tt_wide_level_bwd)
        def arr(ts):
            return (ctypes.c_void_p * nb)(*[t.data_ptr() for t in ts])
        ws = torch.empty(lib.tt_wide_level_scratch_bytes(nb, B, C, H, T), dtype=torch.uint8, device=g_all.device)
        cols = list(zip(*[[targets[4 * i + j][0] for j in range(4)] for i in range(nb)]))      # dw1s, db1s, dw2s, db2s
        dil = (ctypes.c_int * nb)(*ctx.dilations)
        fn = lib.tt_wide_level_bwd_gated if ctx.gate else lib.tt_wide_level_bwd
        args = (nb, arr([saved[2 * i] for i in range(nb)]), arr([saved[2 * i + 1] for i in range(nb)]), ptr(g_all),
                arr([params[4 * i] for i in range(nb)]), arr([params[4 * i + 2] for i in range(nb)]),
                arr([params[4 * i + 3] for i in range(nb)]), ptr(dx), ptr(tmp[0]) if tmp else None,
                ptr(tmp[1]) if tmp else None, arr(cols[0]), arr(cols[1]), arr(cols[2]), arr(cols[3]), ptr(ws),
                B, C, H, T, dil)
        ride = _skip._riding_join(ctx, saved[0])
        with _hip.timed('wide_rb_bwd_C%d' % C, clips=B):
            if ride is not None:
                # one parked skip-join backward on this level's input: it rides on the first block's gated epilogue (tt_wide_level_bwd_gated_join)
                pg, pe, pw, pidx, preps, pds = ride
                check(lib.tt_wide_level_bwd_gated_join(*args, ptr(pg), preps, ptr(pw), pidx, ptr(pds), st), 'tt_wide_level_bwd_gated_join')
                ctx.link.pending = []
            else:
                check(fn(*args, st), 'tt_wide_level_bwd')
        _skip.flush_pending(ctx.link, dx)
        return dx, [r for _, r in targets], de, rs
    if ctx.gate:
        raise RuntimeError('ops.LEVEL_BWD / RECOMPUTE_CHANNELS changed between the forward and the backward of a level')
    ws_bytes = lib.tt_wide_fused_scratch_bytes(C) if recompute else lib.tt_wide_scratch_bytes(B, C, H, T)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=g_all.device)
    g = g_all
    for i in reversed(range(nb)):
        w1, b1_, w2, b2 = params[4 * i: 4 * i + 4]
        (dw1, _), (db1, _), (dw2, _), (db2, _) = targets[4 * i: 4 * i + 4]
        gx = dx if i == 0 else tmp[i & 1]
        with _hip.timed('wide_rb_bwd_C%d' % C, clips=B):
            if recompute:
                check(lib.tt_wide_rb_bwd_fused(ptr(saved[i]), ptr(g), ptr(w1), ptr(b1_), ptr(w2), ptr(b2), ptr(gx), ptr(dw1), ptr(db1),
                                               ptr(dw2), ptr(db2), ptr(ws), B, C, H, T, ctx.dilations[i], st), 'tt_wide_rb_bwd_fused')
            else:
                check(lib.tt_wide_rb_bwd(ptr(saved[2 * i]), ptr(saved[2 * i + 1]), ptr(g), ptr(w1), ptr(w2), ptr(b2), ptr(gx), ptr(dw1), ptr(db1),
                                         ptr(dw2), ptr(db2), ptr(ws), B, C, H, T, ctx.dilations[i], st), 'tt_wide_rb_bwd')
        g = gx
    _skip.flush_pending(ctx.link, dx)
    return dx, [r for _, r in targets], de, rs


@instrumented('widelevel', lambda x, *a: 'C%d' % x.size(1))
@loss_scaled_backward(lambda ctx: ctx.saved_tensors[-1].dtype)
class Level16Fn(torch.autograd.Function):
    """The residual blocks of one level on cl16 tensors (csrc/conv_wide_bf16.hip, csrc/conv_level_bf16.hip); see WideLevelFn for
    the fp32-facing form.  Saved for backward: the input of every block, plus its hidden activation at the widths whose
    backward does not recompute it (RECOMPUTE_CHANNELS)."""

    @staticmethod
    def forward(ctx, x, dilations, link, *params):
        return _level16_forward(ctx, x, dilations, link, None, params)

    @staticmethod
    def backward(ctx, dy):
        dx, rp, _, _ = _level16_backward(ctx, dy)
        return (dx, None, None, *rp)


@instrumented('widelevel', lambda x, *a: 'C%d' % x.size(1))
@loss_scaled_backward(lambda ctx: ctx.saved_tensors[-1].dtype)
class Level16JoinFn(torch.autograd.Function):
    """Level16Fn whose LAST block adds the weighted skip in its epilogue: level(x) + weights[idx] * e[b mod Be] (round 6: the join behind a
    DecoderBlock, reference modules.py:569-589, without a pass of its own -- tt_wide_rb_fwd_join; backward = the level's backward on the
    incoming gradient + tt_skip_join16_bwd for e and the weight).  ``elink``: the GateLink of e (see SkipJoin16Fn)."""

    @staticmethod
    def forward(ctx, x, dilations, link, e, weights, idx, elink, defer, *params):
        return _level16_forward(ctx, x, dilations, link, (e, weights, idx, elink, defer), params)

    @staticmethod
    def backward(ctx, dy):
        dx, rp, de, rs = _level16_backward(ctx, dy)
        return (dx, None, None, de, rs, None, None, None, *rp)


@instrumented('sconv16', lambda x, *a: 'C%d' % x.size(1))
@loss_scaled_backward(lambda ctx: ctx.saved_tensors[0].dtype)
class SConv16Fn(torch.autograd.Function):
    """EncoderBlock.sconv on cl16 tensors: (B,C,H,T) -> (B,2C,(H-4)/2+1,T) (csrc/conv_stride_bf16.hip)."""

    @staticmethod
    def forward(ctx, x, w, b, link=None):
        B, C, H, T = x.shape
        y = new_cl16(B, 2 * C, (H - 4) // 2 + 1, T, x.device, x.dtype)
        check(lib16(x).tt_sconv16_fwd(ptr(x), ptr(w), ptr(b), ptr(y), B, C, H, T, stream_ptr()), 'tt_sconv16_fwd')
        ctx.params = (w, b)
        ctx.link = link
        if link is not None:
            link.producer = True
        ctx.save_for_backward(x, w, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        B, C, H, T = x.shape
        lib = lib16(x)
        g = _as_cl16(dy, x.dtype)
        dx = new_cl16(B, C, H, T, x.device, x.dtype) if ctx.needs_input_grad[0] else None
        (dw, r1), (db, r2) = (_grad_target(t) for t in ctx.params)
        ws = torch.empty(lib.tt_stride16_scratch_bytes(C), dtype=torch.uint8, device=x.device)
        if ctx.link is not None and ctx.link.gated:              # the level behind this layer left dy * ELU'(y)
            check(lib.tt_sconv16_bwd_pregated(ptr(x), ptr(g), ptr(w), ptr(dx), ptr(dw), ptr(db), ptr(ws), B, C, H, T, stream_ptr()),
                  'tt_sconv16_bwd_pregated')
            return dx, r1, r2, None
        check(lib.tt_sconv16_bwd(ptr(x), ptr(y), ptr(g), ptr(w), ptr(dx), ptr(dw), ptr(db), ptr(ws), B, C, H, T, stream_ptr()),
              'tt_sconv16_bwd')
        return dx, r1, r2, None


@instrumented('tconv16', lambda x, w, *a: 'C%d' % w.size(1))
@loss_scaled_backward(lambda ctx: ctx.saved_tensors[0].dtype)
class TConv16Fn(torch.autograd.Function):
    """DecoderBlock.tconv on cl16 tensors: (B,2C,H,T) -> (B,C,2H+2+out_pad,T)."""

    @staticmethod
    def forward(ctx, x, w, b, out_pad, link=None, uplink=None):
        B, C2, H, T = x.shape
        C = C2 // 2
        # uplink: x is the ELU output of a 16-bit layer that takes its gradient gated (LatDec16Fn); this layer's pregated backward can do it
        ctx.uplink = uplink if (uplink is not None and uplink.producer and link is not None and C in (16, 32)
                                and ctx.needs_input_grad[0]) else None
        if ctx.uplink is not None:
            uplink.depends = link
            uplink.gated = True
        y = new_cl16(B, C, 2 * H + 2 + out_pad, T, x.device, x.dtype)
        check(lib16(x).tt_tconv16_fwd(ptr(x), ptr(w), ptr(b), ptr(y), B, C, H, T, out_pad, stream_ptr()), 'tt_tconv16_fwd')
        ctx.params = (w, b)
        ctx.out_pad = out_pad
        ctx.link = link
        if link is not None:
            link.producer = True
        ctx.save_for_backward(x, w, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        B, C2, H, T = x.shape
        C = C2 // 2
        lib = lib16(x)
        g = _as_cl16(dy, x.dtype)
        dx = new_cl16(B, C2, H, T, x.device, x.dtype) if ctx.needs_input_grad[0] else None
        (dw, r1), (db, r2) = (_grad_target(t) for t in ctx.params)
        ws = torch.empty(lib.tt_stride16_scratch_bytes(C), dtype=torch.uint8, device=x.device)
        if ctx.link is not None and ctx.link.gated:              # the level behind this layer left dy * ELU'(y)
            check(lib.tt_tconv16_bwd_pregated(ptr(x), ptr(g), ptr(w), ptr(dx), ptr(dw), ptr(db), ptr(ws), B, C, H, T, ctx.out_pad,
                                              1 if ctx.uplink is not None else 0, stream_ptr()), 'tt_tconv16_bwd_pregated')
            return dx, r1, r2, None, None, None
        check(lib.tt_tconv16_bwd(ptr(x), ptr(y), ptr(g), ptr(w), ptr(dx), ptr(dw), ptr(db), ptr(ws), B, C, H, T, ctx.out_pad,
                                 stream_ptr()), 'tt_tconv16_bwd')
        return dx, r1, r2, None, None, None


@instrumented('widelevel', lambda x, *a: 'C%d' % x.size(1))
@loss_scaled_backward(lambda ctx: ctx.dtype)
class WideLevelFn(torch.autograd.Function):
    """
    The residual blocks of one wide level (reference modules.py:621-624 / 690-693: block1..3, dilation 1, 2, 3) with bf16
    channel-innermost activations in HBM (csrc/conv_wide_bf16.hip).  Input and output are ordinary fp32 (B,C,H,T) tensors;
    the block inputs and hidden activations saved for backward are bf16 (half the bytes of the fp32 path).
    Arguments after x: dilations (tuple), then w1, b1, w2, b2 of every block.
    """

    @staticmethod
    def forward(ctx, x, dilations, *params):
        _hip.require_cuda(x, params[0])
        x = _f32c(x)
        B, C, H, T = x.shape
        ctx.dtype = dt = _ops.cl16_dtype()
        lib, st = lib16(dt), stream_ptr()
        nb = len(dilations)
        needs_grad = any(ctx.needs_input_grad)
        cur = torch.empty((B, H, T, C), dtype=dt, device=x.device)
        check(lib.tt_wide_pack(ptr(x), ptr(cur), B, C, H, T, st), 'tt_wide_pack')
        saved = []
        for i, d in enumerate(dilations):
            w1, b1, w2, b2 = params[4 * i: 4 * i + 4]
            nxt = torch.empty_like(cur)
            h1 = torch.empty_like(cur) if needs_grad else None
            with _hip.timed('wide_rb_fwd_C%d' % C):
                check(lib.tt_wide_rb_fwd(ptr(cur), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(nxt), ptr(h1), B, C, H, T, d, st),
                      'tt_wide_rb_fwd')
            saved += [cur, h1]
            cur = nxt
        y = torch.empty_like(x)
        check(lib.tt_wide_unpack(ptr(cur), ptr(y), B, C, H, T, st), 'tt_wide_unpack')
        ctx.dilations = tuple(dilations)
        ctx.params = params
        ctx.geom = (B, C, H, T)
        if needs_grad:
            ctx.save_for_backward(*params, *saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, C, H, T = ctx.geom
        nb = len(ctx.dilations)
        tensors = ctx.saved_tensors
        params, saved = tensors[:4 * nb], tensors[4 * nb:]
        lib, st = lib16(ctx.dtype), stream_ptr()
        dy = _f32c(dy)
        ls = _ops.loss_scale(ctx.dtype)                                # fp32 outside, 16-bit inside: the loss scale goes on here and comes off at the end
        if ls != 1.0:
            dy = dy * ls
        g = torch.empty((B, H, T, C), dtype=ctx.dtype, device=dy.device)
        check(lib.tt_wide_pack(ptr(dy), ptr(g), B, C, H, T, st), 'tt_wide_pack')
        ws = torch.empty(lib.tt_wide_scratch_bytes(B, C, H, T), dtype=torch.uint8, device=dy.device)
        grads = [None] * (4 * nb)
        for i in reversed(range(nb)):
            w1, b1, w2, b2 = params[4 * i: 4 * i + 4]
            xin, h1 = saved[2 * i], saved[2 * i + 1]
            (dw1, r1), (db1, r2), (dw2, r3), (db2, r4) = (_grad_target(t) for t in ctx.params[4 * i: 4 * i + 4])
            gx = torch.empty_like(g)
            with _hip.timed('wide_rb_bwd_C%d' % C):
                check(lib.tt_wide_rb_bwd(ptr(xin), ptr(h1), ptr(g), ptr(w1), ptr(w2), ptr(b2), ptr(gx), ptr(dw1), ptr(db1),
                                         ptr(dw2), ptr(db2), ptr(ws), B, C, H, T, ctx.dilations[i], st), 'tt_wide_rb_bwd')
            grads[4 * i: 4 * i + 4] = [r1, r2, r3, r4]
            g = gx
        dx = torch.empty((B, C, H, T), dtype=torch.float32, device=dy.device)
        check(lib.tt_wide_unpack(ptr(g), ptr(dx), B, C, H, T, st), 'tt_wide_unpack')
        if ls != 1.0:
            dx.mul_(1.0 / ls)
        return (dx, None, *grads)


@instrumented('latenc16', lambda x, *a: 'C%d' % x.size(1))
@loss_scaled_backward(lambda ctx: ctx.saved_tensors[0].dtype)
class LatEnc16Fn(torch.autograd.Function):
    """Encoder.convlat on the cl16 top embedding (csrc/latent_bf16.hip): (B,CT,E,T) cl16 -> latents (B,D,T) fp32."""

    @staticmethod
    def forward(ctx, x, w, b, link=None):
        B, CT, E, T = x.shape
        D = w.size(0)
        lib = lib16(x)
        y = torch.empty((B, D, T), dtype=torch.float32, device=x.device)
        ws = torch.empty(lib.tt_latent16_scratch_bytes(B, CT, D, E, T), dtype=torch.uint8, device=x.device)
        check(lib.tt_latent16_contract(ptr(x), None, ptr(w), ptr(b), ptr(y), ptr(ws), B, CT, D, D, E, T, stream_ptr()),
              'tt_latent16_contract')
        # x is the output of the encoder's last strided layer (+ ELU): its gradient goes back gated (GateLink)
        ctx.gate = bool(link is not None and link.producer and ctx.needs_input_grad[0])
        if ctx.gate:
            link.gated = True
        ctx.link = link
        if link is not None and ctx.needs_input_grad[0]:
            link.accumulates = True         # flush_pending in backward
        ctx.params = (w, b)
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        B, CT, E, T = x.shape
        D = w.size(0)
        lib, st = lib16(x), stream_ptr()
        dy = _f32c(dy)
        ws = torch.empty(lib.tt_latent16_scratch_bytes(B, CT, D, E, T), dtype=torch.uint8, device=x.device)
        dx = rw = rb = None
        if ctx.needs_input_grad[0]:
            dx = new_cl16(B, CT, E, T, x.device, x.dtype)
            if ctx.gate:
                check(lib.tt_latent16_expand_gated(ptr(dy), ptr(w), ptr(x), ptr(dx), ptr(ws), B, CT, D, E, T, st), 'tt_latent16_expand_gated')
            else:
                check(lib.tt_latent16_expand(ptr(dy), D, 0.0, ptr(w), None, ptr(dx), ptr(ws), B, CT, D, E, T, st), 'tt_latent16_expand')
        _skip.flush_pending(ctx.link, dx)
        if ctx.needs_input_grad[1]:
            dw, rw = _grad_target(ctx.params[0])
            check(lib.tt_latent16_wgrad(ptr(dy), D, 0.0, ptr(x), None, ptr(dw), None, ptr(ws), B, CT, D, E, T, st), 'tt_latent16_wgrad')
            db, rb = _grad_target(ctx.params[1])
            _channel_sum(dy, db, B, D, T, st)
        return dx, rw, rb, None


@instrumented('latdec16', lambda z, w, *a: 'C%d' % w.size(1))
@loss_scaled_backward(lambda ctx: ctx.saved_tensors[2].dtype)
class LatDec16Fn(torch.autograd.Function):
    """
    Decoder.convin producing the cl16 top embedding: z (B,Dz,T) fp32 -> ELU(tconv) (B,CT,E,T) cl16.  ``fill`` is None (z carries
    all D = w.size(0) input channels) or the value of a constant LAST channel that z does not carry (Dz = D - 1): the
    transcription switch of TimbreTrap.decode (reference modules.py:139-142) without building the concatenated tensor.
    ``pair`` = (i0, i1) (TimbreTrap.decode_pair; then ``fill`` is None): the output is two batches back to back, both expanded from z,
    the first with the constant channel i0 and the second with i1 (tt_latent16_expand_reps); the backward sums the two halves' latent
    gradient inside the contraction and returns one (B,Dz,T) tensor -- no concatenated copies of the latents, no sliced cat backward and
    no add.  Either way z is transposed to 16 bits once, in the forward; the backward's weight gradient reads that image.
    """

    @staticmethod
    def forward(ctx, z, w, b, fill, link=None, pair=None):
        z = _f32c(z)
        B, Dz, T = z.shape
        D, CT, E = w.size(0), w.size(1), w.size(2)
        if pair is not None and (fill is not None or Dz != D - 1):
            raise ValueError('LatDec16Fn: a pair decode takes the latents without the indicator channel and no fill')
        ctx.reps = 1 if pair is None else 2
        ctx.ind = (0.0 if fill is None else float(fill),) * 2 if pair is None else (float(pair[0]), float(pair[1]))
        R = ctx.reps
        # the pregated backward carries the bias gradient in a free input row of the weight gradient: the library says where it can
        ctx.link = link if (link is not None and lib16(_ops.cl16_dtype()).tt_latent16_pregated_ok(CT, D)) else None
        if ctx.link is not None:
            ctx.link.producer = True
        y = new_cl16(R * B, CT, E, T, z.device, _ops.cl16_dtype())
        lib = lib16(y)
        ws = torch.empty(lib.tt_latent16_scratch_bytes(R * B, CT, D, E, T), dtype=torch.uint8, device=z.device)
        # the 16-bit image of z (no indicator in it: each use names the halves'), kept for the backward's weight gradient
        zt = torch.empty(lib.tt_latent16_image_bytes(B, CT, D, T), dtype=torch.uint8, device=z.device)
        check(lib.tt_latent16_expand_reps(ptr(z), Dz, ctx.ind[0], ctx.ind[1], R, ptr(w), ptr(b), ptr(y), ptr(zt), ptr(ws), B, CT, D, E, T,
                                          stream_ptr()), 'tt_latent16_expand_reps')
        ctx.params = (w, b)
        ctx.zshape = (B, Dz, T)
        ctx.save_for_backward(zt, w, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        zt, w, y = ctx.saved_tensors
        B, Dz, T = ctx.zshape
        D, CT, E = w.size(0), w.size(1), w.size(2)
        R = ctx.reps
        lib, st = lib16(y), stream_ptr()
        g = _as_cl16(dy, y.dtype)
        ws = torch.empty(lib.tt_latent16_scratch_bytes(R * B, CT, D, E, T), dtype=torch.uint8, device=y.device)
        dz = rw = rb = None
        pre = ctx.link is not None and ctx.link.gated           # the transposed layer behind left dy * ELU'(y)
        gy = None if pre else ptr(y)
        if ctx.needs_input_grad[0]:
            dz = torch.empty((B, Dz, T), dtype=torch.float32, device=y.device)
            check(lib.tt_latent16_contract_reps(ptr(g), gy, ptr(w), ptr(dz), ptr(ws), B, CT, D, Dz, E, T, R, st), 'tt_latent16_contract_reps')
        if ctx.needs_input_grad[1]:
            dw, rw = _grad_target(ctx.params[0])
            db, rb = _grad_target(ctx.params[1])
            check(lib.tt_latent16_wgrad_reps(ptr(zt), Dz, ctx.ind[0], ctx.ind[1], R, ptr(g), gy, ptr(dw), ptr(db), ptr(ws), B, CT, D, E, T, st),
                  'tt_latent16_wgrad_reps')
        return dz, rw, rb, None, None, None
