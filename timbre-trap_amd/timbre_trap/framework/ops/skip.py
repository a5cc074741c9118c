"""Skip joins on cl16 tensors: two steps on scaled tensors (Add16Fn, Scale16Fn), one pass (SkipJoin16Fn), deferred backward (flush_pending)."""

import torch

from .. import ops as _ops
from ..._hip import check, ptr, stream_ptr
from ._common import _device_scalar, _f32c, _grad_target, _off, instrumented, lib16, loss_scaled_backward
from .cl16 import _as_cl16, new_cl16

class Add16Fn(torch.autograd.Function):
    """a + b on cl16 tensors (the skip joins of the 16-bit path when the skips arrive as scaled TENSORS -- the public
    apply_skip_connections / decode route; csrc/conv_generic.hip: tt_scaled_add16).  a is the decoder's own activation, b the skip: a
    tensor that crossed the module boundary, so its gradient leaves the loss-scaled region here (FP16_LOSS_SCALE: b's gradient is the
    TRUE one, divided by S; torch's own ops and Scale16Fn between here and the encoder's tap -- where S goes back on -- see true gradients)."""

    @staticmethod
    def forward(ctx, a, b):
        B, C, H, T = a.shape
        if b.dtype != a.dtype:
            raise TypeError('skip join of %s and %s tensors' % (a.dtype, b.dtype))
        y = new_cl16(B, C, H, T, a.device, a.dtype)
        check(lib16(a).tt_scaled_add16(ptr(a), ptr(b), None, 0, ptr(y), a.numel(), stream_ptr()), 'tt_scaled_add16')
        ctx.dtype = a.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        g = _as_cl16(dy, ctx.dtype)
        s = _ops.loss_scale(ctx.dtype)
        if s == 1.0 or not ctx.needs_input_grad[1]:
            return g, g
        gb = new_cl16(*g.shape, g.device, g.dtype)
        check(lib16(g).tt_scaled_add16(None, ptr(g), ptr(_device_scalar(1.0 / s, g.device)), 0, ptr(gb), g.numel(), stream_ptr()), 'tt_scaled_add16')
        return g, gb


class Scale16Fn(torch.autograd.Function):
    """s[idx] * e on a cl16 tensor (TimbreTrap.apply_skip_connections, reference modules.py:112) -- fp32 weight, 16-bit tensor.  Its
    input and output are tensors OUTSIDE the modules: true gradients in and out, no loss scale (see Add16Fn / GateTapFn)."""

    @staticmethod
    def forward(ctx, e, s, idx):
        B, C, H, T = e.shape
        s = _f32c(s)
        y = new_cl16(B, C, H, T, e.device, e.dtype)
        check(lib16(e).tt_scaled_add16(None, ptr(e), ptr(s), idx, ptr(y), e.numel(), stream_ptr()), 'tt_scaled_add16')
        ctx.idx = idx
        ctx.save_for_backward(e, s)
        return y

    @staticmethod
    def backward(ctx, dy):
        e, s = ctx.saved_tensors
        g = _as_cl16(dy, e.dtype)
        lib, st = lib16(e), stream_ptr()
        de = ds = None
        if ctx.needs_input_grad[0]:
            B, C, H, T = e.shape
            de = new_cl16(B, C, H, T, e.device, e.dtype)
            check(lib.tt_scaled_add16(None, ptr(g), ptr(s), ctx.idx, ptr(de), e.numel(), st), 'tt_scaled_add16')
        if ctx.needs_input_grad[1]:
            ds = torch.zeros_like(s)
            check(lib.tt_dot16(ptr(g), ptr(e), _off(ds, ctx.idx), e.numel(), st), 'tt_dot16')
        return de, ds, None


class SkipJoin:
    """A skip connection that has not been applied yet: (encoder embedding, the skip weights, which one, the embedding's GateLink).
    TimbreTrap.forward hands these to the decoder on the 16-bit path instead of the scaled tensors of apply_skip_connections: the
    product and the join are then ONE pass (SkipJoin16Fn) and the embedding serves both halves of a pair decode."""
    __slots__ = ('e', 'weights', 'idx', 'link', 'defer')

    def __init__(self, e, weights, idx, link=None, defer=False):
        self.e, self.weights, self.idx, self.link = e, weights, idx, link
        # defer (TimbreTrap.forward only, where encoder and decoder are one graph): the embedding's share of the join's backward may be left
        # to the backward of the encoder layer behind the embedding (GateLink.pending) -- see _join_backward
        self.defer = bool(defer)


def _join_backward(g, e, weights, idx, reps, link, param, want_e, want_w, defer):
    """The backward of a weighted skip join, out[r] = y[r] + weights[idx] * e (r < reps), for e and the weight; g = the incoming 16-bit
    gradient (it IS dy).  -> (de, value returned to autograd for the weights).
    Deferred form: where the embedding's other consumer is an encoder layer that accumulates (GateLink.accumulates) and the weight's
    gradient goes straight into the optimizer's flat buffer, NOTHING is computed here -- the arguments wait in link.pending until that
    layer's backward has written its data gradient dx, and ONE pass then does dx += w * (sum of the halves of g) [* ELU'(e)] and the
    weight's dot product (flush_pending): 2 g + e + dx read, dx written, where de written here + autograd's add moved 2 g + e read, de
    written, de + dx read, sum written."""
    if not want_e and not want_w:
        return None, None
    ds = rs = None
    if want_w:
        ds, rs = _grad_target(param)
    if (defer and _ops.SKIP_DEFER and want_e and link is not None and link.accumulates and rs is None and not torch.is_grad_enabled()):
        link.pending.append((g, e, weights, idx, reps, ds))
        return None, None
    de = new_cl16(*e.shape, e.device, e.dtype) if want_e else None
    gate = link is not None and link.gated
    check(lib16(e).tt_skip_join16_bwd(ptr(g), ptr(e), ptr(weights), idx, ptr(de), ptr(ds), e.numel(), reps, int(gate), stream_ptr()),
          'tt_skip_join16_bwd')
    return de, rs


def _riding_join(ctx, x0):
    """The one parked skip-join backward of ``ctx.link`` if it can ride on the level's gated first block (tt_wide_level_bwd_gated_join): the
    level gates, its first block has dilation 1, exactly one join is parked and its embedding IS the level's input; else None."""
    link = ctx.link
    pend = getattr(link, 'pending', None)
    if not _ops.SKIP_RIDE or not ctx.gate or not pend or len(pend) != 1 or ctx.dilations[0] != 1:
        return None
    g, e, weights, idx, reps, ds = pend[0]
    if e.data_ptr() != x0.data_ptr() or e.shape != x0.shape or g.dtype != x0.dtype or g.size(0) != reps * x0.size(0):
        return None
    return pend[0]


def flush_pending(link, dx):
    """Called by the backward of an encoder layer that consumes a linked tensor, after it has written the data gradient ``dx`` of that tensor
    (gated iff link.gated): fold the parked skip-join backwards into it (see _join_backward).  Inside the caller's loss_scaled scope."""
    if not getattr(link, 'pending', None):          # (None, nothing parked, or a link-like object of a stage-wise test)
        return
    pend, link.pending = link.pending, []
    for g, e, weights, idx, reps, ds in pend:
        if dx is None:                      # the layer's input wanted no gradient: only the weight's share is left to do
            if ds is not None:
                check(lib16(e).tt_skip_join16_bwd(ptr(g), ptr(e), ptr(weights), idx, None, ptr(ds), e.numel(), reps, 0, stream_ptr()), 'tt_skip_join16_bwd')
            continue
        flags = (1 if link.gated else 0) | 2
        check(lib16(e).tt_skip_join16_bwd(ptr(g), ptr(e), ptr(weights), idx, ptr(dx), ptr(ds), e.numel(), reps, flags, stream_ptr()), 'tt_skip_join16_bwd')


@instrumented('skipjoin16', lambda y, e, *a: 'C%d' % e.size(1))
@loss_scaled_backward(lambda ctx: ctx.saved_tensors[0].dtype)
class SkipJoin16Fn(torch.autograd.Function):
    """out = y + weights[idx] * e on cl16 tensors in one pass (tt_skip_join16_fwd; reference modules.py:112 and :569-589).  y may hold
    ``reps`` = 2 batches back to back (TimbreTrap.decode_pair) that both take e.  Backward, one pass (tt_skip_join16_bwd): dy is the
    incoming gradient itself, de = weights[idx] * (sum over the halves), d weights[idx] += <sum over the halves, e>.  ``link``: e is the RAW
    output of a 16-bit strided layer whose backward may take its gradient already gated (GateLink, read at backward time): de then
    carries ELU'(e) -- what GateTapFn + tt_gate16 did in two more passes."""

    @staticmethod
    def forward(ctx, y, e, weights, idx, link, defer):
        B, C, H, T = e.shape
        reps = y.size(0) // B
        ctx.defer = defer
        if y.dtype != e.dtype or y.shape[1:] != e.shape[1:] or reps * B != y.size(0) or reps not in (1, 2):
            raise ValueError('skip join of %s %s and %s %s tensors' % (tuple(y.shape), y.dtype, tuple(e.shape), e.dtype))
        out = new_cl16(reps * B, C, H, T, y.device, y.dtype)
        check(lib16(y).tt_skip_join16_fwd(ptr(y), ptr(e), ptr(weights), idx, ptr(out), e.numel(), reps, stream_ptr()), 'tt_skip_join16_fwd')
        ctx.idx, ctx.reps, ctx.link, ctx.param = idx, reps, link, weights
        ctx.save_for_backward(e, weights)
        return out

    @staticmethod
    def backward(ctx, g):
        e, weights = ctx.saved_tensors
        B, C, H, T = e.shape
        g = _as_cl16(g, e.dtype)
        de, rs = _join_backward(g, e, weights, ctx.idx, ctx.reps, ctx.link, ctx.param, ctx.needs_input_grad[1], ctx.needs_input_grad[2], ctx.defer)
        return g, de, rs, None, None, None
