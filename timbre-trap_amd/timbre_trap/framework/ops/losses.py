"""The objectives (squared-error, transcription), the activation maps and the magnitude / decibel launchers of the CQT wrapper."""

import torch

from .. import ops as _ops
from ... import _hip
from ..._hip import check, ptr, stream_ptr
from ._common import _f32c, instrumented

def _partials(device):
    return torch.empty(1024, dtype=torch.float64, device=device)


@instrumented('sqdiff', lambda a, *r: 'n')
class SqDiffLossFn(torch.autograd.Function):
    """loss = scale * sum((a - b)^2); gradients flow into both arguments.  With grad enabled the forward pass, which reads both operands
    anyway, also writes the gradient for an incoming scalar of 1 (tt_sqdiff_sum_grad); backward is a launch that checks the incoming scalar
    on the device and multiplies only if it is not 1 (tt_sqdiff_rescale) -- no second read of the operands.  A second backward through the
    same node (retain_graph) recomputes from the operands (tt_sqdiff_bwd)."""

    @staticmethod
    def forward(ctx, a, b, scale):
        _hip.require_cuda(a, b)
        a, b = _f32c(a), _f32c(b)
        loss = torch.empty((), dtype=torch.float32, device=a.device)
        need = (ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        ctx.grads = None
        if _ops.LOSS_FUSED and any(need) and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0:
            da = torch.empty_like(a) if need[0] else None
            db = torch.empty_like(b) if need[1] else None
            check(_hip.lib().tt_sqdiff_sum_grad(ptr(a), ptr(b), ptr(loss), ptr(_partials(a.device)), a.numel(), scale, ptr(da), ptr(db),
                                                stream_ptr()), 'tt_sqdiff_sum_grad')
            ctx.grads = (da, db)
        else:
            check(_hip.lib().tt_sqdiff_sum(ptr(a), ptr(b), ptr(loss), ptr(_partials(a.device)), a.numel(), scale,
                                           stream_ptr()), 'tt_sqdiff_sum')
        ctx.scale = scale
        ctx.save_for_backward(a, b)
        return loss

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = _f32c(g)
        if ctx.grads is not None:
            da, db = ctx.grads
            ctx.grads = None                                     # single use: autograd may accumulate into these buffers in place
            check(_hip.lib().tt_sqdiff_rescale(ptr(da), ptr(db), ptr(g), a.numel(), stream_ptr()), 'tt_sqdiff_rescale')
            return da, db, None
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        if da is not None or db is not None:
            check(_hip.lib().tt_sqdiff_bwd(ptr(a), ptr(b), ptr(g), ctx.scale, ptr(da), ptr(db), a.numel(),
                                           stream_ptr()), 'tt_sqdiff_bwd')
        return da, db, None


@instrumented('sqdiff2', lambda a, *r: 'n')
class SqDiff2Fn(torch.autograd.Function):
    """
    (scale * sum((a1 - b)^2), scale * sum((a2 - b)^2)): the two consistency terms (reference objectives.py:77-104), which share their
    non-detached second operand.  Same sums as two SqDiffLossFn; the backward is ONE pass (tt_sqdiff2_bwd) that writes the gradient
    of b once, as the sum of both terms -- two SqDiffLossFn left that sum to autograd (an extra elementwise pass over the logits).
    """

    @staticmethod
    def forward(ctx, a1, a2, b, scale):
        _hip.require_cuda(a1, b)
        # tt_sqdiff2_bwd reads 16 bytes per lane: a contiguous view at an odd storage offset (a batch slice ``x[k:]`` whose offset is
        # not a multiple of four floats) is copied once here rather than failing in backward after the forward has succeeded
        a1, a2, b = (t if t.data_ptr() % 16 == 0 else t.clone() for t in (_f32c(a1), _f32c(a2), _f32c(b)))
        lib, st = _hip.lib(), stream_ptr()
        l1 = torch.empty((), dtype=torch.float32, device=b.device)
        l2 = torch.empty((), dtype=torch.float32, device=b.device)
        ctx.grads = None
        if _ops.LOSS_FUSED and any(ctx.needs_input_grad[:3]):
            # one pass over a1, a2, b for both sums and the three gradients at unit incoming scale (tt_sqdiff2_sum_grad; see SqDiffLossFn)
            da1, da2 = torch.empty_like(a1), torch.empty_like(a2)
            db = torch.empty_like(b) if ctx.needs_input_grad[2] else None
            check(lib.tt_sqdiff2_sum_grad(ptr(a1), ptr(a2), ptr(b), ptr(l1), ptr(l2), ptr(torch.empty(2048, dtype=torch.float64, device=b.device)),
                                          b.numel(), scale, ptr(da1), ptr(da2), ptr(db), st), 'tt_sqdiff2_sum_grad')
            ctx.grads = (da1, da2, db)
        else:
            check(lib.tt_sqdiff_sum(ptr(a1), ptr(b), ptr(l1), ptr(_partials(b.device)), b.numel(), scale, st), 'tt_sqdiff_sum')
            check(lib.tt_sqdiff_sum(ptr(a2), ptr(b), ptr(l2), ptr(_partials(b.device)), b.numel(), scale, st), 'tt_sqdiff_sum')
        ctx.scale = scale
        ctx.save_for_backward(a1, a2, b)
        return l1, l2

    @staticmethod
    def backward(ctx, g1, g2):
        a1, a2, b = ctx.saved_tensors
        g1 = None if g1 is None else _f32c(g1)
        g2 = None if g2 is None else _f32c(g2)
        if ctx.grads is not None:
            da1, da2, db = ctx.grads
            ctx.grads = None
            check(_hip.lib().tt_sqdiff2_rescale(ptr(da1), ptr(da2), ptr(db), ptr(g1), ptr(g2), b.numel(), stream_ptr()), 'tt_sqdiff2_rescale')
            return (da1 if ctx.needs_input_grad[0] else None, da2 if ctx.needs_input_grad[1] else None, db, None)
        da1 = torch.empty_like(a1) if ctx.needs_input_grad[0] else None
        da2 = torch.empty_like(a2) if ctx.needs_input_grad[1] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[2] else None
        if da1 is not None or da2 is not None or db is not None:
            check(_hip.lib().tt_sqdiff2_bwd(ptr(a1), ptr(a2), ptr(b), ptr(g1), ptr(g2), ctx.scale, ptr(da1), ptr(da2), ptr(db), b.numel(),
                                            stream_ptr()), 'tt_sqdiff2_bwd')
        return da1, da2, db, None


@instrumented('act', lambda c: 'n')
class ActivationsFn(torch.autograd.Function):
    """tanh(|re + i im|) over the channel pair (TimbreTrap.to_activations, modules.py:287)."""

    @staticmethod
    def forward(ctx, coefficients):
        _hip.require_cuda(coefficients)
        c = _f32c(coefficients)
        B, _, F, T = c.shape
        act = torch.empty((B, F, T), dtype=torch.float32, device=c.device)
        check(_hip.lib().tt_activations_fwd(ptr(c), ptr(act), B, F, T, stream_ptr()), 'tt_activations_fwd')
        ctx.save_for_backward(c, act)
        return act

    @staticmethod
    def backward(ctx, dact):
        c, act = ctx.saved_tensors
        B, _, F, T = c.shape
        dc = torch.empty_like(c)
        check(_hip.lib().tt_activations_bwd(ptr(c), ptr(act), ptr(_f32c(dact)), ptr(dc), B, F, T, stream_ptr()),
              'tt_activations_bwd')
        return dc


@instrumented('act1', lambda c: 'n')
class Activations1Fn(torch.autograd.Function):
    """tanh of the 1-channel magnitude logits, any shape (TimbreTrapMag.to_activations, modules.py:994)."""

    @staticmethod
    def forward(ctx, coefficients):
        _hip.require_cuda(coefficients)
        c = _f32c(coefficients)
        act = torch.empty_like(c)
        check(_hip.lib().tt_activations1_fwd(ptr(c), ptr(act), c.numel(), stream_ptr()), 'tt_activations1_fwd')
        ctx.save_for_backward(act)
        return act

    @staticmethod
    def backward(ctx, dact):
        act, = ctx.saved_tensors
        dc = torch.empty_like(act)
        check(_hip.lib().tt_activations1_bwd(ptr(act), ptr(_f32c(dact)), ptr(dc), act.numel(), stream_ptr()), 'tt_activations1_bwd')
        return dc


def magnitude(coefficients):
    """(..., 2, F, T) fp32 re / im planes -> (..., F, T) magnitudes (tt_magnitude); no autograd."""
    c = _f32c(coefficients)
    F, T = c.shape[-2:]
    out = torch.empty(c.shape[:-3] + (F, T), dtype=torch.float32, device=c.device)
    check(_hip.lib().tt_magnitude(ptr(c), ptr(out), c.numel() // (2 * F * T), F * T, stream_ptr()), 'tt_magnitude')
    return out


def decibels(m, rescale=True):
    """Per item of dim 0: 20 log10(max(m, 1e-10)) floored 80 dB below the item's maximum, optionally 1 + (d - max) / 80 (tt_decibels);
    no autograd."""
    m = _f32c(m)
    lib = _hip.lib()
    ws = torch.empty(lib.tt_decibels_scratch_bytes(m.size(0)), dtype=torch.uint8, device=m.device)
    out = torch.empty_like(m)
    check(lib.tt_decibels(ptr(m), ptr(out), m.size(0), m.numel() // m.size(0), int(bool(rescale)), ptr(ws), stream_ptr()), 'tt_decibels')
    return out


@instrumented('trn', lambda e, *r: 'n')
class TranscriptionLossFn(torch.autograd.Function):
    """compute_transcription_loss (objectives.py:36-74); gradient w.r.t. the estimate only."""

    @staticmethod
    def forward(ctx, estimate, target, weighted):
        _hip.require_cuda(estimate, target)
        e, t = _f32c(estimate), _f32c(target)
        B, F, T = e.shape
        loss = torch.empty((), dtype=torch.float32, device=e.device)
        fs = torch.empty((B, T), dtype=torch.float32, device=e.device) if weighted else None
        ctx.grad = None
        if _ops.LOSS_FUSED and ctx.needs_input_grad[0]:               # the gradient for an incoming scalar of 1 in the same pass (see SqDiffLossFn)
            de = torch.empty_like(e)
            check(_hip.lib().tt_transcription_loss_fwd_grad(ptr(e), ptr(t), ptr(loss), ptr(fs), ptr(_partials(e.device)), ptr(de),
                                                            B, F, T, int(weighted), stream_ptr()), 'tt_transcription_loss_fwd_grad')
            ctx.grad = de
        else:
            check(_hip.lib().tt_transcription_loss_fwd(ptr(e), ptr(t), ptr(loss), ptr(fs), ptr(_partials(e.device)),
                                                       B, F, T, int(weighted), stream_ptr()), 'tt_transcription_loss_fwd')
        ctx.weighted = weighted
        ctx.save_for_backward(e, t, fs)
        return loss

    @staticmethod
    def backward(ctx, g):
        e, t, fs = ctx.saved_tensors
        B, F, T = e.shape
        if ctx.grad is not None:
            de, ctx.grad = ctx.grad, None
            check(_hip.lib().tt_sqdiff_rescale(ptr(de), None, ptr(_f32c(g)), de.numel(), stream_ptr()), 'tt_sqdiff_rescale')
            return de, None, None
        de = torch.empty_like(e)
        check(_hip.lib().tt_transcription_loss_bwd(ptr(e), ptr(t), ptr(fs), ptr(_f32c(g)), ptr(de), B, F, T,
                                                   int(ctx.weighted), stream_ptr()), 'tt_transcription_loss_bwd')
        return de, None, None
