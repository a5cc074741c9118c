"""The FiLM layer of TimbreTrapFiLM (csrc/film.hip): a per-channel affine map of the fp32 latents, switched by a two-entry condition.
Latents are fp32 (B, D, T) on every route -- the 16-bit latent heads return and take fp32 (LatEnc16Fn / LatDec16Fn) -- so this one
Function serves the fp32 path and both autocast dtypes, and the gradient it receives is already unscaled (no loss_scaled_backward)."""

import ctypes

import torch

from ... import _hip
from ..._hip import check, ptr, stream_ptr
from ._common import _f32c, _grad_target


def _host_cond(cond, reps):
    """The conditions as the kernels take them: a host array of reps x 2 floats."""
    values = [float(v) for v in cond]
    if len(values) != 2 * reps:
        raise ValueError('FiLM takes two condition entries per pass, got %d for %d' % (len(values), reps))
    return (ctypes.c_float * 4)(*values)


class FilmFn(torch.autograd.Function):
    """
    x (..., D, T) -> x * G_r + Bt_r with G_r = gamma(c_r), Bt_r = beta(c_r) per channel (reference modules.py:880-887), every product and
    sum rounded on its own like the reference's.  ``cond``: 2 * reps host floats (c_00, c_01[, c_10, c_11]).  ``reps`` = 2 is the pair
    form for x (B, D, T): ONE read of the latents, result (2 B, D, T) with condition 0 in the first half and condition 1 in the second --
    what TimbreTrapFiLM.decode_pair hands the decoder; its backward adds the two halves' gradients in the same pass.
    """

    @staticmethod
    def forward(ctx, x, gw, gb, bw, bb, cond, reps=1):
        _hip.require_cuda(x, gw, gb, bw, bb)
        if reps not in (1, 2) or x.dim() < 2 or (reps == 2 and x.dim() != 3):
            raise ValueError('FilmFn takes (..., D, T) latents, and (B, D, T) ones in its pair form; got %s, reps %r' % (tuple(x.shape), reps))
        x = _f32c(x)
        D, T = x.size(-2), x.size(-1)
        B = x.numel() // (D * T) if D * T else 0
        if B == 0 or gw.shape != (D, 2) or bw.shape != (D, 2) or gb.shape != (D,) or bb.shape != (D,):
            raise ValueError('FiLM over latents %s needs gamma / beta of nn.Linear(2, %d)' % (tuple(x.shape), D))
        ctx.params = (gw, gb, bw, bb)
        gw, gb, bw, bb = (_f32c(p.detach()) for p in (gw, gb, bw, bb))
        ctx.cond, ctx.reps, ctx.dims = _host_cond(cond, reps), reps, (B, D, T)
        y = torch.empty((reps * x.size(0),) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
        with _hip.timed('film_fwd', clips=B):
            check(_hip.lib().tt_film_fwd(ptr(x), ptr(gw), ptr(gb), ptr(bw), ptr(bb), ctx.cond, ptr(y), B, D, T, reps, stream_ptr()), 'tt_film_fwd')
        ctx.save_for_backward(x, gw, gb)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gw, gb = ctx.saved_tensors
        B, D, T = ctx.dims
        lib, st = _hip.lib(), stream_ptr()
        dy = _f32c(dy)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        bufs, rets, ws = [None] * 4, [None] * 4, None
        if any(ctx.needs_input_grad[1:5]):
            # the four gradients come out of one reduction: all or none (a frozen one lands in a buffer nobody reads)
            for i, p in enumerate(ctx.params):
                bufs[i], rets[i] = _grad_target(p)
            ws = torch.empty(lib.tt_film_scratch_bytes(B, D, T, ctx.reps), dtype=torch.uint8, device=x.device)
        with _hip.timed('film_bwd', clips=B):
            check(lib.tt_film_bwd(ptr(x), ptr(dy), ptr(gw), ptr(gb), ctx.cond, ptr(dx), ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3]),
                                  ptr(ws), B, D, T, ctx.reps, st), 'tt_film_bwd')
        return (dx, rets[0], rets[1], rets[2], rets[3], None, None)


def film_modulate(x, gw, gb, bw, bb, cond, reps=1):
    """FilmFn on the parameters of FiLM.gamma / FiLM.beta (the Parameter objects themselves: their gradients land through _grad_target)."""
    return FilmFn.apply(x, gw, gb, bw, bb, tuple(cond), reps)
