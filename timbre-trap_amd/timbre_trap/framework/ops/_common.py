"""What the families of bindings share: constants, lib16, gradient targets, the loss-scaled-backward and event-log class decorators."""

import ctypes
from dataclasses import dataclass

import torch

from .. import ops as _ops          # the package: switches and mode functions are read from it at call time, never copied
from ... import _hip
from ..._hip import check, ptr

ACT_NONE, ACT_ELU = 0, 1
# the output nonlinearities of the magnitude variants' decoders (include/ttrap.h TT_ACT_RELU / TT_ACT_SIGMOID; tt_conv2d's epilogue)
ACT_RELU, ACT_SIGMOID = 2, 3


class _HalfLib:
    """The fp16 twins of the 16-bit entry points (include/ttrap.h "fp16 twins"): attribute tt_x resolves to tt_x_h."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name + '_h' if name in _hip.HALF_TWINS else name)


def lib16(t):
    """The library as seen by a 16-bit channels-last tensor (or dtype) ``t``: bf16 -> the plain entry points, fp16 -> the _h twins."""
    dtype = t if isinstance(t, torch.dtype) else t.dtype
    if dtype == torch.float16:
        return _HalfLib(_hip.lib())
    if dtype != torch.bfloat16:
        raise TypeError('16-bit channels-last kernels take bfloat16 or float16 tensors, got %s' % (dtype,))
    return _hip.lib()


# ops.FP16_LOSS_SCALE: static loss scale of the fp16 channels-last backward (power of two; 1 = off).  The reference runs its train step under
# ``torch.autocast('cuda')`` = float16 WITHOUT a GradScaler (experiments/train.py:415): the loss is a mean over B x T frames, so the
# activation gradients of the first encoder levels are ~1e-7 at training batch sizes -- below fp16's normal range (6.1e-5), where every
# halving costs a bit (round 4 measured parameter gradients 3.4e-2 median / 0.53 worst off the fp32 path at 64 clips).  Here every
# activation gradient that ENTERS the fp16 region (the backward of Decoder.convout, of Encoder.convlat, an fp32 gradient arriving at a
# 16-bit layer) is multiplied by S, and everything that LEAVES it (weight / bias gradients, the gradient of the latents, of the
# encoder's input coefficients, of the skip weights) by 1 / S inside the kernels' own fp32 epilogues (include/ttrap.h:
# tt_set_loss_scale) -- an exact identity in real arithmetic, invisible to the caller: ``.grad`` holds the true gradient, no scaler
# object, the unmodified train.py benefits.  An overflow (inf / NaN gradient norm) makes FusedAdamW skip the step, as GradScaler would.
# bf16 has fp32's exponent range and is never scaled.
class loss_scaled:
    """``with loss_scaled(dtype):`` around the BACKWARD calls of the 16-bit layers: sets the calling thread's loss scale in the library
    (thread-local there: autograd runs backward on its own threads) and restores the previous value."""

    def __init__(self, dtype):
        self.s = _ops.loss_scale(dtype)
        self.prev = None

    def __enter__(self):
        if self.s != 1.0:
            self.prev = _hip.lib().tt_set_loss_scale(self.s)
        return self

    def __exit__(self, *exc):
        if self.prev is not None:
            _hip.lib().tt_set_loss_scale(self.prev)
        return False


@dataclass(frozen=True)
class ConvCfg:
    """Geometry of one layer. kind 'conv' = nn.Conv2d, 'tconv' = nn.ConvTranspose2d (H only)."""
    KH: int
    KW: int
    stride: int = 1
    dil: int = 1
    pad_h: int = 0
    pad_w: int = 0
    kind: str = 'conv'
    out_pad: int = 0
    act: int = ACT_NONE


def _off(t, elements):
    return ctypes.c_void_p(t.data_ptr() + 4 * elements)


def _f32c(t):
    """``t`` as the kernels read it: contiguous fp32 (``t`` itself when it already is; None stays None)."""
    if t is None:
        return None
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _channel_sum(x, db, B, C, inner, st):
    """db[c] += sum of x viewed as (B, C, inner) over b and inner (tt_channel_sum_ws: fixed summation order, through a workspace)."""
    ws = torch.empty(2 * C + 2048, dtype=torch.float32, device=x.device)
    check(_hip.lib().tt_channel_sum_ws(ptr(x), ptr(db), B, C, inner, ptr(ws), st), 'tt_channel_sum_ws')


def _grad_target(p):
    """
    Where a backward kernel accumulates the gradient of parameter ``p``: (buffer, value returned to autograd).
    FusedAdamW keeps every ``.grad`` as a view of ONE flat fp32 buffer and tags its parameters; their kernels then add
    straight into that view (all weight-gradient entry points accumulate, +=) and autograd gets ``None`` -- no zero-fill
    and no ``grad += new`` launch per parameter use (~740 five-microsecond launches per train step).  Any other tensor
    gets a fresh zero buffer that is returned as usual.
    """
    if not p.requires_grad:
        # a parameter frozen after the optimizer tagged it: the kernels still need somewhere to write, but nothing may reach the
        # flat gradient buffer (it would be clipped, averaged and applied) and autograd wants no gradient for it
        return torch.zeros(p.shape, dtype=torch.float32, device=p.device), None
    g = p.grad if getattr(p, '_ttrap_accumulate', False) else None
    if g is not None and g.dtype == torch.float32 and g.is_contiguous() and g.shape == p.shape and g.device == p.device:
        p._ttrap_touched = True           # FusedAdamW: this slot has a gradient of the current step (utils/optim.py, _nograd)
        return g, None
    z = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
    return z, z


_SCALARS = {}


def _device_scalar(value, device):
    """A one-element fp32 device tensor holding ``value`` (cached: the loss scale and its reciprocal as kernel scale arguments)."""
    key = (float(value), str(device))
    t = _SCALARS.get(key)
    if t is None:
        t = _SCALARS[key] = torch.full((1,), float(value), dtype=torch.float32, device=device)
    return t


def loss_scaled_backward(dtype_of):
    """Class decorator: run cls.backward inside ``loss_scaled(<element type of the layer's 16-bit tensors>)``: its kernels then treat
    incoming 16-bit gradients as scaled and unscale every fp32 result (the edge convolutions do it around their own calls)."""
    def wrap(cls):
        bwd = cls.backward

        def backward(ctx, *grads):
            with loss_scaled(dtype_of(ctx)):
                return bwd(ctx, *grads)
        cls.backward = staticmethod(backward)
        cls._tt_loss_scaled = True
        return cls
    return wrap


def instrumented(name, keyfn):
    """Class decorator (outermost): when _hip.EVENT_LOG is a dict (bench.py), each forward / backward is bracketed by an event pair
    recorded on the launch stream under '<name>_fwd|bwd_<shape tag>' (no cost when logging is off)."""
    def wrap(cls):
        fwd, bwd = cls.forward, cls.backward

        def forward(ctx, *args):
            if _hip.EVENT_LOG is None:
                return fwd(ctx, *args)
            ctx._tt_key = keyfn(*args)
            ctx._tt_clips = args[0].size(0) if (torch.is_tensor(args[0]) and args[0].dim() >= 3) else None
            with _hip.timed('%s_fwd_%s' % (name, ctx._tt_key), clips=ctx._tt_clips):
                return fwd(ctx, *args)

        def backward(ctx, *grads):
            if _hip.EVENT_LOG is None:
                return bwd(ctx, *grads)
            with _hip.timed('%s_bwd_%s' % (name, getattr(ctx, '_tt_key', '?')), clips=getattr(ctx, '_tt_clips', None)):
                return bwd(ctx, *grads)
        cls.forward = staticmethod(forward)
        cls.backward = staticmethod(backward)
        cls._tt_event = name
        return cls
    return wrap
