"""fp32-class inference on split fp16 operands ("x3", csrc/conv_x3.hip): the thread-local scopes that select it and the no-grad launchers;
and, at the end, the opt-in split-operand TRAINING of the wide levels (X3LevelTrainFn, ops.X3_TRAIN).
Without autocast and without grad (evaluate.py:94-95, transcribe() / reconstruct()) the wide levels do not need the hidden
activations the fp32 backward reads, and the fp32 matrix instructions are what bounds tt_resblock_fwd: the level then runs on
(hi, lo) fp16 pairs -- fp32-level results (tests/test_gpu_x3.py: 2e-6 of the tensor's scale against float64) at the 16-bit matrix
rate.  TTRAP_X3_INFER=0 / ops.X3_INFER = False keeps the fp32 kernels."""

import ctypes
import threading

import torch

from .. import ops as _ops
from ... import _hip
from ..._hip import check, ptr, stream_ptr
from ._common import _f32c, _grad_target

_X3_LOCAL = threading.local()


def x3_inference():
    return (_ops.X3_INFER and not getattr(_X3_LOCAL, 'off', False) and not torch.is_grad_enabled() and _ops.precision() == 'fp32'
            and _ops.wide_storage() == 'fp32')


class _x3_scope:
    """``with`` scope that sets one flag of the calling thread (``flag``) and restores the previous value on the way out."""

    def __init__(self, enabled=True):
        self.enabled = enabled

    def __enter__(self):
        self.prev = getattr(_X3_LOCAL, self.flag, False)
        setattr(_X3_LOCAL, self.flag, bool(self.enabled))
        return self

    def __exit__(self, *exc):
        setattr(_X3_LOCAL, self.flag, self.prev)
        return False


class x3_disabled(_x3_scope):
    """Inside this scope the calling thread's no-grad fp32 forwards stay on the fp32 kernels (the range fallback below)."""
    flag = 'off'


def x3_range_ok(out):
    """
    The split representation holds |v| <= 65504 (hi = fp16(v)); beyond that -- activations or weights -- csrc/conv_x3.hip returns
    NON-FINITE values, never a finite wrong number, where the reference's fp32 evaluation stays finite.  Callers that took the
    split-operand path check their result with this (one read-only pass and one host sync per inference call) and, when it is not
    finite, repeat the computation inside ``x3_disabled()`` on the fp32 kernels: a genuinely non-finite result (NaN weights) comes
    out non-finite again, an out-of-range one finite -- the reference's answer either way (round-4 advisor finding).
    """
    return bool(torch.isfinite(out.float().sum()))


class x3_vouched_scope(_x3_scope):
    """Inside this scope an OUTER caller checks the final result of the no-grad forward once (TimbreTrap._inference: its logits;
    TimbreTrap.chunked_inference: the cross-faded coefficients of all chunks -- ONE reduction and ONE host sync per transcribe() /
    reconstruct()), so the levels that went fp32 -> split -> fp32 do not each vouch for their own range with a reduction and a sync of
    their own (round-5 advisor finding: eight per forward of a skip-connection model).  A value beyond the split format's range comes out
    NaN (hi = inf, lo = inf - inf) and stays NaN through every later layer, so the final check sees it."""
    flag = 'vouched'


def x3_vouched():
    return getattr(_X3_LOCAL, 'vouched', False)


def _x3_size_ok(B, H, T):
    """The launchers of csrc/conv_x3.hip count tiles in 32-bit integers (64-bit element offsets): B * H * T / 16 stays far below 2^31."""
    return B * H * T < 2 ** 34


class x3_chain_scope(_x3_scope):
    """
    Inside this scope (TimbreTrap._inference when there are no skip connections: the encoder's embeddings are dropped) the layers
    between two split-operand levels hand x3 tensors to each other -- torch.float16 tensors of shape (B, H, T, 2, C), the layout of
    csrc/conv_x3.hip -- instead of fp32 planar ones: no pack / unpack passes, strided layers on tt_x3_sconv_fwd / tt_x3_tconv_fwd.
    Such tensors never leave the model: every consumer without an x3 kernel converts (to_planar32).
    """
    flag = 'chain'


def x3_chain():
    return getattr(_X3_LOCAL, 'chain', False) and x3_inference()


def is_x3(t):
    return t.dtype == torch.float16 and t.dim() == 5 and t.size(3) == 2 and t.is_contiguous()


def from_x3(t):
    """x3 (B, H, T, 2, C) -> fp32 planar (B, C, H, T) (tt_x3_unpack: hi + lo 2^-11, exact)."""
    B, H, T, _, C = t.shape
    y = torch.empty((B, C, H, T), dtype=torch.float32, device=t.device)
    check(_hip.lib().tt_x3_unpack(ptr(t), ptr(y), B, C, H, T, stream_ptr()), 'tt_x3_unpack')
    return y


def _x3_blocks_ok(C, blocks):
    return (_ops.FUSED_RESBLOCK and 1 <= len(blocks) <= 8
            and all(b.conv1[0].weight.shape == (C, C, 3, 3) and b.conv2[0].weight.shape == (C, C, 1, 1) and 1 <= b.dilation <= 3
                    for b in blocks))


def _x3_params(x, blocks):
    """The blocks' (w1, b1, w2, b2) as contiguous fp32 tensors without a graph, and arr(j): the j-th of them over all blocks as a C pointer array."""
    params = [[_f32c(t.detach()) for t in (b.conv1[0].weight, b.conv1[0].bias, b.conv2[0].weight, b.conv2[0].bias)] for b in blocks]
    _hip.require_cuda(x, params[0][0])
    return params, lambda j: (ctypes.c_void_p * len(blocks))(*[p[j].data_ptr() for p in params])


def x3_level(x, blocks, out_x3=False):
    """block_n(...block1(x)) without an autograd graph: tt_x3_level_fwd.  x: fp32 planar (B,C,H,T) or an x3 tensor; returns an x3
    tensor if out_x3 (the caller's next layer takes one), else fp32 planar."""
    in_x3 = is_x3(x)
    if in_x3:
        B, H, T, _, C = x.shape
        if C not in _ops.X3_CHANNELS or not _x3_blocks_ok(C, blocks) or not _x3_size_ok(B, H, T):
            with x3_disabled():
                return _ops.residual_level(from_x3(x), blocks)
    else:
        x = _f32c(x)
        B, C, H, T = x.shape
        if not _x3_size_ok(B, H, T):
            with x3_disabled():
                return _ops.residual_level(x, blocks)
    lib, st = _hip.lib(), stream_ptr()
    n = len(blocks)
    params, arr = _x3_params(x, blocks)
    ws = torch.empty(lib.tt_x3_level_scratch_bytes(B, C, H, T), dtype=torch.uint8, device=x.device)
    y = (torch.empty((B, H, T, 2, C), dtype=torch.float16, device=x.device) if out_x3
         else torch.empty((B, C, H, T), dtype=torch.float32, device=x.device))
    if _hip.EVENT_LOG is not None:
        # bench.py's instrumented steps: the same launches as tt_x3_level_fwd, one at a time, each block between its own pair of events
        half = ws.numel() // 2
        buf = (ws[:half], ws[half:])
        cur = x
        if not in_x3:
            check(lib.tt_x3_pack(ptr(x), ptr(buf[0]), B, C, H, T, st), 'tt_x3_pack')
            cur = buf[0]
        for i, (b, p) in enumerate(zip(blocks, params)):
            last = i == n - 1
            dst = y if last else (buf[1] if cur is buf[0] else buf[0])
            with _hip.timed('x3_rb_fwd_C%d' % C):
                check(lib.tt_x3_rb_fwd(ptr(cur), ptr(p[0]), ptr(p[1]), ptr(p[2]), ptr(p[3]), ptr(dst), int(last and not out_x3), B, C, H, T,
                                       b.dilation, st), 'tt_x3_rb_fwd')
            cur = dst
        _ops.X3_SHAPES['x3_rb_fwd_C%d' % C] = (B, C, H, T)
        return y
    check(lib.tt_x3_level_fwd(n, ptr(x), int(in_x3), ptr(y), int(out_x3), arr(0), arr(1), arr(2), arr(3),
                              (ctypes.c_int * n)(*[b.dilation for b in blocks]), ptr(ws), B, C, H, T, st), 'tt_x3_level_fwd')
    return y


def x3n_level(x, blocks):
    """block_n(...block1(x)) of a NARROW level (C = 4, 8) without an autograd graph: tt_x3n_level_fwd, fp32 planar (B,C,H,T) in and
    out, split-operand tensors between the blocks."""
    x = _f32c(x)
    B, C, H, T = x.shape
    lib, st = _hip.lib(), stream_ptr()
    n = len(blocks)
    params, arr = _x3_params(x, blocks)
    ws = torch.empty(lib.tt_x3n_level_scratch_bytes(B, C, H, T), dtype=torch.uint8, device=x.device)
    y = torch.empty((B, C, H, T), dtype=torch.float32, device=x.device)
    if _hip.EVENT_LOG is not None:
        # bench.py's instrumented steps: the same launches, each block between its own pair of events
        half = ws.numel() // 2
        buf = (ws[:half], ws[half:])
        cur = x
        for i, (b, p) in enumerate(zip(blocks, params)):
            last = i == n - 1
            dst = y if last else buf[i & 1]
            with _hip.timed('x3n_rb_fwd_C%d' % C):
                check(lib.tt_x3n_rb_fwd(ptr(cur), int(i == 0), ptr(p[0]), ptr(p[1]), ptr(p[2]), ptr(p[3]), ptr(dst), int(last), B, C, H, T,
                                        b.dilation, st), 'tt_x3n_rb_fwd')
            cur = dst
        _ops.X3_SHAPES['x3n_rb_fwd_C%d' % C] = (B, C, H, T)
        return y
    check(lib.tt_x3n_level_fwd(n, ptr(x), ptr(y), arr(0), arr(1), arr(2), arr(3), (ctypes.c_int * n)(*[b.dilation for b in blocks]), ptr(ws),
                               B, C, H, T, st), 'tt_x3n_level_fwd')
    return y


def x3_strided_conv(x, w, b, out_x3):
    """EncoderBlock.sconv with split operands (tt_x3_sconv_fwd).  x: an x3 tensor (C = 16, 32) or fp32 planar (C = 8: the layer that
    enters the split-operand part); returns x3 (B, Hout, T, 2, 2C) or fp32 planar (B, 2C, Hout, T)."""
    pin = not is_x3(x)
    if pin:
        x = _f32c(x)
        B, C, H, T = x.shape
    else:
        B, H, T, _, C = x.shape
    Ho = (H - 4) // 2 + 1
    w, b = _f32c(w.detach()), _f32c(b.detach())
    _hip.require_cuda(x, w)
    y = (torch.empty((B, Ho, T, 2, 2 * C), dtype=torch.float16, device=x.device) if out_x3
         else torch.empty((B, 2 * C, Ho, T), dtype=torch.float32, device=x.device))
    with _hip.timed('x3_sconv_C%d' % C):
        check(_hip.lib().tt_x3_sconv_fwd(ptr(x), int(pin), ptr(w), ptr(b), ptr(y), int(not out_x3), B, C, H, T, stream_ptr()),
              'tt_x3_sconv_fwd')
    return y


def x3_transposed_conv(x, w, b, out_pad, out_x3):
    """DecoderBlock.tconv with split operands (tt_x3_tconv_fwd).  x: an x3 tensor with 2C = 32 channels or fp32 planar with 2C = 64;
    returns x3 (B, Hout, T, 2, C) or fp32 planar (B, C, Hout, T)."""
    pin = not is_x3(x)
    if pin:
        x = _f32c(x)
        B, C2, H, T = x.shape
    else:
        B, H, T, _, C2 = x.shape
    C, Ho = C2 // 2, 2 * H + 2 + out_pad
    w, b = _f32c(w.detach()), _f32c(b.detach())
    _hip.require_cuda(x, w)
    y = (torch.empty((B, Ho, T, 2, C), dtype=torch.float16, device=x.device) if out_x3
         else torch.empty((B, C, Ho, T), dtype=torch.float32, device=x.device))
    with _hip.timed('x3_tconv_C%d' % C):
        check(_hip.lib().tt_x3_tconv_fwd(ptr(x), int(pin), ptr(w), ptr(b), ptr(y), int(not out_x3), B, C, H, T, out_pad, stream_ptr()),
              'tt_x3_tconv_fwd')
    return y


def x3_latent_ok(C, D, w_enc=None, w_dec=None):
    return ((C, D) in _ops.X3_LATENT_SHAPES and (w_enc is None or (w_enc.dim() == 4 and w_enc.shape[:2] == (D, C) and w_enc.size(3) == 1))
            and (w_dec is None or (w_dec.dim() == 4 and w_dec.shape[:2] == (D + 1, C) and w_dec.size(3) == 1)))


def x3_latent_encode(top, w, b):
    """Encoder.convlat on an x3 embedding (B, E, T, 2, C) -> latents (B, D, T) fp32 (tt_x3_latent_encode)."""
    B, E, T, _, C = top.shape
    D = w.size(0)
    lib = _hip.lib()
    w = _f32c(w.detach())
    b = None if b is None else _f32c(b.detach())
    ws = torch.empty(lib.tt_x3_latent_scratch_bytes(C, E, D), dtype=torch.uint8, device=top.device)
    z = torch.empty((B, D, T), dtype=torch.float32, device=top.device)
    with _hip.timed('x3_latent_encode'):
        check(lib.tt_x3_latent_encode(ptr(top), ptr(w), ptr(b), ptr(z), ptr(ws), B, C, E, D, T, stream_ptr()), 'tt_x3_latent_encode')
    return z


def x3_latent_decode(z, w, b, fill, out_x3):
    """Decoder.convin + ELU with split operands: latents (B, D or D + 1, T) fp32 -> x3 (B, E, T, 2, C) or fp32 planar (tt_x3_latent_decode)."""
    z = _f32c(z)
    B, Dz, T = z.shape
    D, C, E = w.size(0) - 1, w.size(1), w.size(2)
    lib = _hip.lib()
    w = _f32c(w.detach())
    b = None if b is None else _f32c(b.detach())
    ws = torch.empty(lib.tt_x3_latent_scratch_bytes(C, E, D), dtype=torch.uint8, device=z.device)
    y = (torch.empty((B, E, T, 2, C), dtype=torch.float16, device=z.device) if out_x3
         else torch.empty((B, C, E, T), dtype=torch.float32, device=z.device))
    with _hip.timed('x3_latent_decode'):
        check(lib.tt_x3_latent_decode(ptr(z), Dz, float(fill) if fill is not None else 0.0, ptr(w), ptr(b), ptr(y), int(not out_x3), ptr(ws),
                                      B, C, E, D, T, stream_ptr()), 'tt_x3_latent_decode')
    return y


# ---- split-operand training of the wide levels (ops.X3_TRAIN) --------------------------------------------------------------------------

def x3_training(x, blocks):
    """ops.residual_level's test for the X3LevelTrainFn route: the switch, fp32 mode with fp32 storage, grad enabled and wanted by the input
    or a parameter, a width of ops.X3_TRAIN_CHANNELS, blocks and sizes the kernels take."""
    if not (_ops.X3_TRAIN and torch.is_grad_enabled() and _ops.precision() == 'fp32' and _ops.wide_storage() == 'fp32'):
        return False
    if not (x.dim() == 4 and x.is_cuda and x.dtype == torch.float32):
        return False
    C = x.size(1)
    if not (C in _ops.X3_CHANNELS and C in _ops.X3_TRAIN_CHANNELS and _x3_blocks_ok(C, blocks) and _x3_size_ok(x.size(0), x.size(2), x.size(3))):
        return False
    return x.requires_grad or any(p.requires_grad for b in blocks for p in (b.conv1[0].weight, b.conv1[0].bias, b.conv2[0].weight, b.conv2[0].bias))


class X3LevelTrainFn(torch.autograd.Function):
    """
    block_n(...block1(x)) of a wide level (C = 16, 32) with split operands in BOTH directions (csrc/conv_x3.hip, "training"): fp32 planar
    (B,C,H,T) in and out; inside, every activation -- and what is saved for backward: each block's input and hidden activation, as many
    bytes as the fp32 path saves -- is an x3 tensor.  The backward scales the incoming gradient by a power of two chosen on the device
    (tt_x3_grad_scale: no host sync), runs tt_x3_rb_bwd per block from the last to the first, and returns true (unscaled) gradients.
    Values beyond +-65504 come out non-finite (no fp32 fallback here: the caller's finite check on the loss catches it).
    Not @instrumented: its launches are timed one by one under 'x3_rb_{fwd,bwd}_train_C<C>'.
    """

    @staticmethod
    def forward(ctx, x, dilations, *params):
        x = _f32c(x)
        B, C, H, T = x.shape
        lib, st = _hip.lib(), stream_ptr()
        n = len(dilations)
        ps = [_f32c(p.detach()) for p in params]
        _hip.require_cuda(x, ps[0])
        new = lambda: torch.empty((B, H, T, 2, C), dtype=torch.float16, device=x.device)
        xs, hs = [new()], []
        check(lib.tt_x3_pack(ptr(x), ptr(xs[0]), B, C, H, T, st), 'tt_x3_pack')
        y = torch.empty_like(x)
        for i in range(n):
            last = i == n - 1
            w1, b1, w2, b2 = ps[4 * i:4 * i + 4]
            dst = y if last else new()
            h1 = new()
            with _hip.timed('x3_rb_fwd_train_C%d' % C):
                check(lib.tt_x3_rb_fwd_train(ptr(xs[i]), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(dst), int(last), ptr(h1), B, C, H, T,
                                             dilations[i], st), 'tt_x3_rb_fwd_train')
            hs.append(h1)
            if not last:
                xs.append(dst)
        ctx.dilations, ctx.params, ctx.n = tuple(dilations), params, n
        ctx.save_for_backward(*xs, *hs, *ps)
        return y

    @staticmethod
    def backward(ctx, dy):
        n = ctx.n
        saved = ctx.saved_tensors
        xs, hs, ps = saved[:n], saved[n:2 * n], saved[2 * n:]
        dy = _f32c(dy)
        B, C, H, T = dy.shape
        lib, st = _hip.lib(), stream_ptr()
        dev = dy.device
        scale = torch.empty(2, dtype=torch.float32, device=dev)
        sws = torch.empty(lib.tt_x3_grad_scale_scratch_bytes(), dtype=torch.uint8, device=dev)
        check(lib.tt_x3_grad_scale(ptr(dy), dy.numel(), ptr(scale), ptr(sws), st), 'tt_x3_grad_scale')
        new = lambda: torch.empty((B, H, T, 2, C), dtype=torch.float16, device=dev)
        cur = new()
        check(lib.tt_x3_pack_scaled(ptr(dy), ptr(cur), ptr(scale), B, C, H, T, st), 'tt_x3_pack_scaled')
        other = new() if n > 1 else None
        dx = torch.empty((B, C, H, T), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        ws = torch.empty(lib.tt_x3_rb_bwd_scratch_bytes(B, C, H, T), dtype=torch.uint8, device=dev)
        targets = [_grad_target(p) for p in ctx.params]
        for i in reversed(range(n)):
            first = i == 0
            w1, _, w2, b2 = ps[4 * i:4 * i + 4]
            (dw1, _), (db1, _), (dw2, _), (db2, _) = targets[4 * i:4 * i + 4]
            dst = dx if first else other
            with _hip.timed('x3_rb_bwd_train_C%d' % C):
                check(lib.tt_x3_rb_bwd(ptr(xs[i]), ptr(hs[i]), ptr(cur), ptr(w1), ptr(w2), ptr(b2), ptr(dst), int(first), ptr(dw1), ptr(db1),
                                       ptr(dw2), ptr(db2), ptr(scale), ptr(ws), B, C, H, T, ctx.dilations[i], st), 'tt_x3_rb_bwd')
            if not first:
                cur, other = dst, cur
        return (dx, None) + tuple(r for _, r in targets)


def x3_level_train(x, blocks):
    params = []
    for b in blocks:
        params += [b.conv1[0].weight, b.conv1[0].bias, b.conv2[0].weight, b.conv2[0].bias]
    return X3LevelTrainFn.apply(x, tuple(b.dilation for b in blocks), *params)
