"""
torch.autograd bindings of the gfx950 kernels (C ABI: include/ttrap.h) and the routing in front of them.  Which switches exist: the block
right below.  Which kernel a call takes: the routing functions at the end of this file (what modules.py / objectives.py / cqtwrapper.py
call).  What a binding does: the family modules -- fp32 (channel-planar), cl16 / level16 / skip (16-bit channels-last), x3 (split-operand
inference), losses, film (the FiLM layer of TimbreTrapFiLM).  Every Function owns a forward and a hand-written backward that call straight into libttrap_hip.so on the current HIP
stream; torch only allocates the tensors.  Nothing here has a CPU path -- tensors must live on the GPU.
"""

import math
import os

import torch

# ---- switches: assignable at run time (ops.PRECISION = 'fp32'); the family modules read them through the package, never a copy --------
# The fused ResidualConv2dBlock kernels (csrc/conv_mfma.hip, csrc/conv_small.hip) are the default; TTRAP_FUSED=0 composes
# the block from the general convolution kernels instead (used to cross-check the two on the GPU).
FUSED_RESBLOCK = os.environ.get('TTRAP_FUSED', '1') != '0'
# Keep the hidden activation of every residual block for backward (one more (B,C,H,T) tensor per block, no 3x3
# recompute).  TTRAP_SAVE_HIDDEN=0 recomputes instead and halves the residual-block activation memory.
SAVE_HIDDEN = os.environ.get('TTRAP_SAVE_HIDDEN', '1') != '0'
# Arithmetic of the wide (C >= 16) residual blocks on the matrix cores:
#   'fp32'    v_mfma_f32_16x16x4_f32, exact fp32 -- what every parity test pins
#   'bf16x3'  fp32 tensors, every operand fed as hi + lo bf16 (three products): fp32-class results at 16/3 of the fp32 rate
#   'bf16'    operands rounded to bf16, fp32 accumulation (v_mfma_f32_16x16x32_bf16)
#   'fp16'    the same kernels with fp16 elements (v_mfma_f32_16x16x32_f16; the _h entry points of include/ttrap.h)
#   'auto'    (default) inside a ``torch.autocast('cuda')`` region the region's own dtype ('fp16' for torch's default, as the reference's
#             train step runs; 'bf16' for dtype=torch.bfloat16, as bench.py runs) and 'fp32' outside, like the reference's evaluation
PRECISION = os.environ.get('TTRAP_PRECISION', 'auto')
# Storage of the activations INSIDE the wide levels (C = 16, 32: the three residual blocks of an Encoder/DecoderBlock):
#   'fp32'  channel-planar fp32 tensors, one ResBlockFn per block (any precision above)
#   'bf16'  bf16 channel-innermost tensors in HBM, csrc/conv_wide_bf16.hip: the "bf16 MFMA conv path" of BASELINE config[2].
#   'fp16'  the same with fp16 elements.
# Default: follows the precision ('bf16' / 'fp16' mean 16-bit operands AND 16-bit storage); TTRAP_WIDE_STORAGE overrides.
WIDE_STORAGE = os.environ.get('TTRAP_WIDE_STORAGE', '')
# Static loss scale of the fp16 channels-last backward (power of two; 1 = off; bf16 is never scaled): see _common.loss_scaled.
FP16_LOSS_SCALE = float(os.environ.get('TTRAP_FP16_LOSS_SCALE', '4096'))
# TTRAP_LEVEL_RECOMPUTE=1: the memory-saving fused backward of the wide levels C = 16, 32 (level16.py); computed once, here
RECOMPUTE_CHANNELS = (16, 32) if os.environ.get('TTRAP_LEVEL_RECOMPUTE', '0') == '1' else ()
# TTRAP_LEVEL_BWD=0: one tt_wide_rb_bwd call (with its own reduce launch) per block instead of tt_wide_level_bwd (A/B switch)
LEVEL_BWD = os.environ.get('TTRAP_LEVEL_BWD', '1') != '0'
# TTRAP_PREGATE=0: no layer takes its gradient already multiplied by its own ELU derivative (cl16.GateLink; A/B)
PREGATE = os.environ.get('TTRAP_PREGATE', '1') != '0'
# TTRAP_SKIP_FUSED=0: scale and join as two passes per decode, decodes one by one (A/B)
SKIP_FUSED = os.environ.get('TTRAP_SKIP_FUSED', '1') != '0'
# TTRAP_SKIP_DEFER=0: every skip join writes the embedding's gradient in its own backward and autograd adds it to the encoder level's
# data gradient (A/B)
SKIP_DEFER = os.environ.get('TTRAP_SKIP_DEFER', '1') != '0'
# TTRAP_SKIP_RIDE=0: a parked skip-join backward is applied by a pass of its own (flush_pending) instead of riding on the gated epilogue
# of the encoder level's first block (A/B)
SKIP_RIDE = os.environ.get('TTRAP_SKIP_RIDE', '1') != '0'
# TTRAP_SKIP_FOLD=0: the join behind a DecoderBlock as a pass of its own (SkipJoin16Fn) instead of the epilogue of the level's last
# block (A/B)
SKIP_FOLD = os.environ.get('TTRAP_SKIP_FOLD', '1') != '0'
# TTRAP_X3_INFER=0: the no-grad fp32 forward keeps the fp32 kernels instead of split fp16 operands (x3.py)
X3_INFER = os.environ.get('TTRAP_X3_INFER', '1') != '0'
# TTRAP_X3N_INFER=0: the narrow levels stay on the exact-fp32 kernels (A/B, bench.py)
X3N_INFER = os.environ.get('TTRAP_X3N_INFER', '1') != '0'
# TTRAP_X3_TRAIN=1 (default off): in fp32 mode the wide levels TRAIN on split fp16 operands too -- forward with saved x3 activations and a
# split-operand backward (x3.X3LevelTrainFn): fp32-class gradients without the fp32 matrix instructions.  Values beyond +-65504 come out
# non-finite and there is no fp32 fallback under grad (it would take a host sync per level): check the loss for finiteness.
X3_TRAIN = os.environ.get('TTRAP_X3_TRAIN', '0') == '1'
# TTRAP_LOSS_FUSED=0: the squared-error losses compute their gradients in backward from the saved operands (A/B)
LOSS_FUSED = os.environ.get('TTRAP_LOSS_FUSED', '1') != '0'

FUSED_CHANNELS = (4, 8, 16, 32)
WIDE_CHANNELS = (4, 8, 16, 32)        # every level of the model (C = 4 needs an even number of frames)
CL16_CHANNELS = (4, 8, 16, 32, 64)
X3_CHANNELS = (16, 32)
# widths on the X3_TRAIN route: those whose level (forward + backward) is faster than the fp32 kernels by more than the round-to-round spread
# (tools/kb_x3_train.py, profiles/kb_x3_train.txt: C = 32 1.70x, C = 16 1.18x)
X3_TRAIN_CHANNELS = (16, 32)
X3N_CHANNELS = (4, 8)                 # the narrow levels: lane-per-pixel split-operand blocks (tt_x3n_level_fwd), fp32 planar in and out
X3_LATENT_SHAPES = ((64, 128), (32, 32))          # (channels of the top embedding, latent size) with split-operand latent heads
X3_SHAPES = {}                        # event key -> (B, C, H, T) of the last instrumented call (bench.py's roofline_x3_fwd)


def precision():
    """The arithmetic in force for the call being made: PRECISION with 'auto' resolved against the autocast state."""
    if PRECISION == 'auto':
        if not torch.is_autocast_enabled('cuda'):
            return 'fp32'
        return 'fp16' if torch.get_autocast_dtype('cuda') == torch.float16 else 'bf16'
    if PRECISION not in ('fp32', 'bf16', 'fp16', 'bf16x3'):
        raise ValueError('TTRAP_PRECISION / ops.PRECISION must be auto, fp32, bf16x3, bf16 or fp16, got %r' % (PRECISION,))
    return PRECISION


def wide_storage():
    p = precision()
    mode = WIDE_STORAGE or (p if p in ('bf16', 'fp16') else 'fp32')
    if mode not in ('fp32', 'bf16', 'fp16'):
        raise ValueError('TTRAP_WIDE_STORAGE / ops.WIDE_STORAGE must be fp32, bf16 or fp16, got %r' % (mode,))
    return mode


def cl16_mode():
    """True where the layers run on 16-bit channels-last activations (either element type)."""
    return wide_storage() in ('bf16', 'fp16')


def cl16_dtype():
    """Element type of the 16-bit channels-last activations a forward creates from fp32 inputs in the current mode."""
    return torch.float16 if wide_storage() == 'fp16' else torch.bfloat16


def loss_scale(dtype):
    """The factor carried by the 16-bit activation gradients of element type ``dtype`` during backward."""
    if dtype != torch.float16 or FP16_LOSS_SCALE == 1.0:
        return 1.0
    s = float(FP16_LOSS_SCALE)
    if not (1.0 <= s <= 2.0 ** 24) or math.frexp(s)[0] != 0.5:
        raise ValueError('TTRAP_FP16_LOSS_SCALE / ops.FP16_LOSS_SCALE must be a power of two in [1, 2^24], got %r' % (FP16_LOSS_SCALE,))
    return s


def _flags():
    # the fp32-tensor kernels (shapes without a 16-bit channels-last kernel) know bf16 operand rounding only: fp16 mode takes it too
    return {'fp32': 0, 'bf16': 1, 'fp16': 1, 'bf16x3': 2}[precision()]


# ---- the bindings (after the switches: the family modules import this package back) -----------------------------------------------------

from ._common import ACT_ELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, ConvCfg, _channel_sum, _device_scalar, _f32c, _grad_target, _off, lib16, loss_scaled  # noqa
from .fp32 import AddFn, ConvFn, LatentDecodeFn, LatentEncodeFn, ResBlockFn, ScaleFn, StridedConvFn, TransposedConvFn  # noqa: E402,F401
from .cl16 import (ConvIn16Fn, ConvIn16x1Fn, ConvOut16Fn, ConvOut16PairFn, ConvOut16x1Fn, ConvOut16x1PairFn, GateLink, GateTapFn, ToCL16Fn,  # noqa
                   ToPlanar32Fn, _as_cl16, _cl16_ok, _pack, _unpack, gate_link, is_cl16, new_cl16)
from .skip import Add16Fn, Scale16Fn, SkipJoin, SkipJoin16Fn, _join_backward, _riding_join, flush_pending  # noqa: E402,F401
from .level16 import LatDec16Fn, LatEnc16Fn, Level16Fn, Level16JoinFn, SConv16Fn, TConv16Fn, WideLevelFn  # noqa: E402,F401
from .x3 import (X3LevelTrainFn, _x3_blocks_ok, _x3_size_ok, from_x3, is_x3, x3_chain, x3_chain_scope, x3_disabled, x3_inference,  # noqa: E402,F401
                 x3_latent_decode, x3_latent_encode, x3_latent_ok, x3_level, x3_level_train, x3_range_ok, x3_strided_conv, x3_training,
                 x3_transposed_conv, x3_vouched, x3_vouched_scope, x3n_level)
from .losses import Activations1Fn, ActivationsFn, SqDiff2Fn, SqDiffLossFn, TranscriptionLossFn, decibels, magnitude  # noqa: E402,F401
from .film import FilmFn, film_modulate  # noqa: E402,F401


# ---- routing: which kernel a call takes ---------------------------------------------------------------------------------------------------

def _i32_ok(x, channels=None):
    """The bf16 kernels index one clip with 32-bit offsets (shape_ok / ok_shape / edge_ok in csrc/): H * T * channels < 2^31.
    Longer one-shot inputs take the fp32 planar path like every other unsupported shape instead of raising TT_E_BADARG."""
    return x.size(2) * x.size(3) * (channels or x.size(1)) < 2 ** 31


def _f32ok(w):
    return w.dtype == torch.float32 and w.is_contiguous()


def to_cl16(x):
    if is_cl16(x):
        return x
    if not _cl16_ok(x.size(1), x.size(3)):
        raise ValueError('no bf16 channels-last form for %d channels x %d frames' % (x.size(1), x.size(3)))
    return ToCL16Fn.apply(x)


def to_planar32(x):
    """What every fp32-only layer calls on its input: identity for fp32 tensors."""
    if is_cl16(x):
        return ToPlanar32Fn.apply(x)
    if is_x3(x):
        return from_x3(x)
    return x


def gate_tap(y, link):
    """The copy of a 16-bit layer's output that leaves the module (see GateTapFn); y itself when there is nothing to do."""
    if not torch.is_grad_enabled() or not y.requires_grad or not is_cl16(y) or y.numel() % 8:
        return y
    if (link is None or not link.producer) and loss_scale(y.dtype) == 1.0:
        return y
    return GateTapFn.apply(y, link)


def _edge16_ok(x, b):
    """What the 3x3 edge kernels ask on either side: a bias, an even number of frames, 32-bit offsets within one clip of 4 channels."""
    return b is not None and x.dim() == 4 and x.size(3) % 2 == 0 and FUSED_RESBLOCK and x.size(2) * x.size(3) * 4 < 2 ** 31


def conv(x, w, b, cfg, link=None):
    same3 = cfg.kind == 'conv' and (cfg.KH, cfg.KW, cfg.stride, cfg.dil, cfg.pad_h, cfg.pad_w) == (3, 3, 1, 1, 1, 1) and _edge16_ok(x, b)
    if same3 and cfg.act == ACT_ELU and w.shape == (4, 2, 3, 3) and not is_cl16(x) and cl16_mode():
        return ConvIn16Fn.apply(x, w, b, link)                   # Encoder.convin feeding the bf16 channels-last interior
    if same3 and cfg.act == ACT_NONE and w.shape == (2, 4, 3, 3) and is_cl16(x):
        return ConvOut16Fn.apply(x, w, b)                        # Decoder.convout leaving it
    # the one-channel edges of the magnitude variants (TimbreTrapMag / TimbreTrapMagDB)
    if same3 and cfg.act == ACT_ELU and w.shape == (4, 1, 3, 3) and not is_cl16(x) and cl16_mode():
        return ConvIn16x1Fn.apply(x, w, b, link)
    if same3 and cfg.act in (ACT_NONE, ACT_RELU, ACT_SIGMOID) and w.shape == (1, 4, 3, 3) and is_cl16(x):
        return ConvOut16x1Fn.apply(x, w, b, cfg.act)
    x = to_planar32(x)
    return ConvFn.apply(x, w, b, cfg)


def conv_out_pair(x, w, b, act=ACT_NONE):
    """Conv2d(4, 2, 3, padding 'same') on a batch of two halves -> (first half, second half) (ConvOut16PairFn; else conv + slices).
    ``act``: the output nonlinearity of the magnitude variants (ACT_RELU / ACT_SIGMOID), fused into tt_conv2d's epilogue."""
    pairable = x.dim() == 4 and x.size(0) % 2 == 0 and is_cl16(x) and _edge16_ok(x, b)
    if pairable and act == ACT_NONE and w.shape == (2, 4, 3, 3):
        return ConvOut16PairFn.apply(x, w, b)
    if pairable and w.shape == (1, 4, 3, 3):
        return ConvOut16x1PairFn.apply(x, w, b, act)             # the magnitude variants' convout, nonlinearity in the epilogue
    y = conv(x, w, b, ConvCfg(3, 3, 1, 1, 1, 1, 'conv', 0, act))
    h = y.size(0) // 2
    return y[:h], y[h:]


def _wide16_ok(C, T):
    """A width the level / strided kernels of the 16-bit path take (C = 4 packs two frames per lane)."""
    return FUSED_RESBLOCK and C in WIDE_CHANNELS and (C != 4 or T % 2 == 0)


def _stride16_ok(C, T, w, b):
    return _wide16_ok(C, T) and w.shape == (2 * C, C, 4, 1) and b is not None


def strided_conv(x, w, b, win, hop, out_x3=False, link=None):
    """Conv2d(C, Cout, (win,1), stride (hop,1)) + ELU.  x may be an x3 tensor (is_x3); out_x3: the next layer takes one."""
    if is_x3(x):
        C = x.size(4)
        if (win == 4 and hop == 2 and x.size(1) >= 4 and C in X3_CHANNELS and w.shape == (2 * C, C, 4, 1) and b is not None
                and _x3_size_ok(x.size(0), x.size(1), x.size(2))):
            return x3_strided_conv(x, w, b, out_x3)
        x = from_x3(x)
    C = x.size(1)
    if (win == 4 and hop == 2 and x.size(2) >= 4 and _stride16_ok(C, x.size(-1), w, b) and (is_cl16(x) or cl16_mode())
            and _i32_ok(x, 2 * C)):
        return SConv16Fn.apply(to_cl16(x), w, b, link)
    x = to_planar32(x)
    if (out_x3 and x3_chain() and C == 8 and 2 * C in X3_CHANNELS and win == 4 and hop == 2 and x.size(2) >= 4 and x.is_cuda
            and w.shape == (2 * C, C, 4, 1) and b is not None and _x3_size_ok(x.size(0), x.size(2), x.size(3))):
        return x3_strided_conv(x, w, b, True)                    # the layer that enters the split-operand part of the encoder
    if FUSED_RESBLOCK and win == 4 and hop == 2 and C in FUSED_CHANNELS and w.shape == (2 * C, C, 4, 1) and b is not None:
        return StridedConvFn.apply(x, w, b)
    return conv(x, w, b, ConvCfg(win, 1, hop, 1, 0, 0, 'conv', 0, ACT_ELU))


def transposed_conv(x, w, b, win, hop, out_pad, out_x3=False, link=None, uplink=None):
    """ConvTranspose2d(Cin, C, (win,1), stride (hop,1), output_padding (out_pad,0)) + ELU.  x may be an x3 tensor."""
    C = w.size(1)
    if is_x3(x):
        if (win == 4 and hop == 2 and C in (16, 32) and x.size(4) == 2 * C and w.shape == (2 * C, C, 4, 1) and b is not None
                and out_pad in (0, 1) and _x3_size_ok(x.size(0), 2 * x.size(1) + 3, x.size(2))):
            return x3_transposed_conv(x, w, b, out_pad, out_x3)
        x = from_x3(x)
    if (win == 4 and hop == 2 and x.size(1) == 2 * C and out_pad in (0, 1) and _stride16_ok(C, x.size(-1), w, b)
            and (is_cl16(x) or cl16_mode()) and (2 * x.size(2) + 2 + out_pad) * x.size(3) * 2 * C < 2 ** 31):
        return TConv16Fn.apply(to_cl16(x), w, b, out_pad, link, uplink if is_cl16(x) else None)
    x = to_planar32(x)
    if (out_x3 and x3_chain() and C == 32 and x.size(1) == 64 and win == 4 and hop == 2 and x.is_cuda and w.shape == (64, 32, 4, 1)
            and b is not None and out_pad in (0, 1) and _x3_size_ok(x.size(0), 2 * x.size(2) + 3, x.size(3))):
        return x3_transposed_conv(x, w, b, out_pad, True)        # the layer that enters the split-operand part of the decoder
    if (FUSED_RESBLOCK and win == 4 and hop == 2 and C in FUSED_CHANNELS and w.shape == (2 * C, C, 4, 1)
            and x.size(1) == 2 * C and b is not None and out_pad in (0, 1)):
        return TransposedConvFn.apply(x, w, b, out_pad)
    return conv(x, w, b, ConvCfg(win, 1, hop, 1, 0, 0, 'tconv', out_pad, ACT_ELU))


def residual_block(x, w1, b1, w2, b2, dilation):
    x = to_planar32(x)
    C = x.size(1)
    if (FUSED_RESBLOCK and C in FUSED_CHANNELS and w1.shape == (C, C, 3, 3) and w2.shape == (C, C, 1, 1)
            and 1 <= dilation <= 3):
        return ResBlockFn.apply(x, w1, b1, w2, b2, dilation)
    k = w1.size(-1)
    h = conv(x, w1, b1, ConvCfg(k, k, 1, dilation, dilation * (k - 1) // 2, dilation * (k - 1) // 2, 'conv', 0, ACT_ELU))
    h = conv(h, w2, b2, ConvCfg(1, 1, 1, 1, 0, 0, 'conv', 0, ACT_ELU))
    return AddFn.apply(h, x)


def _join16_ok(y, e, w):
    """The tensors of a weighted skip join y + w[idx] * e that the one-pass 16-bit join kernels take (the batch ratio is the caller's)."""
    return (is_cl16(y) and is_cl16(e) and y.dtype == e.dtype and e.numel() % 8 == 0 and w.dtype == torch.float32 and w.is_contiguous()
            and y.shape[1:] == e.shape[1:])


def skip_join(y, skip):
    """y + skip for the decoder's joins: ``skip`` is a tensor (already scaled: apply_skip_connections) or a SkipJoin."""
    if not isinstance(skip, SkipJoin):
        return add(y, skip)
    e, w = skip.e, skip.weights
    if _join16_ok(y, e, w) and y.size(0) in (e.size(0), 2 * e.size(0)):
        return SkipJoin16Fn.apply(y, e, w, skip.idx, skip.link, skip.defer)
    # any other layout: the two-step form on whatever the tensors are (the tap carries the gate of a linked embedding)
    scaled = scale(gate_tap(e, skip.link), w, skip.idx)
    if y.size(0) == 2 * e.size(0):
        scaled = torch.cat((scaled, scaled), dim=0)
    return add(y, scaled)


def add(a, b):
    """a + b for the skip joins: on cl16 tensors when either side is one (Add16Fn), AddFn otherwise."""
    if is_cl16(a) or is_cl16(b):
        return Add16Fn.apply(to_cl16(a), to_cl16(b))
    return AddFn.apply(a, b)


def scale(e, weights, i):
    """weights[i] * e (TimbreTrap.apply_skip_connections)."""
    if is_cl16(e):
        return Scale16Fn.apply(e, weights, i)
    return ScaleFn.apply(e, weights, i)


def _level16_ok(x, blocks):
    """The level runs on cl16 tensors (Level16Fn / Level16JoinFn)."""
    C, T = x.size(1), x.size(-1)
    return (cl16_mode() and _wide16_ok(C, T) and _i32_ok(x)
            and all(b.conv1[0].weight.shape == (C, C, 3, 3) and 1 <= b.dilation <= 3 for b in blocks))


def _level16_args(blocks):
    """(dilations, [w1, b1, w2, b2 of every block]) as Level16Fn / Level16JoinFn take them."""
    params = []
    for b in blocks:
        params += [b.conv1[0].weight, b.conv1[0].bias, b.conv2[0].weight, b.conv2[0].bias]
    return tuple(b.dilation for b in blocks), params


def residual_level(x, blocks, out_x3=False, link=None, join=None):
    """
    block3(block2(block1(x))) for the ResidualConv2dBlock modules ``blocks``.  With ops.cl16_mode() the level runs
    on cl16 tensors (Level16Fn) and RETURNS a cl16 tensor -- the next layer either has a bf16 kernel or converts with
    to_planar32; otherwise the per-block fp32 path.  ``out_x3``: the caller's next layer takes a split-operand tensor (is_x3):
    honoured only where the level itself runs on them (x3_inference()).  ``join`` (a SkipJoin): the result + the weighted skip -- in the
    epilogue of the level's last block where the level runs on cl16 tensors (Level16JoinFn), else skip_join() behind it.
    """
    if join is not None:
        e = join.e
        if (SKIP_FOLD and _level16_ok(x, blocks) and _join16_ok(x, e, join.weights) and x.size(0) % e.size(0) == 0
                and x.size(0) // e.size(0) in (1, 2)):
            dilations, params = _level16_args(blocks)
            return Level16JoinFn.apply(x, dilations, link, e, join.weights, join.idx, join.link, join.defer, *params)
        return skip_join(residual_level(x, blocks, False, link), join)
    if is_x3(x):
        return x3_level(x, blocks, out_x3)
    C = x.size(1)
    if _level16_ok(x, blocks):
        dilations, params = _level16_args(blocks)
        # link: only when x is the producing layer's own output tensor (to_cl16 is the identity on it)
        return Level16Fn.apply(to_cl16(x), dilations, link if is_cl16(x) else None, *params)
    x = to_planar32(x)
    if (x3_inference() and X3N_INFER and C in X3N_CHANNELS and x.is_cuda and _x3_blocks_ok(C, blocks)
            and _x3_size_ok(x.size(0), x.size(2), x.size(3))):
        y = x3n_level(x, blocks)
        if x3_chain() or x3_vouched() or x3_range_ok(y):          # same range rule as the wide levels below
            return y
        with x3_disabled():
            return residual_level(x, blocks)
    if x3_inference() and C in X3_CHANNELS and x.is_cuda and _x3_blocks_ok(C, blocks):
        y = x3_level(x, blocks, out_x3)
        # outside TimbreTrap._inference (which checks its final result once) a level that went fp32 -> split -> fp32 vouches for
        # its own range: beyond +-65504 the split form is non-finite and the level is repeated on the fp32 kernels
        if x3_chain() or x3_vouched() or is_x3(y) or x3_range_ok(y):
            return y
        with x3_disabled():
            return residual_level(x, blocks)
    if x3_training(x, blocks):
        return x3_level_train(x, blocks)                         # opt-in (X3_TRAIN): split operands forward AND backward
    for b in blocks:
        x = b(x)
    return x


def _lat16_ok(CT, D, E, T, b):
    return b is not None and T % 16 == 0 and ((CT == 32 and D <= 48) or (CT == 64 and D <= 144))


def latent_encode(top, w, b, link=None):
    """Encoder.convlat (modules.py:446)."""
    if is_x3(top):
        if x3_latent_ok(top.size(4), w.size(0), w_enc=w) and w.size(2) == top.size(1):
            return x3_latent_encode(top, w, b)
        top = from_x3(top)
    if is_cl16(top) and _f32ok(w) and _lat16_ok(top.size(1), w.size(0), top.size(2), top.size(3), b) and w.shape[1:] == (top.size(1), top.size(2), 1):
        return LatEnc16Fn.apply(top, w, b, link)
    return LatentEncodeFn.apply(to_planar32(top), w, b)


def latent_decode(z, w, b, fill=None, out_x3=False, link=None):
    """
    Decoder.convin (modules.py:534) + ELU; cl16 output in the bf16 mode.  ``fill``: value of a constant last input channel that z
    does not carry (see LatDec16Fn); on the fp32 path the channel is concatenated like the reference does.  A PAIR of values
    (TimbreTrap.decode_pair): the output is two batches back to back, the first decoded with fill[0] and the second with fill[1] -- inside
    the 16-bit head (LatDec16Fn ``pair``); elsewhere the two batches are concatenated first.  ``out_x3`` (inside
    ops.x3_chain_scope): the next layer takes a split-operand tensor.
    """
    Dz = z.size(1) + (fill is not None)
    if isinstance(fill, (tuple, list)):
        if (cl16_mode() and FUSED_RESBLOCK and _f32ok(w) and z.dim() == 3 and z.is_cuda and w.size(0) == Dz and w.size(3) == 1
                and not (out_x3 and x3_chain()) and _lat16_ok(w.size(1), w.size(0), w.size(2), z.size(2), b)):
            return LatDec16Fn.apply(z, w, b, None, link, (float(fill[0]), float(fill[1])))
        z = torch.cat([torch.cat((z, torch.full_like(z[..., :1, :], float(v))), dim=-2) for v in fill], dim=0)
        fill = None
    if (out_x3 and x3_chain() and z.dim() == 3 and z.is_cuda and w.size(0) == Dz and x3_latent_ok(w.size(1), Dz - 1, w_dec=w)
            and w.size(2) * w.size(1) * 4 + 2 * ((Dz - 1) // 32) * (w.size(1) // 16) * 2048 <= 160 * 1024):
        return x3_latent_decode(z, w, b, fill, True)
    if (cl16_mode() and FUSED_RESBLOCK and _f32ok(w) and z.dim() == 3 and w.size(0) == Dz and w.size(3) == 1
            and _lat16_ok(w.size(1), w.size(0), w.size(2), z.size(2), b)):
        return LatDec16Fn.apply(z, w, b, fill, link)
    if fill is not None:
        z = torch.cat((z, torch.full_like(z[..., :1, :], float(fill))), dim=-2)
    return LatentDecodeFn.apply(z, w, b)
