"""
The 16-bit channels-last ("cl16") kernels called through the C ABI of include/ttrap.h in both element types (ops.lib16: bf16 and the fp16
_h twins), every element held to a derived rounding bound against the float64 restatements of tests/cl16_ref.py (pinned against torch
and proven on the CPU by tests/test_cl16_restatement.py).  The model is tests/test_gpu_conv_parity.py.

Families here: tt_wide_pack / _unpack; tt_gate16, tt_skip_join16_fwd / _bwd, tt_scaled_add16, tt_dot16; the eight edge convolutions
(csrc/conv_edge_bf16.hip); the nine latent-head entry points (csrc/latent_bf16.hip); the strided pair tt_sconv16_* / tt_tconv16_* with
the pregated forms and gate_dx (csrc/conv_stride_bf16.hip); the residual block: tt_wide_rb_fwd, _fwd_join, tt_wide_rb_bwd at every width,
tt_wide_rb_bwd_onepass and tt_wide_rb_bwd_fused (csrc/conv_wide_bf16.hip, conv_level_bf16.hip); the level calls tt_wide_level_bwd, _gated,
_gated_join; the refusals of all of these.
How the level calls are held.  tt_wide_level_bwd: every output bit-identical to nblocks calls of tt_wide_rb_bwd (the header's claim), each of
which this file holds to float64.  _gated / _gated_join: every gradient bit-identical to the plain call; dx against the PLAIN call's dx
(itself held through the block calls) times ELU'(x[0]), plus the join's share: the gated epilogue multiplies the fp32 sum v of which the
plain call shows the 16-bit rounding, |v - dx16| <= e |v|, so the bar is that distance through the gate plus the epilogue's own fp32
roundings -- a bound relative to the plain call, not a second float64 restatement of the whole level.

Arena (cl16_ref.Arena).  Every operand of a call -- cl16 tensors, fp32 weights / biases / gradients / planar images, scratch of exactly
the header's *_scratch_bytes -- is a window of ONE byte buffer, on a 16-byte boundary, 128 bytes of guard around it.  Kinds: in
(bit-unchanged afterwards), out (guard pattern before; every element written and finite afterwards), acc (a non-zero pattern before: the
+= contract), scratch.  Every case runs twice: guard byte 0xFF (NaN in bf16, fp16 and fp32) and 0x46 (12672 / 6.27 / 12689.6: what a
halo misread cannot hide from the median-form ELU of the residual block, which turns a NaN into 0).  A refused call must leave the
whole buffer untouched.

Operands.  16-bit operands uniform in +-[0.5, 1] rounded to the element type; weights +-[0.5, 1) with a 4-bit significand times a power
of two near 1 / sqrt(K): exact in both types, products with 16-bit operands exact in fp32; one dropped, doubled or mis-addressed product
moves a result by >= 0.25 / sqrt(K).  The saved output y that a backward gates with is a free operand of the same kind (the kernels
read it as data), which makes the gate dy * min(y + 1, 1) exact in fp32.

Bars (u = 2^-24; S, K from the restatement: sum of absolute products, number of products restricted to taps inside the image):
    fp32 accumulator or output   K u S + 3 u (|bias| + |previous content|)
    ELU                          + 4 u max(1, |v|): __expf(a) - 1 is within 2u of expm1(a) for a <= 0 (v_exp_f32 to 1 ulp of a value
                                 below 1, the product a log2(e) to u |a|); the median form returns that same e for 0 < a < 3e-4, where
                                 |e - a| <= 2u + a^2 / 2 < 2.8u: covered
    sigmoid                      + 4 u (as test_gpu_conv_parity.py)
    ELU' through the output      + u |dy| (the y + 1) + u |g| (the product); sigmoid' (dy (1 - y)) y: three roundings, 3 u (1 + u)^2 |g|
    the residual add, the join   + u |result| each (one fp32 add, one fma)
    stored 16-bit result         beta + max(e (|want| + beta), h): e the unit roundoff of the element type, h half the spacing of its
                                 subnormals (fp16: 2^-25, for results below 6.1e-5 -- a gate close to 0 times a cancelling sum -- where
                                 the spacing no longer shrinks with the value; bf16: 2^-134, never reached)
    stored intermediate          h1 of a forward with h1: held to its own bar, then the kernel's own tensor feeds the second stage
    rounded, exactly known       z of the latent heads; the gated operand of tt_latent16_contract / _wgrad and of the strided layers'
                                 backward: inputs, or exact in fp32 -- the restatement rounds the same value, no bar grows
    rounded, not observable      the hidden activation of a forward without h1 or of tt_wide_rb_bwd_fused (recomputed); dA2 everywhere;
                                 dA1 where it stays in LDS (C = 4, 8, 16, the fused form): the restatement rounds its own at the same
                                 place, and every bar downstream grows by |w| . boundary_spread -- per contributor 0 unless it lies
                                 within its own bar of a rounding boundary of the element type, then the distance of the two candidate
                                 roundings (one spacing; more only where the bar itself exceeds the spacing).  No cap, no statistical
                                 allowance.  dA1 of C = 32 is stored in ws: held to its bar, then the kernel's own tensor is used.
    the block backward           from the kernels: a2 = W2 h1 + b2, dA2 = dy min(exp(a2), 1) (1-Lipschitz in a2, __expf to 2u below 1), dA1 =
                                 (W2^T dA2) min(h1 + 1, 1); db2 sums the UNROUNDED dA2 in every kernel; db1 sums the unrounded dA1
                                 (k_nrb_bwd_fused, k_wrb_bwds, k_wrb_bwd_a) -- except tt_wide_rb_bwd_fused, which sums the rounded dA1 it
                                 reads back as the centre tap; dW2, dW1 and dx take the 16-bit roundings
The rounding term e.  The issue sets e = 2^-9 (bf16) / 2^-12 (fp16).  That is half the unit roundoff of the formats (8 and 11 significant
bits: round-to-nearest moves v by up to 2^-8 |v| / 2^-11 |v|, reached near the low end of every binade), so a correctly rounded store of
the EXACT value misses it on about a quarter of all elements -- tests/test_cl16_restatement.py::test_rounding_term shows torch's own
conversion at 0.99 x 2^-8.  This is the case the issue provides for ("a finding about the derivation ... re-derived from documented
arithmetic of the instruction"): v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32 round to nearest even, error <= 2^-p |v|, and the asserted bar
uses e = 2^-8 / 2^-11.  Every 16-bit check also prints its ratio to the bar with the issue's e ("issue-e"), so the figure is on record.

Every check prints its ratio to the bar (pytest -rP).

Read from the code (issue section 3).  Planes below H = 5 / T = 16:
    k_wide_pack / _unpack   one thread per 16-byte piece of the cl16 side, guard ``pix >= npix``; C = 4 pairs two pixels (T even keeps the
                            pair in one row, H T even in one clip); the planar side by 4-byte accesses: any plane, no access outside.
    k_gate_dx, k_skip_join_*, k_scaled_add16, k_dot16   flat loops over n / 8 pieces: nothing depends on a plane.
    conv_edge_bf16.hip      a border tile stages element by element, ``ok`` = inside the image, and a lane without an element reads offset 0
                            (StagePlanar VEC reads 16 bytes there: T % 4 == 0 gives the tensor >= 4 floats; StageCl4 8 bytes: >= one pixel);
                            the interior fast path needs h0 >= 1, h0 + 17 <= H, t0 >= 1 (4) and t0 + 65 (68) <= T, and its last staged
                            element is row h0 + 16, column t0 + 64 (67): inside; stores are masked by t < T && h < H; the partials are
                            blockIdx NPARTW + tid with tid < 76 <= NPARTW and grid <= EDGE_MAX_WG = the scratch size.  No access outside.
    latent_bf16.hip         T = 16 < 64: k_lat_wgrad's chunk of 64 pixels spans clips, handled by the ``T >= 64 ... else`` wrap, pixels
                            beyond B T by ``okp`` (the DMA then reads the zero piece, the gated form offset 0); k_lat_contract / _expand clamp
                            a dead lane's offset to 0 and guard the stores by ``ok``; E = 1: one or two K steps, the prefetch of step
                            s + 1 == nsteps is dead (offset 0).  D = 1 .. 48 / 144 only changes zero padding.  No access outside.
    conv_stride_bf16.hip    k_s4 / k_p2 / k_s4n / k_p2n: no LDS; every load goes through load_gated's ``ok`` (group index, t < T, input row in
                            [0, Hin)), prefetches of the group after the last included; stores by t < T and the output row < Hout.  k_w4:
                            stage_tile tests row and frame of every piece (DMA: the zero piece; the gated staging: offset 0, masked); at
                            C = 4 a piece is a pixel pair, whole because T is even; the data gradient riding on it reads LDS rows
                            2 r + kh <= 2 TR + 2 < BROWS (tconv) or the halo row above the tile, guarded by hi in [0, Hs) (sconv, whose last
                            tile also writes the rows past 2 Hs, zeros for the unused row of an odd H); the extra bias rows of the pregated
                            tconv are 2 nvalid .. BROWS - 1.  H = 4 (one output row), tconv H = 1, T = 2: no access outside.
    k_nrb_bwd_fused         (C = 4, 8 backward) border tiles stage piece by piece with ``ok`` = inside the image (zero piece otherwise; pixel pairs
                            at C = 4 whole because T is even), the fast path only for tiles whose whole halo is inside; phase 1 and 2b touch
                            LDS only; phase 2a reads LDS at (r + kh D) RW + DP + lane + (kw - 1) D < ROWS RW, the join's gradients at a frame
                            clamped to T - 1, and stores under t < T, h < H; dumps at blockIdx < MAX_W_WG <= MAX_A_WG.  No access outside.
    k_wrb_bwd_a, k_wrb_dxw  (C = 32 per stage) the chain is flat over B H T pixels under ``pix < npix``; the dxw tile stages dA1 (+ D halo) and x
                            under ``ok``, asks for dy (and the join's operands) at a frame clamped to T - 1 and a row inside the tile and the
                            image, computes only groups with t0 + 16 w < T and h < H, stores under ``valid``; LDS reads of dW1 stay inside
                            IR x IW.  No access outside.
    k_wrb_bwds              (the strips: C = 16, and C = 32 through tt_wide_rb_bwd_onepass) rows above / below the image and columns beside it
                            come from the zero piece (whole rows by a scalar test, edge strips piece by piece), the x rows under h < H and
                            t0 + px < T; step d. reads dy / x / the join at clamped frames and rows inside the image, stores under ``valid``;
                            ring slots are taken modulo RING for rows -D .. H - 1 + D.  No access outside.
    k_wrb_bwd_fused         x (+ 2 D halo) and dy (+ D halo) staged under ``ok``; h1 recomputed on the halo'd tile (outside the image dy = 0 makes
                            dA1 = 0 whatever ELU(b1) is); dy re-read at a clamped frame; stores under ``valid``, h < H.  No access outside.
    k_wrb_conv, k_nrb_conv  (the block forward) tile + halo staged piece by piece, ``ok`` = inside the image, else the zero piece; the
                            narrow kernel's column halo is rounded up to whole pieces (DP), pixel pairs at C = 4 whole because T is even;
                            LDS reads (r + kh D) RW + column + kw D stay below ROWS RW; the join's loads clamp row and frame to the image;
                            stores by t < T and h < H.  Planes down to (1, 2): no access outside.
Alignment, (entry point, pointer) by what the code issues; every refusal is TT_E_BADARG before anything is launched and is tested here:
    cl16 pointers           pack out / unpack in / gate16 g, y: 16-byte vector accesses -> 16 bytes (skip join, scaled add and dot already
                            tested it).  Edge convolutions: one pixel = 8 bytes at a time -> 8 bytes (ops/cl16.py hands them batch halves
                            of an odd plane: test_pair_wrapper_hands_the_halves_of_an_odd_plane_to_the_edge_convolutions).  Latent heads:
                            16-byte pieces everywhere, LDS-DMA on g of the weight gradient and on the operands prepared in ws -> every
                            cl16 pointer and ws 16 bytes.  Strided pair: LDS-DMA on the un-gated operand of k_w4 (both operands in the
                            pregated forms), 16-byte pieces elsewhere -> every cl16 pointer 16 bytes; ws holds fp32 partials, 4 bytes.
                            Residual block and level: LDS-DMA on x, h1, dy and the dA1 region of ws, 16-byte pieces for y, h1 (stored),
                            dx, skip, tmp0 / tmp1, skip_g -> all of them and ws 16 bytes (test_block_and_level_refusals; the level call
                            tests every block's x and h1 before its first launch).  ws at C = 4, 8, 16 holds fp32 partials only (4-byte
                            accesses): the 16 bytes are asked of it at every width so that the contract is one rule.
    fp32 pointers           x of pack, y of unpack, s / ds / out of the helpers, w / b / dw / db / dx / y of the edge convolutions,
                            z / w / bias / out / dw / db of the heads, w / b / dw / db of the strided pair, w1 / b1 / w2 / b2 / skip weights
                            of the block forward, w1 / b1 / w2 / b2 / dw1 / db1 / dw2 / db2 of the block backward (all three forms): 4-byte
                            accesses; one float off a 16-byte boundary meets the same bars.
                            x of tt_convin16[_1]_fwd / _bwd, dy and the saved y of tt_convout16[_1]_bwd: StagePlanar's float4 loads were
                            chosen on T % 4 == 0 alone -- the host condition now includes the pointers (edge_vec), a misaligned one takes
                            the 4-byte staging and meets the same bars.  ws of the edge convolutions and of the strided pair: 4-byte stores.
Bug fixed: tt_latent16_contract_pregated ran at D = 48 / 144, where the header promises TT_E_UNSUPPORTED and tt_latent16_pregated_ok says
0 (test_latent_pregated_agrees_with_ok).

Worst ratios measured on an MI355X (1350 cases, 26 s for the file; bf16 / fp16 where they differ):
    every stored 16-bit result    0.95 - 1.00 of the bar, as a half-ulp bar must be met by tens of thousands of correctly rounded
                                  elements: gate16 0.99, skip_join_fwd 1.00, skip_join_bwd de 1.00, scaled_add16 0.99, convin16[_1] fwd
                                  0.99 / 1.00, convout16[_1] bwd dx 0.99 / 1.00, latent expand 1.00 (+ ELU 1.00, gated 1.00), sconv16 fwd
                                  0.99, bwd dx 1.00, tconv16 fwd 1.00 / 0.99, bwd dx 0.99, gated dx 0.99 / 0.96; rb_fwd h1 0.99 / 0.98
                                  (C = 4, 8, 16), 0.99 / 0.96 (C = 32), y 1.00 / 0.99, y with h1 NULL 0.99 - 1.00 (C = 32 fp16 0.96);
                                  rb_fwd_join the same.  With the issue's e the same checks stand at 1.89 - 2.00, and where a result is
                                  subnormal at 2.8 (tconv16 gated dx fp16), 5.0 (latent expand gated fp16) and 82.8 (skip_join_bwd de fp16)
    pack / unpack                 exact
    tt_dot16                      < 0.001          skip_join_bwd ds 0.04
    convin16 bwd                  dw 0.25 / 0.50, db 0.04, dx 0.03 / 0.14        convin16_1 bwd    dw 0.49 / 0.17, db 0.35, dx 0.02 / 0.05
    convout16 fwd                 0.05             convout16 bwd dw 0.32 / 0.25, db 0.09
    convout16_1 fwd               0.07 / 0.10      convout16_1 bwd dw 0.22 / 0.21, db 0.02 / 0.20
    latent contract               0.015 (pregated < 0.001)
    latent wgrad                  dw 0.05 / 0.08; gated dw 0.06 / 0.11, db 0.02 / 0.04; pregated dw 0.05 / 0.11, db 0.02
    sconv16 bwd                   dw 0.28 / 0.42, db 0.24; pregated dw 0.25 / 0.26, db 0.16
    tconv16 bwd                   dw 0.30 / 0.46, db 0.02 / 0.05; pregated dw 0.26 / 0.25, db 0.03
    rb_bwd (C 4 / 8 / 16 / 32)    dx 0.99 - 1.00 (dA1 of C = 32 0.99); dw1 0.35 / 0.39 / 0.46 / 0.61, dw2 0.24 / 0.27 / 0.28 / 0.38, db1 0.11 / 0.06 /
                                  0.06 / 0.01, db2 0.09 / 0.04 / 0.03 / 0.01; rb_bwd_onepass (C 16, 32): dx bit-identical to tt_wide_rb_bwd, the
                                  gradients at the same ratios
    rb_bwd_fused (C 16 / 32)      dx 0.99 / 0.98, dw1 0.38 / 0.41, dw2 0.30 / 0.31, db1 0.20 / 0.15, db2 0.02 / 0.01
    level                         tt_wide_level_bwd bit-identical to block by block in every case; gated dx 0.85 - 0.97, gated_join dx 0.92 - 0.99,
                                  skip_dw <= 0.001; issue-e ratios of these families up to 2.0, 56 where a gated dx is subnormal in fp16
    one pointer misaligned        every (entry point, fp32 pointer) pair and the cl16 tensors of the edge convolutions 8 bytes off met the
                                  same bars; every cl16 pointer off its requirement was refused with the buffer untouched
(The weight- and bias-gradient bars grow with K = the pixels summed, so on the larger planes they catch a lost tile or lost previous
content; the smallest planes, where K is 1 to 32, are the ones that catch a single product.)

Broken on purpose in scratch copies of the sources, ONE library per break, nothing moved outside an operand's window; each library ran
this file (refusal tests left out) and the stage-wise tests of tests/test_gpu_wide_bf16.py (test_wide_block_stagewise, test_sconv16_ /
test_tconv16_stagewise, test_latent_heads_stagewise, test_edge_convs, test_skip_joins_on_the_device, test_fused_skip_joins_stagewise,
test_strided_latent_edge_capped_grids):
    edge, halo column        the right halo column of a border tile of the 4-byte planar staging read one column inward: 68 cases here --
                             every case whose planar operand takes that staging: T % 4 != 0 (test_edge_convolutions[*-1-1], [*-2-3],
                             [*-17-65] of all six layers, less the relu case at (2, 3); the (35, 131) capped grids) and x one float off
                             (test_edge_one_fp32_pointer_misaligned[*-in*]).  Stage-wise: test_edge_convs 2 of 5.
    edge, tap dropped        tap (ci 3, k 8) of the two-channel convout forward: 18 cases here -- test_edge_convolutions[*-out-H-T] at
                             every plane with a bottom-right neighbour, both capped grids, test_edge_one_fp32_pointer_misaligned[*-out-*].
                             Stage-wise: test_edge_convs 5 of 5, test_strided_latent_edge_capped_grids 2 of 2.
    latent, += -> store      k_lat_wred's ``dw +=``: 22 cases here (all 20 test_latent_heads, test_latent_one_fp32_pointer_misaligned).
                             Stage-wise: NOT noticed (118 of 118 passed: those tests accumulate onto zeros).
    helpers, gate skipped    lane 5, element 3 of k_skip_join_bwd: test_flat_helpers at n = 8 * 37 and 8 * 4099 (the lengths that reach lane 5),
                             both element types.  Stage-wise: test_fused_skip_joins_stagewise 6 of 6 with the gate on.
    pack, channels swapped   channels j and j ^ 1 of pixel 4: test_pack_unpack, every case with more than four pixels (100 of 110).
                             Stage-wise: 103 failures (every test that packs its operands).
    strided, gate skipped    thread 5, element 3 of k_w4's gated staging: 260 cases here (test_sconv16 110, test_tconv16 144, misaligned 6).
                             Stage-wise: test_sconv16_stagewise 15 of 16, test_tconv16_stagewise 16 of 16.
    block forward, tap       product (tap 8, ob 0, kb 0) of k_nrb_conv: 122 cases here (108 of the 132 C = 4, 8 cases of test_residual_block_forward -- those
                             with a bottom-right neighbour inside the image -- the multi-tile and misaligned cases).  Stage-wise:
                             test_wide_block_stagewise 30 of 60.
    block backward, gate     the ELU' of dA1 skipped on lane 5, element 3 of k_wrb_bwd_a (C = 32): 64 cases here -- test_residual_block_backward
                             [*-32-*] (56), its multi-tile (6) and misaligned (2) cases.  test_level_backward does NOT fail: it compares the
                             level call with block-by-block calls of the same library, which is all its equality claims; the values are
                             held by the block cases.  Stage-wise: test_wide_block_stagewise 15 of 60, test_wide_block_multitile 2.
    level, gate              the gated epilogue of k_nrb_bwd_fused (C = 4, 8) skipping ELU'(x) on lane 5, channel 3: the 24 test_level_backward
                             cases of C = 4, 8 whose first dilation is 1.  Stage-wise:
                             test_level_hands_the_layer_in_front_its_gradient_already_gated 3 of 14.
"""

import ctypes
import functools
import zlib

import pytest
import torch

import cl16_ref as C

pytestmark = pytest.mark.gpu

U = C.U
BADARG, UNSUPPORTED = -1, -2
BF16, FP16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [BF16, FP16]
FILLS = [C.FILL_NAN, C.FILL_BIG]
ISSUE_E = {BF16: 2.0 ** -9, FP16: 2.0 ** -12}


def _tag(dtype):
    return 'bf16' if dtype == BF16 else 'fp16'


def _api(dtype):
    from timbre_trap import _hip
    from timbre_trap.framework import ops
    return ops.lib16(dtype), _hip.stream_ptr()


_worst = {}


def _note(key, ratio):
    _worst[key] = max(_worst.get(key, 0.0), ratio)
    print('ratio to bar: %-44s %.3f (worst so far %.3f)' % (key, ratio, _worst[key]))


def _hold(key, got, want, bar, what=''):
    e = (got.double() - want).abs()
    r = (e / bar.clamp_min(1e-300)).reshape(-1)
    ratio = float(r.max()) if e.numel() else 0.0
    _note(key, ratio)
    if not bool((e <= bar).all()):
        i = int(r.argmax())
        raise AssertionError('%s %s: %.3f of the bar at element %d (wanted %.9g, off by %.3e; %d of %d elements over)' % (
            key, what, ratio, i, float((want + torch.zeros_like(e)).reshape(-1)[i]), float(e.reshape(-1)[i]), int((e > bar).sum()), e.numel()))


def _hold16(key, got, want, beta, dtype, what=''):
    """A stored 16-bit result: beta + e (|want| + beta) with e the unit roundoff; the ratio to the same bar with the issue's e is printed."""
    e = (got.double() - want).abs()
    issue = beta + ISSUE_E[dtype] * (want.abs() + beta)
    _note(key + ' issue-e', float((e / issue.clamp_min(1e-300)).max()) if e.numel() else 0.0)
    _hold(key, got, want, C.bar16(want, beta, dtype), what)


def _gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


@pytest.fixture
def cu_limit():
    """Cap the CU count the persistent grids are sized with; restored afterwards."""
    lib, _ = _api(BF16)
    prev = lib.tt_set_cu_limit(0)
    yield lib.tt_set_cu_limit
    lib.tt_set_cu_limit(prev)


def _arena(fill):
    return C.Arena(fill, 'cuda')


def _finish(A, rc, what):
    """0 after a verified call; the status of a refused one, with the buffer proven untouched."""
    if rc != 0:
        A.untouched(what + ' (refused with %d)' % rc)
        return rc
    A.verify(what)
    return 0


PLANES = [(1, 2), (2, 4), (3, 6),                  # smaller than any halo or tile
          (4, 32), (8, 64), (16, 64),              # exact tiles
          (5, 34), (9, 66), (17, 66),              # one past
          (7, 62), (15, 30)]                       # one short


# ---- 1. pack and unpack -----------------------------------------------------------------------------------------------------------
def _pack(dtype, fill, Cc, B, H, T, shift=0, cl_shift=0):
    lib, st = _api(dtype)
    x = C.pm32(_gen('pack', Cc, H, T), B, Cc, H, T)
    A = _arena(fill)
    A.inp('x', x, shift)
    A.out('out', (B, H, T, Cc), dtype, cl_shift)
    A.build()
    what = 'tt_wide_pack %s C %d plane (%d, %d)' % (_tag(dtype), Cc, H, T)
    rc = _finish(A, lib.tt_wide_pack(A.ptr('x'), A.ptr('out'), B, Cc, H, T, st), what)
    if rc == 0:
        assert torch.equal(A.get('out'), x.permute(0, 2, 3, 1).contiguous().to(dtype)), what
    return rc


def _unpack(dtype, fill, Cc, B, H, T, shift=0, cl_shift=0):
    lib, st = _api(dtype)
    v = C.pm16(_gen('unpack', Cc, H, T), dtype, B, H, T, Cc)
    A = _arena(fill)
    A.inp('in', v, cl_shift)
    A.out('y', (B, Cc, H, T), F32, shift)
    A.build()
    what = 'tt_wide_unpack %s C %d plane (%d, %d)' % (_tag(dtype), Cc, H, T)
    rc = _finish(A, lib.tt_wide_unpack(A.ptr('in'), A.ptr('y'), B, Cc, H, T, st), what)
    if rc == 0:
        assert torch.equal(A.get('y'), v.float().permute(0, 3, 1, 2).contiguous()), what
    return rc


@pytest.mark.parametrize('H,T', PLANES)
@pytest.mark.parametrize('Cc', [4, 8, 16, 32, 64])
@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_pack_unpack(dtype, Cc, H, T, B=2):
    """Exact equality: the rounding of pack is the element type's round-to-nearest-even of an fp32 input, unpack is exact."""
    for fill in FILLS:
        assert _pack(dtype, fill, Cc, B, H, T) == 0
        assert _unpack(dtype, fill, Cc, B, H, T) == 0
    assert _pack(dtype, C.FILL_NAN, Cc, B, H, T, shift=4) == 0           # the planar side one float off a 16-byte boundary
    assert _unpack(dtype, C.FILL_NAN, Cc, B, H, T, shift=4) == 0


@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_pack_unpack_refusals(dtype):
    lib, st = _api(dtype)
    assert _pack(dtype, C.FILL_BIG, 4, 1, 3, 5) == BADARG                # T odd at C = 4
    assert _unpack(dtype, C.FILL_BIG, 4, 1, 3, 5) == BADARG
    assert _pack(dtype, C.FILL_BIG, 12, 1, 3, 6) == BADARG               # a width that is not compiled
    for off in (2, 8):                                                   # the cl16 side off its 16-byte boundary
        assert _pack(dtype, C.FILL_BIG, 8, 1, 3, 6, cl_shift=off) == BADARG
        assert _unpack(dtype, C.FILL_BIG, 8, 1, 3, 6, cl_shift=off) == BADARG


# ---- 2. the flat helpers ----------------------------------------------------------------------------------------------------------
NS = [8, 16, 8 * 37, 8 * 4099]


def _gate16(dtype, fill, n, shifts=None):
    lib, st = _api(dtype)
    shifts = shifts or {}
    gen = _gen('gate', n)
    g, y = C.pm16(gen, dtype, n), C.pm16(gen, dtype, n)
    A = _arena(fill)
    A.acc('g', g, shifts.get('g', 0))
    A.inp('y', y, shifts.get('y', 0))
    A.build()
    what = 'tt_gate16 %s n %d' % (_tag(dtype), n)
    rc = _finish(A, lib.tt_gate16(A.ptr('g'), A.ptr('y'), n, st), what)
    if rc == 0:
        v, S, _ = C.gate16(g.double(), y.double())
        _hold16('gate16 %s' % _tag(dtype), A.get('g'), v, 2 * U * S, dtype, what)         # the y + 1 and the product
    return rc


def _skip_fwd(dtype, fill, n, reps, with_s, shifts=None):
    lib, st = _api(dtype)
    shifts = shifts or {}
    gen = _gen('sjf', n, reps)
    y, e, s = C.pm16(gen, dtype, reps, n), C.pm16(gen, dtype, n), C.pm32(gen, 3)
    A = _arena(fill)
    A.inp('y', y, shifts.get('y', 0))
    A.inp('e', e, shifts.get('e', 0))
    if with_s:
        A.inp('s', s, shifts.get('s', 0))
    A.out('out', (reps, n), dtype, shifts.get('out', 0))
    A.build()
    what = 'tt_skip_join16_fwd %s n %d reps %d%s' % (_tag(dtype), n, reps, '' if with_s else ' s NULL')
    rc = _finish(A, lib.tt_skip_join16_fwd(A.ptr('y'), A.ptr('e'), A.ptr('s'), 1, A.ptr('out'), n, reps, st), what)
    if rc == 0:
        v, S, _ = C.skip_join_fwd(y.double(), e.double(), float(s[1]) if with_s else 1.0, reps)
        _hold16('skip_join_fwd %s' % _tag(dtype), A.get('out'), v, U * S, dtype, what)
    return rc


def _skip_bwd(dtype, fill, n, reps, gate, with_s=True, with_de=True, with_ds=True, shifts=None):
    lib, st = _api(dtype)
    shifts = shifts or {}
    gen = _gen('sjb', n, reps, gate)
    g, e, s = C.pm16(gen, dtype, reps, n), C.pm16(gen, dtype, n), C.pm32(gen, 3)
    prev_de, prev_ds = C.pm16(gen, dtype, n), C.pm32(gen, 3)
    A = _arena(fill)
    A.inp('g', g, shifts.get('g', 0))
    A.inp('e', e, shifts.get('e', 0))
    if with_s:
        A.inp('s', s, shifts.get('s', 0))
    if with_de:
        if gate & 2:
            A.acc('de', prev_de, shifts.get('de', 0))
        else:
            A.out('de', (n,), dtype, shifts.get('de', 0))
    if with_ds:
        A.acc('ds', prev_ds, shifts.get('ds', 0))
    A.build()
    what = 'tt_skip_join16_bwd %s n %d reps %d gate %d%s%s%s' % (_tag(dtype), n, reps, gate, '' if with_s else ' s NULL',
                                                            '' if with_de else ' de NULL', '' if with_ds else ' ds NULL')
    rc = _finish(A, lib.tt_skip_join16_bwd(A.ptr('g'), A.ptr('e'), A.ptr('s'), 1, A.ptr('de'), A.ptr('ds'), n, reps, gate, st), what)
    if rc == 0:
        de, rS, ds, Sd, Kd = C.skip_join_bwd(g.double(), e.double(), float(s[1]) if with_s else 1.0, gate, prev_de.double())
        if with_de:
            _hold16('skip_join_bwd de %s' % _tag(dtype), A.get('de'), de, U * rS, dtype, what)
        if with_ds:
            want, bar = prev_ds.double().clone(), torch.zeros(3, dtype=torch.float64)     # the other two weights: not one bit
            want[1] += ds
            bar[1] = Kd * U * Sd + 3 * U * abs(float(prev_ds[1]))
            _hold('skip_join_bwd ds %s' % _tag(dtype), A.get('ds'), want, bar, what)
    return rc


def _scaled_add(dtype, fill, n, with_a, with_s, shifts=None):
    lib, st = _api(dtype)
    shifts = shifts or {}
    gen = _gen('sadd', n)
    a, b, s = C.pm16(gen, dtype, n), C.pm16(gen, dtype, n), C.pm32(gen, 3)
    A = _arena(fill)
    if with_a:
        A.inp('a', a, shifts.get('a', 0))
    A.inp('b', b, shifts.get('b', 0))
    if with_s:
        A.inp('s', s, shifts.get('s', 0))
    A.out('y', (n,), dtype, shifts.get('y', 0))
    A.build()
    what = 'tt_scaled_add16 %s n %d%s%s' % (_tag(dtype), n, '' if with_a else ' a NULL', '' if with_s else ' s NULL')
    rc = _finish(A, lib.tt_scaled_add16(A.ptr('a'), A.ptr('b'), A.ptr('s'), 2, A.ptr('y'), n, st), what)
    if rc == 0:
        v, S, _ = C.scaled_add(a.double() if with_a else None, b.double(), float(s[2]) if with_s else 1.0)
        _hold16('scaled_add16 %s' % _tag(dtype), A.get('y'), v, U * S, dtype, what)
    return rc


def _dot(dtype, fill, n, shifts=None):
    lib, st = _api(dtype)
    shifts = shifts or {}
    gen = _gen('dot', n)
    a, b, prev = C.pm16(gen, dtype, n), C.pm16(gen, dtype, n), C.pm32(gen, 1)
    A = _arena(fill)
    A.inp('a', a, shifts.get('a', 0))
    A.inp('b', b, shifts.get('b', 0))
    A.acc('out', prev, shifts.get('out', 0))
    A.build()
    what = 'tt_dot16 %s n %d' % (_tag(dtype), n)
    rc = _finish(A, lib.tt_dot16(A.ptr('a'), A.ptr('b'), A.ptr('out'), n, st), what)
    if rc == 0:
        v, S, K = C.dot(a.double(), b.double())
        _hold('dot16 %s' % _tag(dtype), A.get('out'), prev.double() + v, (K * U * S + 3 * U * prev.double().abs()).view(1), what)
    return rc


@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_flat_helpers(dtype, n):
    """tt_gate16, tt_skip_join16_fwd / _bwd (gate 0..3, reps 1 and 2; s, de, ds NULL in turn), tt_scaled_add16, tt_dot16; n from one 16-byte
    piece to more pieces than one grid-stride pass of one workgroup."""
    for fill in FILLS:
        assert _gate16(dtype, fill, n) == 0
        for reps in (1, 2):
            assert _skip_fwd(dtype, fill, n, reps, True) == 0
            for gate in range(4):
                assert _skip_bwd(dtype, fill, n, reps, gate) == 0
        assert _skip_fwd(dtype, fill, n, 2, False) == 0
        assert _skip_bwd(dtype, fill, n, 2, 1, with_s=False) == 0
        assert _skip_bwd(dtype, fill, n, 1, 1, with_de=False) == 0
        assert _skip_bwd(dtype, fill, n, 2, 3, with_ds=False) == 0
        assert _scaled_add(dtype, fill, n, True, True) == 0
        assert _scaled_add(dtype, fill, n, False, False) == 0
        assert _dot(dtype, fill, n) == 0
    # the fp32 operands one float off a 16-byte boundary: 4-byte accesses, the same bars
    assert _skip_fwd(dtype, C.FILL_NAN, n, 2, True, {'s': 4}) == 0
    assert _skip_bwd(dtype, C.FILL_NAN, n, 2, 3, shifts={'s': 4}) == 0
    assert _skip_bwd(dtype, C.FILL_NAN, n, 2, 3, shifts={'ds': 4}) == 0
    assert _scaled_add(dtype, C.FILL_NAN, n, True, True, {'s': 4}) == 0
    assert _dot(dtype, C.FILL_NAN, n, {'out': 4}) == 0


@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_flat_helper_refusals(dtype):
    """n % 8 (gate and skip join; tt_scaled_add16 and tt_dot16 take any n: their tails are run), a skip-join backward with nothing to write or
    += without de, and every 16-bit pointer in turn off its 16-byte boundary: TT_E_BADARG, the buffer untouched."""
    big = C.FILL_BIG
    assert _gate16(dtype, big, 12) == BADARG
    assert _skip_fwd(dtype, big, 12, 1, True) == BADARG
    assert _skip_bwd(dtype, big, 12, 1, 0) == BADARG
    assert _skip_fwd(dtype, big, 16, 3, True) == BADARG
    assert _skip_bwd(dtype, big, 16, 1, 0, with_de=False, with_ds=False) == BADARG
    assert _skip_bwd(dtype, big, 16, 1, 2, with_de=False) == BADARG
    assert _scaled_add(dtype, big, 13, True, True) == 0 and _dot(dtype, big, 13) == 0
    for p in ('g', 'y'):
        assert _gate16(dtype, big, 16, {p: 8}) == BADARG
    for p in ('y', 'e', 'out'):
        assert _skip_fwd(dtype, big, 16, 2, True, {p: 8}) == BADARG
    for p in ('g', 'e', 'de'):
        assert _skip_bwd(dtype, big, 16, 2, 3, shifts={p: 8}) == BADARG
    for p in ('a', 'b', 'y'):
        assert _scaled_add(dtype, big, 16, True, True, {p: 8}) == BADARG
    for p in ('a', 'b'):
        assert _dot(dtype, big, 16, {p: 2}) == BADARG


# ---- 3. the edge convolutions -----------------------------------------------------------------------------------------------------
EDGE_PLANES = [(1, 1), (1, 4), (2, 3), (3, 4), (16, 64), (17, 65), (17, 68)]


@functools.lru_cache(maxsize=4)
def _edge_setup(kind, NP, act, dtype, B, H, T):
    """Operands of one edge layer and its float64 forward, shared (unchanged) by the forward and backward checks.  kind 'in': fp32 planar
    (B, NP, H, T) -> cl16 (B, 4, H, T) with ELU; 'out': cl16 -> fp32 planar (B, NP, H, T) with ``act``."""
    gen = _gen('edge', kind, NP, act, H, T)
    Cin, Cout = (NP, 4) if kind == 'in' else (4, NP)
    s = dict(w=C.exact_weights(gen, 9 * Cin, Cout, Cin, 3, 3), b=C.pm32(gen, Cout), dw=C.pm32(gen, Cout, Cin, 3, 3), db=C.pm32(gen, Cout))
    if kind == 'in':
        s['x'] = C.pm32(gen, B, Cin, H, T)
        s['dy'] = C.pm16(gen, dtype, B, H, T, 4)
        xv = s['x'].double()
    else:
        s['x'] = C.pm16(gen, dtype, B, H, T, 4)
        s['dy'] = C.pm32(gen, B, Cout, H, T)
        xv = C.from_cl(s['x'])
    s['xv'] = xv
    y, v, S, K = C.edge_fwd(xv, s['w'].double(), s['b'].double(), act)
    beta = K * U * S + 3 * U * s['b'].double().abs().view(1, Cout, 1, 1)
    if act == C.ACT_ELU:
        beta = beta + 4 * U * v.abs().clamp_min(1.0)
    elif act == C.ACT_SIGMOID:
        beta = beta + 4 * U
    s['y'], s['beta'] = y, beta
    return s


def _edge_entry(lib, kind, NP, which):
    return getattr(lib, 'tt_conv%s16%s_%s' % (kind, '_1' if NP == 1 else '', which))


def _edge_forward(kind, NP, act, dtype, fill, B, H, T, shifts=None):
    lib, st = _api(dtype)
    shifts = shifts or {}
    s = _edge_setup(kind, NP, act, dtype, B, H, T)
    A = _arena(fill)
    A.inp('x', s['x'], shifts.get('x', 0))
    A.inp('w', s['w'], shifts.get('w', 0))
    A.inp('b', s['b'], shifts.get('b', 0))
    if kind == 'in':
        A.out('y', (B, H, T, 4), dtype, shifts.get('y', 0))
    else:
        A.out('y', (B, NP, H, T), F32, shifts.get('y', 0))
    A.build()
    what = 'tt_conv%s16%s_fwd %s plane (%d, %d) act %d %s' % (kind, '_1' if NP == 1 else '', _tag(dtype), H, T, act, shifts or '')
    tail = (act, st) if (kind, NP) == ('out', 1) else (st,)
    rc = _finish(A, _edge_entry(lib, kind, NP, 'fwd')(A.ptr('x'), A.ptr('w'), A.ptr('b'), A.ptr('y'), B, H, T, *tail), what)
    if rc == 0:
        key = 'conv%s16%s fwd %s' % (kind, '_1' if NP == 1 else '', _tag(dtype))
        if kind == 'in':
            _hold16(key, C.from_cl(A.get('y')), s['y'], s['beta'], dtype, what)
        else:
            _hold(key, A.get('y'), s['y'], s['beta'], what)
    return rc


def _edge_backward(kind, NP, act, dtype, fill, B, H, T, shifts=None, with_dx=True, pregated=False):
    lib, st = _api(dtype)
    shifts = shifts or {}
    s = _edge_setup(kind, NP, act, dtype, B, H, T)
    Cin, Cout = (NP, 4) if kind == 'in' else (4, NP)
    A = _arena(fill)
    A.inp('x', s['x'], shifts.get('x', 0))
    ysaved = None
    if kind == 'in' and not pregated:
        ysaved = C.to_cl(s['y'].float(), dtype)                   # what the forward stored: the 16-bit rounding of the reference's output
        A.inp('y', ysaved, shifts.get('y', 0))
    if kind == 'out' and NP == 1 and act != C.ACT_NONE:
        ysaved = s['y'].float()
        A.inp('y', ysaved, shifts.get('y', 0))
    A.inp('dy', s['dy'], shifts.get('dy', 0))
    A.inp('w', s['w'], shifts.get('w', 0))
    if kind == 'out':
        A.out('dx', (B, H, T, 4), dtype, shifts.get('dx', 0))
    elif with_dx:
        A.out('dx', (B, NP, H, T), F32, shifts.get('dx', 0))
    A.acc('dw', s['dw'], shifts.get('dw', 0))
    A.acc('db', s['db'], shifts.get('db', 0))
    A.scratch('ws', lib.tt_edge16_scratch_bytes(), shifts.get('ws', 0))
    A.build()
    name = 'conv%s16%s' % (kind, '_1' if NP == 1 else '')
    what = 'tt_%s_bwd %s plane (%d, %d) act %d%s%s %s' % (name, _tag(dtype), H, T, act, '' if with_dx else ' dx NULL',
                                                       ' pregated' if pregated else '', shifts or '')
    fn = _edge_entry(lib, kind, NP, 'bwd')
    if kind == 'in':
        rc = fn(A.ptr('x'), A.ptr('y'), A.ptr('dy'), A.ptr('w'), A.ptr('dx'), A.ptr('dw'), A.ptr('db'), A.ptr('ws'), B, H, T, st)
    elif NP == 2:
        rc = fn(A.ptr('x'), A.ptr('dy'), A.ptr('w'), A.ptr('dx'), A.ptr('dw'), A.ptr('db'), A.ptr('ws'), B, H, T, st)
    else:
        rc = fn(A.ptr('x'), A.ptr('y'), A.ptr('dy'), A.ptr('w'), A.ptr('dx'), A.ptr('dw'), A.ptr('db'), A.ptr('ws'), B, H, T, act, st)
    rc = _finish(A, rc, what)
    if rc != 0:
        return rc
    if kind == 'in':
        dy = C.from_cl(s['dy'])
        if pregated:
            g, bar_g = dy, torch.zeros_like(dy)
        else:
            g = dy * C.elu_gate(C.from_cl(ysaved))
            bar_g = U * dy.abs() + U * g.abs()
    else:
        dy = s['dy'].double()
        g, r = C.act_grad(dy, ysaved.double() if ysaved is not None else None, act)
        bar_g = r * U * (1 + U) ** 2 * g.abs()
    res = C.edge_bwd(s['xv'], g, s['w'].double())
    cw, cb, cx = C.edge_carry(s['xv'].abs(), bar_g, s['w'].double().abs())
    key = '%s bwd %s' % (name, _tag(dtype))
    pw, pb = s['dw'].double(), s['db'].double()
    dw, S, K = res['dw']
    _hold(key + ' dw', A.get('dw'), pw + dw, K.view(1, 1, 3, 3) * U * S + cw + 3 * U * pw.abs(), what)
    db, Sb, Kb = res['db']
    _hold(key + ' db', A.get('db'), pb + db, Kb * U * Sb + cb + 3 * U * pb.abs(), what)
    dx, Sx, Kx = res['dx']
    if kind == 'out':
        _hold16(key + ' dx', C.from_cl(A.get('dx')), dx, Kx * U * Sx + cx, dtype, what)
    elif with_dx:
        _hold(key + ' dx', A.get('dx'), dx, Kx * U * Sx + cx, what)
    return 0


EDGE_LAYERS = [('in', 2, C.ACT_ELU), ('in', 1, C.ACT_ELU), ('out', 2, C.ACT_NONE), ('out', 1, C.ACT_NONE), ('out', 1, C.ACT_RELU),
               ('out', 1, C.ACT_SIGMOID)]
EDGE_IDS = ['in', 'in_1', 'out', 'out_1-none', 'out_1-relu', 'out_1-sigmoid']


def _edge_case(kind, NP, act, dtype, B, H, T):
    for fill in FILLS:
        assert _edge_forward(kind, NP, act, dtype, fill, B, H, T) == 0
        assert _edge_backward(kind, NP, act, dtype, fill, B, H, T) == 0
    if kind == 'in':
        assert _edge_backward(kind, NP, act, dtype, C.FILL_BIG, B, H, T, with_dx=False) == 0
        assert _edge_backward(kind, NP, act, dtype, C.FILL_BIG, B, H, T, pregated=True) == 0
        assert _edge_backward(kind, NP, act, dtype, C.FILL_NAN, B, H, T, with_dx=False, pregated=True) == 0


@pytest.mark.parametrize('H,T', EDGE_PLANES)
@pytest.mark.parametrize('kind,NP,act', EDGE_LAYERS, ids=EDGE_IDS)
@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_edge_convolutions(dtype, kind, NP, act, H, T, B=2):
    """Two-channel and _1 forms, all three activations of convout16_1, dx NULL and y NULL (pregated) of convin; planes from one pixel over the
    16 x 64 tile to one past it, T % 4 == 0 (float4 staging of the planar operand) and not."""
    _edge_case(kind, NP, act, dtype, B, H, T)


@pytest.mark.parametrize('H,T', [(35, 132), (35, 131)])
@pytest.mark.parametrize('kind,NP,act', EDGE_LAYERS, ids=EDGE_IDS)
@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_edge_convolutions_interior_tiles_capped_grid(dtype, kind, NP, act, H, T, cu_limit, B=1):
    """3 x 3 tiles on 4 workgroups: the middle tile takes the interior fast path (both stagings), the persistent loop prefetches the next
    tile under the arithmetic of this one, and convout's forward stores one iteration late."""
    cu_limit(1)
    _edge_case(kind, NP, act, dtype, B, H, T)


EDGE_FP32_POINTERS = {('in', 'fwd'): ['x', 'w', 'b'], ('in', 'bwd'): ['x', 'w', 'dx', 'dw', 'db', 'ws'],
                      ('out', 'fwd'): ['w', 'b', 'y'], ('out', 'bwd'): ['dy', 'y', 'w', 'dw', 'db', 'ws']}


@pytest.mark.parametrize('H,T', [(16, 64), (17, 68)])
@pytest.mark.parametrize('kind,NP,act', EDGE_LAYERS, ids=EDGE_IDS)
@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_edge_one_fp32_pointer_misaligned(dtype, kind, NP, act, H, T, B=2):
    """Each fp32 pointer (and the scratch) in turn one float off a 16-byte boundary, the others aligned: the same bars.  The cl16 tensors 8
    bytes off a 16-byte boundary (what a batch half of an odd plane is): the same bars."""
    for p in EDGE_FP32_POINTERS[kind, 'fwd']:
        assert _edge_forward(kind, NP, act, dtype, C.FILL_NAN, B, H, T, {p: 4}) == 0
    for p in EDGE_FP32_POINTERS[kind, 'bwd']:
        if p == 'y' and not (NP == 1 and act != C.ACT_NONE):
            continue
        assert _edge_backward(kind, NP, act, dtype, C.FILL_NAN, B, H, T, {p: 4}) == 0
    cl = {'in': ['y', 'dy'], 'out': ['x', 'dx']}[kind]
    assert _edge_forward(kind, NP, act, dtype, C.FILL_BIG, B, H, T, {cl[0]: 8}) == 0
    assert _edge_backward(kind, NP, act, dtype, C.FILL_BIG, B, H, T, {p: 8 for p in cl}) == 0


@pytest.mark.parametrize('kind,NP,act', EDGE_LAYERS[:4], ids=EDGE_IDS[:4])
@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_edge_refusals(dtype, kind, NP, act, B=1, H=3, T=4):
    """A cl16 pointer that is not a multiple of 8 bytes: TT_E_BADARG before anything is launched."""
    big = C.FILL_BIG
    if kind == 'in':
        assert _edge_forward(kind, NP, act, dtype, big, B, H, T, {'y': 4}) == BADARG
        for p in ('y', 'dy'):
            assert _edge_backward(kind, NP, act, dtype, big, B, H, T, {p: 2}) == BADARG
    else:
        assert _edge_forward(kind, NP, act, dtype, big, B, H, T, {'x': 2}) == BADARG
        for p in ('x', 'dx'):
            assert _edge_backward(kind, NP, act, dtype, big, B, H, T, {p: 4}) == BADARG
    if (kind, NP) == ('out', 1):
        lib, st = _api(dtype)
        t = torch.ones(4096, device='cuda')
        p = ctypes.c_void_p(t.data_ptr())
        assert lib.tt_convout16_1_fwd(p, p, p, p, 1, 3, 4, 1, st) == BADARG                     # TT_ACT_ELU is not an epilogue of this layer
        assert lib.tt_convout16_1_bwd(p, None, p, p, p, p, p, p, 1, 3, 4, C.ACT_RELU, st) == BADARG   # relu needs the saved output
        torch.cuda.synchronize()
        assert bool((t == 1).all())


# ---- 4. the latent heads ----------------------------------------------------------------------------------------------------------
# (CT, D, E, T, B): the capacity edges of both configurations (D = 47 / 48 of 3 row tiles, 143 / 144 of 9; 15 / 16 / 17 around one tile),
# E = 1 (one or two K steps), 2 and 31, T = 16 (one 16-frame group; a 64-pixel chunk of the weight gradient spans clips) and 80 (one whole
# chunk and a ragged one), B = 1 and 2
LATENT_CASES = [(32, 1, 31, 16, 2), (32, 15, 2, 80, 1), (32, 16, 1, 16, 2), (32, 17, 2, 16, 1), (32, 47, 31, 80, 2), (32, 48, 2, 16, 1),
                (64, 1, 2, 80, 2), (64, 128, 1, 16, 1), (64, 143, 31, 16, 2), (64, 144, 2, 80, 1)]


@functools.lru_cache(maxsize=2)
def _lat_setup(dtype, CT, D, E, T, B):
    gen = _gen('lat', CT, D, E, T, B)
    return dict(x=C.pm16(gen, dtype, B, E, T, CT), gy=C.pm16(gen, dtype, B, E, T, CT), z=C.pm32(gen, B, D, T),
                wc=C.exact_weights(gen, CT * E, D, CT, E), we=C.exact_weights(gen, D, D, CT, E), bd=C.pm32(gen, D), bc=C.pm32(gen, CT),
                dw=C.pm32(gen, D, CT, E), db=C.pm32(gen, CT))


def _lat_ws(A, lib, B, CT, D, E, T, shifts):
    A.scratch('ws', lib.tt_latent16_scratch_bytes(B, CT, D, E, T), shifts.get('ws', 0))


def _lat_contract(dtype, fill, case, gated, with_bias, Dout, pregated=False, shifts=None):
    CT, D, E, T, B = case
    lib, st = _api(dtype)
    shifts = shifts or {}
    s = _lat_setup(dtype, *case)
    A = _arena(fill)
    A.inp('in', s['x'], shifts.get('in', 0))
    if gated:
        A.inp('gy', s['gy'], shifts.get('gy', 0))
    A.inp('w', s['wc'], shifts.get('w', 0))
    if with_bias:
        A.inp('bias', s['bd'], shifts.get('bias', 0))
    A.out('out', (B, Dout, T), F32, shifts.get('out', 0))
    _lat_ws(A, lib, B, CT, D, E, T, shifts)
    A.build()
    what = 'tt_latent16_contract%s %s CT %d D %d Dout %d E %d T %d B %d%s%s %s' % (
        '_pregated' if pregated else '', _tag(dtype), CT, D, Dout, E, T, B, ' gy' if gated else '', ' bias' if with_bias else '', shifts or '')
    if pregated:
        rc = lib.tt_latent16_contract_pregated(A.ptr('in'), A.ptr('w'), A.ptr('out'), A.ptr('ws'), B, CT, D, Dout, E, T, st)
    else:
        rc = lib.tt_latent16_contract(A.ptr('in'), A.ptr('gy'), A.ptr('w'), A.ptr('bias'), A.ptr('out'), A.ptr('ws'), B, CT, D, Dout, E, T, st)
    rc = _finish(A, rc, what)
    if rc == 0:
        x = C.from_cl(s['x'])
        if gated:
            x = C.round16(x * C.elu_gate(C.from_cl(s['gy'])), dtype)       # exact in fp32, then the kernel's 16-bit operand
        v, S, K = C.lat_contract(x, s['wc'], Dout)
        bar = K * U * S
        if with_bias:
            bd = s['bd'].double()[:Dout].view(1, Dout, 1)
            v, bar = v + bd, bar + 3 * U * bd.abs()
        _hold('latent contract%s %s' % (' pregated' if pregated else '', _tag(dtype)), A.get('out'), v, bar, what)
    return rc


def _lat_expand(dtype, fill, case, with_bias, Dz, gated=False, shifts=None, fill_value=0.75):
    CT, D, E, T, B = case
    lib, st = _api(dtype)
    shifts = shifts or {}
    s = _lat_setup(dtype, *case)
    z = s['z'][:, :Dz].contiguous()
    A = _arena(fill)
    A.inp('z', z, shifts.get('z', 0))
    A.inp('w', s['we'], shifts.get('w', 0))
    if with_bias:
        A.inp('bias', s['bc'], shifts.get('bias', 0))
    if gated:
        A.inp('gy', s['gy'], shifts.get('gy', 0))
    A.out('out', (B, E, T, CT), dtype, shifts.get('out', 0))
    _lat_ws(A, lib, B, CT, D, E, T, shifts)
    A.build()
    what = 'tt_latent16_expand%s %s CT %d D %d Dz %d E %d T %d B %d%s %s' % ('_gated' if gated else '', _tag(dtype), CT, D, Dz, E, T, B,
                                                                          ' bias' if with_bias else '', shifts or '')
    if gated:
        rc = lib.tt_latent16_expand_gated(A.ptr('z'), A.ptr('w'), A.ptr('gy'), A.ptr('out'), A.ptr('ws'), B, CT, D, E, T, st)
    else:
        rc = lib.tt_latent16_expand(A.ptr('z'), Dz, fill_value, A.ptr('w'), A.ptr('bias'), A.ptr('out'), A.ptr('ws'), B, CT, D, E, T, st)
    rc = _finish(A, rc, what)
    if rc == 0:
        v, S, K = C.lat_expand(C.lat_z(z, Dz, D, fill_value, dtype), s['we'])
        beta = K * U * S
        if with_bias:
            bc = s['bc'].double().view(1, CT, 1, 1)
            a = v + bc
            v, beta = C.elu(a), beta + 3 * U * bc.abs() + 4 * U * a.abs().clamp_min(1.0)
        elif gated:
            gate = C.elu_gate(C.from_cl(s['gy']))
            v, beta = v * gate, beta * gate + 2 * U * (v * gate).abs()      # the y + 1 and the product
        _hold16('latent expand%s %s' % (' gated' if gated else (' ELU' if with_bias else ''), _tag(dtype)), C.from_cl(A.get('out')), v, beta,
                dtype, what)
    return rc


def _lat_wgrad(dtype, fill, case, gated, Dz, pregated=False, shifts=None, fill_value=0.75):
    CT, D, E, T, B = case
    lib, st = _api(dtype)
    shifts = shifts or {}
    s = _lat_setup(dtype, *case)
    z = s['z'][:, :Dz].contiguous()
    with_db = gated or pregated
    A = _arena(fill)
    A.inp('z', z, shifts.get('z', 0))
    A.inp('g', s['x'], shifts.get('g', 0))
    if gated:
        A.inp('gy', s['gy'], shifts.get('gy', 0))
    A.acc('dw', s['dw'], shifts.get('dw', 0))
    if with_db:
        A.acc('db', s['db'], shifts.get('db', 0))
    _lat_ws(A, lib, B, CT, D, E, T, shifts)
    A.build()
    what = 'tt_latent16_wgrad%s %s CT %d D %d Dz %d E %d T %d B %d%s %s' % ('_pregated' if pregated else '', _tag(dtype), CT, D, Dz, E, T, B,
                                                                         ' gy' if gated else '', shifts or '')
    if pregated:
        rc = lib.tt_latent16_wgrad_pregated(A.ptr('z'), Dz, fill_value, A.ptr('g'), A.ptr('dw'), A.ptr('db'), A.ptr('ws'), B, CT, D, E, T, st)
    else:
        rc = lib.tt_latent16_wgrad(A.ptr('z'), Dz, fill_value, A.ptr('g'), A.ptr('gy'), A.ptr('dw'), A.ptr('db'), A.ptr('ws'), B, CT, D, E, T, st)
    rc = _finish(A, rc, what)
    if rc == 0:
        g = C.from_cl(s['x'])
        gsum = g
        if gated:
            gsum = g * C.elu_gate(C.from_cl(s['gy']))                      # exact in fp32: the bias gradient sums it unrounded,
            g = C.round16(gsum, dtype)                                     # the matrix operand is its 16-bit rounding
        dw, S, K, _, _, _ = C.lat_wgrad(C.lat_z(z, Dz, D, fill_value, dtype), g)
        _, _, _, db, Sb, Kb = C.lat_wgrad(C.lat_z(z, Dz, D, fill_value, dtype), gsum)
        key = 'latent wgrad%s %s' % (' pregated' if pregated else (' gated' if gated else ''), _tag(dtype))
        pw = s['dw'].double()
        _hold(key + ' dw', A.get('dw'), pw + dw, K * U * S + 3 * U * pw.abs(), what)
        if with_db:
            pb = s['db'].double()
            _hold(key + ' db', A.get('db'), pb + db, Kb * U * Sb + 3 * U * pb.abs(), what)
    return rc


@pytest.mark.parametrize('case', LATENT_CASES, ids=['CT%d-D%d-E%d-T%d-B%d' % c for c in LATENT_CASES])
@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_latent_heads(dtype, case):
    """contract (with and without gy, with and without bias, Dout = D and D - 1), expand (Dz = D and D - 1 with fill, with and without
    bias), expand_gated, wgrad (both forms, Dz = D and D - 1), and the pregated pair where tt_latent16_pregated_ok says so."""
    CT, D, E, T, B = case
    lib, _ = _api(dtype)
    ok = lib.tt_latent16_pregated_ok(CT, D)
    assert ok == int(D < (48 if CT == 32 else 144))
    lo = max(D - 1, 1)
    for fill in FILLS:
        first = fill == C.FILL_NAN
        assert _lat_contract(dtype, fill, case, gated=not first, with_bias=first, Dout=D) == 0
        assert _lat_contract(dtype, fill, case, gated=first, with_bias=not first, Dout=lo) == 0
        assert _lat_expand(dtype, fill, case, with_bias=first, Dz=D) == 0
        assert _lat_expand(dtype, fill, case, with_bias=not first, Dz=D - 1 if D > 1 else D) == 0
        assert _lat_expand(dtype, fill, case, with_bias=False, Dz=D, gated=True) == 0
        assert _lat_wgrad(dtype, fill, case, gated=first, Dz=D) == 0
        assert _lat_wgrad(dtype, fill, case, gated=not first, Dz=D - 1 if D > 1 else D) == 0
        want = 0 if ok else UNSUPPORTED
        assert _lat_contract(dtype, fill, case, gated=False, with_bias=False, Dout=lo if first else D, pregated=True) == want
        assert _lat_wgrad(dtype, fill, case, gated=False, Dz=D if first else (D - 1 if D > 1 else D), pregated=True) == want


@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_latent_pregated_agrees_with_ok(dtype):
    """tt_latent16_pregated_ok is the promise a caller makes before it hands on a gated gradient: BOTH pregated entry points refuse exactly where
    it says 0 (tt_latent16_contract_pregated used to run at D = 48 / 144), with nothing written."""
    lib, _ = _api(dtype)
    for case in [(32, 47, 1, 16, 1), (32, 48, 1, 16, 1), (64, 143, 1, 16, 1), (64, 144, 1, 16, 1)]:
        CT, D = case[:2]
        want = 0 if lib.tt_latent16_pregated_ok(CT, D) else UNSUPPORTED
        assert want == (0 if D in (47, 143) else UNSUPPORTED)
        assert _lat_contract(dtype, C.FILL_BIG, case, False, False, D, pregated=True) == want
        assert _lat_wgrad(dtype, C.FILL_BIG, case, False, D, pregated=True) == want
    assert lib.tt_latent16_pregated_ok(32, 49) == 0 and lib.tt_latent16_pregated_ok(16, 8) == 0


@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_latent_one_fp32_pointer_misaligned(dtype, case=(32, 17, 2, 16, 2)):
    """Each fp32 pointer of each entry point one float off a 16-byte boundary: 4-byte accesses, the same bars."""
    nan = C.FILL_NAN
    for p in ('w', 'bias', 'out'):
        assert _lat_contract(dtype, nan, case, True, True, 17, shifts={p: 4}) == 0
    for p in ('w', 'out'):
        assert _lat_contract(dtype, nan, case, False, False, 16, pregated=True, shifts={p: 4}) == 0
    for p in ('z', 'w', 'bias'):
        assert _lat_expand(dtype, nan, case, True, 16, shifts={p: 4}) == 0
    for p in ('z', 'w'):
        assert _lat_expand(dtype, nan, case, False, 17, gated=True, shifts={p: 4}) == 0
    for p in ('z', 'dw', 'db'):
        assert _lat_wgrad(dtype, nan, case, True, 17, shifts={p: 4}) == 0
        assert _lat_wgrad(dtype, nan, case, False, 16, pregated=True, shifts={p: 4}) == 0


@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_latent_refusals(dtype, case=(32, 17, 2, 16, 1)):
    """T % 16, a head that is not compiled, Dout / Dz out of range, and every cl16 pointer and the scratch in turn off their 16-byte
    boundary: refused before anything is launched."""
    big = C.FILL_BIG
    odd = (32, 17, 2, 24, 1)
    assert _lat_contract(dtype, big, odd, False, True, 17) == BADARG
    assert _lat_contract(dtype, big, odd, False, False, 17, pregated=True) == BADARG
    assert _lat_expand(dtype, big, odd, True, 17) == BADARG
    assert _lat_expand(dtype, big, odd, False, 17, gated=True) == BADARG
    assert _lat_wgrad(dtype, big, odd, True, 17) == BADARG
    assert _lat_wgrad(dtype, big, odd, False, 17, pregated=True) == BADARG
    assert _lat_contract(dtype, big, case, False, True, 18) == BADARG
    assert _lat_expand(dtype, big, case, True, 15) == BADARG
    assert _lat_wgrad(dtype, big, case, True, 15) == BADARG
    lib, st = _api(dtype)
    assert lib.tt_latent16_scratch_bytes(1, 32, 49, 2, 16) == -1 and lib.tt_latent16_scratch_bytes(1, 48, 8, 2, 16) == -1
    for p in ('in', 'gy', 'ws'):
        assert _lat_contract(dtype, big, case, True, True, 17, shifts={p: 8}) == BADARG
    for p in ('in', 'ws'):
        assert _lat_contract(dtype, big, case, False, False, 17, pregated=True, shifts={p: 8}) == BADARG
    for p in ('out', 'ws'):
        assert _lat_expand(dtype, big, case, True, 17, shifts={p: 8}) == BADARG
    for p in ('gy', 'out', 'ws'):
        assert _lat_expand(dtype, big, case, False, 17, gated=True, shifts={p: 8}) == BADARG
    for p in ('g', 'gy', 'ws'):
        assert _lat_wgrad(dtype, big, case, True, 17, shifts={p: 8}) == BADARG
    for p in ('g', 'ws'):
        assert _lat_wgrad(dtype, big, case, False, 17, pregated=True, shifts={p: 8}) == BADARG


# ---- 5. the strided pair ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _stride_setup(kind, Cc, dtype, B, H, T, out_pad):
    """Operands of one strided layer and its float64 forward.  y and dy of the backward are free 16-bit operands in +-[0.5, 1] (the backward
    reads the saved output as data): the gate dy * min(y + 1, 1) is then exact in fp32 and its 16-bit rounding inside the kernels is known
    bit for bit."""
    gen = _gen('stride', kind, Cc, H, T, out_pad)
    Ci, Co = (Cc, 2 * Cc) if kind == 'sconv' else (2 * Cc, Cc)
    s = dict(x=C.pm16(gen, dtype, B, H, T, Ci), w=C.exact_weights(gen, 4 * Cc, 2 * Cc, Cc, 4, 1), b=C.pm32(gen, Co),
             dw=C.pm32(gen, 2 * Cc, Cc, 4, 1), db=C.pm32(gen, Co))
    s['xv'] = C.from_cl(s['x'])
    y, v, S, K = C.stride_fwd(kind, Cc, s['xv'], s['w'].double(), s['b'].double(), out_pad)
    s['y'], s['Hout'] = y, y.size(2)
    s['beta'] = K * U * S + 3 * U * s['b'].double().abs().view(1, Co, 1, 1) + 4 * U * v.abs().clamp_min(1.0)
    s['ysaved'] = C.pm16(gen, dtype, B, s['Hout'], T, Co)
    s['dy'] = C.pm16(gen, dtype, B, s['Hout'], T, Co)
    return s


def _stride_tail(kind, B, Cc, H, T, out_pad, st, extra=()):
    return (B, Cc, H, T) + ((out_pad,) if kind == 'tconv' else ()) + tuple(extra) + (st,)


def _stride_forward(kind, Cc, dtype, fill, B, H, T, out_pad=0, shifts=None):
    lib, st = _api(dtype)
    shifts = shifts or {}
    if kind == 'sconv' and H < 4:                        # refused: no forward to restate
        Ci, Co, Hout = Cc, 2 * Cc, 1
        s = dict(x=C.pm16(_gen(H), dtype, B, H, T, Ci), w=C.pm32(_gen(1), 2 * Cc, Cc, 4, 1), b=C.pm32(_gen(2), Co))
    else:
        s = _stride_setup(kind, Cc, dtype, B, H, T, out_pad)
        Co, Hout = s['b'].numel(), s['Hout']
    A = _arena(fill)
    A.inp('x', s['x'], shifts.get('x', 0))
    A.inp('w', s['w'], shifts.get('w', 0))
    A.inp('b', s['b'], shifts.get('b', 0))
    A.out('y', (B, Hout, T, Co), dtype, shifts.get('y', 0))
    A.build()
    what = 'tt_%s16_fwd %s C %d plane (%d, %d) out_pad %d %s' % (kind, _tag(dtype), Cc, H, T, out_pad, shifts or '')
    fn = getattr(lib, 'tt_%s16_fwd' % kind)
    rc = _finish(A, fn(A.ptr('x'), A.ptr('w'), A.ptr('b'), A.ptr('y'), *_stride_tail(kind, B, Cc, H, T, out_pad, st)), what)
    if rc == 0:
        _hold16('%s16 fwd %s' % (kind, _tag(dtype)), C.from_cl(A.get('y')), s['y'], s['beta'], dtype, what)
    return rc


def _stride_backward(kind, Cc, dtype, fill, B, H, T, out_pad=0, shifts=None, with_dx=True, pregated=False, gate_dx=0):
    lib, st = _api(dtype)
    shifts = shifts or {}
    refused_shape = kind == 'sconv' and H < 4
    s = _stride_setup(kind, Cc, dtype, B, 4 if refused_shape else H, T, out_pad)
    Ci = Cc if kind == 'sconv' else 2 * Cc
    x = s['x'][:, :H] if refused_shape else s['x']
    A = _arena(fill)
    A.inp('x', x.contiguous(), shifts.get('x', 0))
    if not pregated:
        A.inp('y', s['ysaved'], shifts.get('y', 0))
    A.inp('dy', s['dy'], shifts.get('dy', 0))
    A.inp('w', s['w'], shifts.get('w', 0))
    if with_dx:
        A.out('dx', (B, H, T, Ci), dtype, shifts.get('dx', 0))
    A.acc('dw', s['dw'], shifts.get('dw', 0))
    A.acc('db', s['db'], shifts.get('db', 0))
    A.scratch('ws', lib.tt_stride16_scratch_bytes(Cc), shifts.get('ws', 0))
    A.build()
    name = 'tt_%s16_bwd%s' % (kind, '_pregated' if pregated else '')
    what = '%s %s C %d plane (%d, %d) out_pad %d%s%s %s' % (name, _tag(dtype), Cc, H, T, out_pad, '' if with_dx else ' dx NULL',
                                                          ' gate_dx' if gate_dx else '', shifts or '')
    fn = getattr(lib, name)
    if pregated:
        extra = (gate_dx,) if kind == 'tconv' else ()
        rc = fn(A.ptr('x'), A.ptr('dy'), A.ptr('w'), A.ptr('dx'), A.ptr('dw'), A.ptr('db'), A.ptr('ws'),
                *_stride_tail(kind, B, Cc, H, T, out_pad, st, extra))
    else:
        rc = fn(A.ptr('x'), A.ptr('y'), A.ptr('dy'), A.ptr('w'), A.ptr('dx'), A.ptr('dw'), A.ptr('db'), A.ptr('ws'),
                *_stride_tail(kind, B, Cc, H, T, out_pad, st))
    rc = _finish(A, rc, what)
    if rc != 0:
        return rc
    dy = C.from_cl(s['dy'])
    if pregated:
        g, gsum = dy, dy
    else:
        gsum = dy * C.elu_gate(C.from_cl(s['ysaved']))            # exact in fp32: what the bias gradient sums,
        g = C.round16(gsum, dtype)                                # and its 16-bit rounding, the matrix operand
    res = C.stride_bwd(kind, Cc, s['xv'], g, s['w'].double(), gsum)
    key = '%s16 bwd%s %s' % (kind, ' pregated' if pregated else '', _tag(dtype))
    pw, pb = s['dw'].double(), s['db'].double()
    dw, S, K = res['dw']
    _hold(key + ' dw', A.get('dw'), pw + dw, K * U * S + 3 * U * pw.abs(), what)
    db, Sb, Kb = res['db']
    _hold(key + ' db', A.get('db'), pb + db, Kb * U * Sb + 3 * U * pb.abs(), what)
    if with_dx:
        dx, Sx, Kx = res['dx']
        beta = Kx * U * Sx
        if gate_dx:
            gate = C.elu_gate(s['xv'])
            dx, beta = dx * gate, beta * gate + 2 * U * (dx * gate).abs()     # the x + 1 and the product
        got = C.from_cl(A.get('dx'))
        _hold16(key + (' dx gated' if gate_dx else ' dx'), got, dx, beta, dtype, what)
        if kind == 'sconv' and H % 2 == 1:
            assert bool((got[:, :, -1] == 0).all()), 'the unused last input row has no term: its dx is 0'
    return 0


@pytest.mark.parametrize('T', [2, 4, 30, 66])
@pytest.mark.parametrize('H', [4, 5, 6, 7, 13])
@pytest.mark.parametrize('Cc', [4, 8, 16, 32])
@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_sconv16(dtype, Cc, H, T, B=2):
    """tt_sconv16_fwd / _bwd / _bwd_pregated, dx given and NULL: the minimum height (one output row), odd heights (the last input row is
    unused: its dx row is exactly 0), more rows than one tile of the weight-gradient kernel at C >= 8; T from one pixel pair to one past
    the 64-frame tile."""
    for fill in FILLS:
        assert _stride_forward('sconv', Cc, dtype, fill, B, H, T) == 0
        assert _stride_backward('sconv', Cc, dtype, fill, B, H, T) == 0
        assert _stride_backward('sconv', Cc, dtype, fill, B, H, T, pregated=True) == 0
    assert _stride_backward('sconv', Cc, dtype, C.FILL_BIG, B, H, T, with_dx=False) == 0
    assert _stride_backward('sconv', Cc, dtype, C.FILL_NAN, B, H, T, with_dx=False, pregated=True) == 0


@pytest.mark.parametrize('T', [2, 4, 30, 66])
@pytest.mark.parametrize('H,out_pad', [(1, 0), (1, 1), (2, 0), (2, 1), (3, 1), (9, 0), (9, 1)])
@pytest.mark.parametrize('Cc', [4, 8, 16, 32])
@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_tconv16(dtype, Cc, H, out_pad, T, B=2):
    """tt_tconv16_fwd / _bwd / _bwd_pregated with and without the output-padding row, dx given and NULL, and gate_dx: dx * ELU'(x) at
    C = 16, 32, TT_E_UNSUPPORTED with nothing written at C = 4, 8."""
    for fill in FILLS:
        assert _stride_forward('tconv', Cc, dtype, fill, B, H, T, out_pad) == 0
        assert _stride_backward('tconv', Cc, dtype, fill, B, H, T, out_pad) == 0
        assert _stride_backward('tconv', Cc, dtype, fill, B, H, T, out_pad, pregated=True) == 0
        assert _stride_backward('tconv', Cc, dtype, fill, B, H, T, out_pad, pregated=True, gate_dx=1) == (0 if Cc >= 16 else UNSUPPORTED)
    assert _stride_backward('tconv', Cc, dtype, C.FILL_BIG, B, H, T, out_pad, with_dx=False) == 0
    assert _stride_backward('tconv', Cc, dtype, C.FILL_NAN, B, H, T, out_pad, with_dx=False, pregated=True) == 0


@pytest.mark.parametrize('Cc', [4, 32])
@pytest.mark.parametrize('kind', ['sconv', 'tconv'])
@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_strided_one_fp32_pointer_misaligned(dtype, kind, Cc, B=2, T=66):
    """w, b, dw, db and the scratch (fp32 partials) in turn one float off a 16-byte boundary: 4-byte accesses, the same bars."""
    H, out_pad = (7, 0) if kind == 'sconv' else (3, 1)
    for p in ('w', 'b'):
        assert _stride_forward(kind, Cc, dtype, C.FILL_NAN, B, H, T, out_pad, {p: 4}) == 0
    for p in ('w', 'dw', 'db', 'ws'):
        assert _stride_backward(kind, Cc, dtype, C.FILL_NAN, B, H, T, out_pad, {p: 4}) == 0
        assert _stride_backward(kind, Cc, dtype, C.FILL_NAN, B, H, T, out_pad, {p: 4}, pregated=True) == 0


@pytest.mark.parametrize('Cc', [4, 16])
@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_strided_refusals(dtype, Cc, B=1):
    """H < 4 for sconv, T odd at C = 4, gate_dx without dx, and every cl16 pointer in turn off its 16-byte boundary: TT_E_BADARG before
    anything is launched."""
    big = C.FILL_BIG
    assert _stride_forward('sconv', Cc, dtype, big, B, 3, 4) == BADARG
    assert _stride_backward('sconv', Cc, dtype, big, B, 3, 4) == BADARG
    assert _stride_backward('sconv', Cc, dtype, big, B, 3, 4, pregated=True) == BADARG
    if Cc == 4:
        for kind in ('sconv', 'tconv'):
            assert _stride_forward(kind, 4, dtype, big, B, 5, 3) == BADARG
            assert _stride_backward(kind, 4, dtype, big, B, 5, 3) == BADARG
            assert _stride_backward(kind, 4, dtype, big, B, 5, 3, pregated=True) == BADARG
    assert _stride_backward('tconv', Cc, dtype, big, B, 2, 4, 1, with_dx=False, pregated=True, gate_dx=1) == BADARG
    for kind, H in (('sconv', 6), ('tconv', 2)):
        for p in ('x', 'y'):
            assert _stride_forward(kind, Cc, dtype, big, B, H, 4, 0, {p: 8}) == BADARG
        for p in ('x', 'y', 'dy', 'dx'):
            assert _stride_backward(kind, Cc, dtype, big, B, H, 4, 0, {p: 8}) == BADARG
        for p in ('x', 'dy', 'dx'):
            assert _stride_backward(kind, Cc, dtype, big, B, H, 4, 0, {p: 8}, pregated=True) == BADARG


# ---- 6. refusals of the residual-block and level entry points (no kernel runs; their parity is not in this file yet) ---------------------
@pytest.mark.parametrize('Cc', [4, 16, 32])
@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_block_and_level_refusals(dtype, Cc, B=1, H=3, T=6):
    """Every cl16 pointer and the scratch of tt_wide_rb_fwd / _fwd_join / _bwd / _bwd_onepass / _bwd_fused and of the three level calls in turn
    8 bytes off its 16-byte boundary: TT_E_BADARG before anything is launched (LDS-DMA on x, h1, dy and the dA1 region of ws, 16-byte pieces
    elsewhere).  T odd at C = 4: TT_E_BADARG.  tt_wide_level_bwd_gated_join with a first dilation other than 1: TT_E_UNSUPPORTED.  Nothing
    is written in any of them."""
    lib, st = _api(dtype)
    buf = torch.full((1 << 16,), 0x3C, dtype=torch.uint8, device='cuda')
    before = buf.clone()
    base = buf.data_ptr()
    assert base % 256 == 0

    def P(i, off=0):                                             # the i-th 4 KiB slot of the buffer
        return ctypes.c_void_p(base + 4096 * i + off)

    w = P(10)
    names = ['x', 'y', 'h1', 'skip', 'dy', 'dx', 'ws', 'tmp0', 'tmp1', 'skip_g']

    def ptrs(bad=None):
        return {k: P(i, 8 if k == bad else 0) for i, k in enumerate(names)}

    def arr(p, nb):
        return (ctypes.c_void_p * nb)(*[p] * nb)

    def fwd(p):
        return lib.tt_wide_rb_fwd(p['x'], w, w, w, w, p['y'], p['h1'], B, Cc, H, T, 1, st)

    def fwd_join(p):
        return lib.tt_wide_rb_fwd_join(p['x'], w, w, w, w, p['y'], p['h1'], p['skip'], w, 0, 1, B, Cc, H, T, 1, st)

    def bwd(p, entry='tt_wide_rb_bwd'):
        return getattr(lib, entry)(p['x'], p['h1'], p['dy'], w, w, w, p['dx'], w, w, w, w, p['ws'], B, Cc, H, T, 1, st)

    def fused(p):
        return lib.tt_wide_rb_bwd_fused(p['x'], p['dy'], w, w, w, w, p['dx'], w, w, w, w, p['ws'], B, Cc, H, T, 1, st)

    def level(p, entry, nb=2, dil=(1, 2), badx=False):
        xs = arr(P(0, 8 if badx == 'x' else 0), nb)
        hs = arr(P(2, 8 if badx == 'h1' else 0), nb)
        ws_, fs = arr(w, nb), arr(w, nb)
        d = (ctypes.c_int * nb)(*dil)
        args = [nb, xs, hs, p['dy'], ws_, ws_, ws_, p['dx'], p['tmp0'], p['tmp1'], fs, fs, fs, fs, p['ws'], B, Cc, H, T, d]
        if entry.endswith('_join'):
            args += [p['skip_g'], 1, w, 0, w]
        return getattr(lib, entry)(*args, st)

    for bad in ('x', 'y', 'h1'):
        assert fwd(ptrs(bad)) == BADARG, bad
    for bad in ('x', 'y', 'h1', 'skip'):
        assert fwd_join(ptrs(bad)) == BADARG, bad
    for bad in ('x', 'h1', 'dy', 'dx', 'ws'):
        assert bwd(ptrs(bad)) == BADARG, bad
        if Cc >= 16:
            assert bwd(ptrs(bad), 'tt_wide_rb_bwd_onepass') == BADARG, bad
    if Cc >= 16:
        for bad in ('x', 'dy', 'dx', 'ws'):
            assert fused(ptrs(bad)) == BADARG, bad
    for entry in ('tt_wide_level_bwd', 'tt_wide_level_bwd_gated', 'tt_wide_level_bwd_gated_join'):
        for bad in ('dy', 'dx', 'tmp0', 'tmp1', 'ws') + (('skip_g',) if entry.endswith('_join') else ()):
            assert level(ptrs(bad), entry) == BADARG, (entry, bad)
        for bad in ('x', 'h1'):
            assert level(ptrs(), entry, badx=bad) == BADARG, (entry, bad)
    assert level(ptrs(), 'tt_wide_level_bwd_gated_join', dil=(2, 1)) == UNSUPPORTED
    assert level(ptrs(), 'tt_wide_level_bwd_gated_join', nb=1, dil=(3,)) == UNSUPPORTED
    if Cc == 4:
        p = ptrs()
        assert bwd(p, 'tt_wide_rb_bwd_onepass') == UNSUPPORTED and fused(p) == UNSUPPORTED      # the strips and the fused form: C = 16, 32
        assert lib.tt_wide_rb_fwd(p['x'], w, w, w, w, p['y'], p['h1'], B, 4, H, 5, 1, st) == BADARG
        assert lib.tt_wide_rb_bwd(p['x'], p['h1'], p['dy'], w, w, w, p['dx'], w, w, w, w, p['ws'], B, 4, H, 5, 1, st) == BADARG
        assert lib.tt_wide_scratch_bytes(B, 4, H, 5) == -1
    torch.cuda.synchronize()
    assert torch.equal(buf, before), 'a refused call wrote'


# ---- 7. the one caller that hands in less than 16-byte alignment ----------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_pair_wrapper_hands_the_halves_of_an_odd_plane_to_the_edge_convolutions(dtype, H=3, T=5):
    """ops.ConvOut16PairFn runs tt_convout16_fwd / _bwd on the two batch halves of ONE cl16 tensor.  With one clip of 3 x 5 pixels per half
    the second half starts 120 bytes in -- 8 bytes off a 16-byte boundary, the case the 8-byte requirement of the edge convolutions leaves
    room for: outputs and dx equal, bit for bit, what ops.ConvOut16Fn gives for each half as a tensor of its own."""
    from timbre_trap.framework import ops
    gen = _gen('pair', H, T)
    x = C.pm16(gen, dtype, 2, H, T, 4).cuda().permute(0, 3, 1, 2)
    assert ops.is_cl16(x) and x[1:].data_ptr() % 16 == 8
    w, b = C.exact_weights(gen, 36, 2, 4, 3, 3).cuda(), C.pm32(gen, 2).cuda()
    g = [C.pm32(gen, 1, 2, H, T).cuda() for _ in range(2)]
    xa = x.clone().requires_grad_()
    ya = ops.ConvOut16PairFn.apply(xa, w, b)
    torch.autograd.backward(list(ya), g)
    for i in range(2):
        xi = x[i:i + 1].clone().requires_grad_()
        assert xi.data_ptr() % 16 == 0
        yi = ops.ConvOut16Fn.apply(xi, w, b)
        yi.backward(g[i])
        assert torch.equal(yi, ya[i]) and torch.equal(xi.grad, xa.grad[i:i + 1]), i


# ---- 8. the residual block, forward -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _rb_setup(Cc, d, dtype, B, H, T):
    gen = _gen('rb', Cc, d, H, T)
    s = dict(x=C.pm16(gen, dtype, B, H, T, Cc), w1=C.exact_weights(gen, 9 * Cc, Cc, Cc, 3, 3), b1=C.pm32(gen, Cc),
             w2=C.exact_weights(gen, Cc, Cc, Cc), b2=C.pm32(gen, Cc), skip=C.pm16(gen, dtype, B, H, T, Cc), sw=C.pm32(gen, 3))
    s['xv'] = C.from_cl(s['x'])
    h, a1, S1, K1 = C.rb_stage1(s['xv'], s['w1'].double(), s['b1'].double(), d)
    s['h'] = h
    s['beta_h'] = K1 * U * S1 + 3 * U * s['b1'].double().abs().view(1, Cc, 1, 1) + 4 * U * a1.abs().clamp_min(1.0)
    return s


def _rb_forward(Cc, d, dtype, fill, B, H, T, with_h1, skip_B=0, with_sw=True, shifts=None):
    """tt_wide_rb_fwd (skip_B = 0) or tt_wide_rb_fwd_join.  h1 given: held to its own bar, then the kernel's own tensor -- bit for bit the
    16-bit operand of its second product -- feeds the second stage of the restatement.  h1 NULL: the rounded hidden activation is not
    observable; the restatement rounds its own at the same place and the bar of y grows by |W2| . boundary_spread, which is 0 except for
    elements within their bar of a rounding boundary."""
    lib, st = _api(dtype)
    shifts = shifts or {}
    s = _rb_setup(Cc, d, dtype, B, H, T)
    A = _arena(fill)
    A.inp('x', s['x'], shifts.get('x', 0))
    for n in ('w1', 'b1', 'w2', 'b2'):
        A.inp(n, s[n], shifts.get(n, 0))
    if skip_B:
        A.inp('skip', s['skip'][:skip_B].contiguous())
        if with_sw:
            A.inp('sw', s['sw'], shifts.get('sw', 0))
    A.out('y', (B, H, T, Cc), dtype)
    if with_h1:
        A.out('h1', (B, H, T, Cc), dtype)
    A.build()
    what = 'tt_wide_rb_fwd%s %s C %d d %d plane (%d, %d) B %d %s h1%s %s' % (
        '_join' if skip_B else '', _tag(dtype), Cc, d, H, T, B, 'with' if with_h1 else 'without',
        ' skip_B %d%s' % (skip_B, '' if with_sw else ' weights NULL') if skip_B else '', shifts or '')
    if skip_B:
        rc = lib.tt_wide_rb_fwd_join(A.ptr('x'), A.ptr('w1'), A.ptr('b1'), A.ptr('w2'), A.ptr('b2'), A.ptr('y'), A.ptr('h1'), A.ptr('skip'),
                                     A.ptr('sw'), 1, skip_B, B, Cc, H, T, d, st)
    else:
        rc = lib.tt_wide_rb_fwd(A.ptr('x'), A.ptr('w1'), A.ptr('b1'), A.ptr('w2'), A.ptr('b2'), A.ptr('y'), A.ptr('h1'), B, Cc, H, T, d, st)
    rc = _finish(A, rc, what)
    if rc != 0:
        return rc
    key = 'rb_fwd%s C%d %s' % ('_join' if skip_B else '', Cc, _tag(dtype))
    W2 = s['w2'].double()
    if with_h1:
        hh = C.from_cl(A.get('h1'))
        _hold16(key + ' h1', hh, s['h'], s['beta_h'], dtype, what)
        carried = 0.0
    else:
        hh = C.round16(s['h'], dtype)
        carried = torch.einsum('oc,bcht->boht', W2.abs(), C.boundary_spread(s['h'], s['beta_h'], dtype))
    e, a2, S2 = C.rb_stage2(hh, W2, s['b2'].double())
    want = e + s['xv']
    beta = Cc * U * S2 + 3 * U * s['b2'].double().abs().view(1, Cc, 1, 1) + 4 * U * a2.abs().clamp_min(1.0) + U * want.abs() + carried
    if skip_B:
        sc = float(s['sw'][1]) if with_sw else 1.0
        sk = C.from_cl(s['skip'][:skip_B]).repeat(B // skip_B, 1, 1, 1)          # clip b joins the embedding b mod skip_B
        want = want + sc * sk
        beta = beta + U * want.abs()                                             # the fma of the join
    _hold16(key + (' y' if with_h1 else ' y (h1 NULL)'), C.from_cl(A.get('y')), want, beta, dtype, what)
    return 0


def _rb_case(Cc, d, dtype, B, H, T):
    for fill in FILLS:
        assert _rb_forward(Cc, d, dtype, fill, B, H, T, True) == 0
        assert _rb_forward(Cc, d, dtype, fill, B, H, T, False) == 0
    assert _rb_forward(Cc, d, dtype, C.FILL_BIG, B, H, T, True, skip_B=B) == 0
    assert _rb_forward(Cc, d, dtype, C.FILL_NAN, B, H, T, False, skip_B=B // 2, with_sw=False) == 0
    assert _rb_forward(Cc, d, dtype, C.FILL_BIG, B, H, T, False, skip_B=B // 2) == 0


@pytest.mark.parametrize('H,T', PLANES)
@pytest.mark.parametrize('d', [1, 2, 3])
@pytest.mark.parametrize('Cc', [4, 8, 16, 32])
@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_residual_block_forward(dtype, Cc, d, H, T):
    """tt_wide_rb_fwd with h1 given and NULL, tt_wide_rb_fwd_join with skip_B = B and B / 2, weights given and NULL; planes smaller than the
    halo (every tap but the centre outside at dilation 3), exact tiles (8 x 64 at C = 16, 32; 16 x 64 at C = 4, 8), one past, one short.
    This is the kernel family whose ELU is the median form: a NaN it reads from a halo that is not there would come out as 0, the 0x46
    fill as a large finite value."""
    _rb_case(Cc, d, dtype, 2, H, T)


@pytest.mark.parametrize('d', [1, 2, 3])
@pytest.mark.parametrize('Cc', [4, 8, 16, 32])
@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_residual_block_forward_multitile(dtype, Cc, d, cu_limit, H=17, T=130):
    """One CU's worth of workgroups walks the tiles of two clips of (17, 130): the persistent loop, and the join's pairing of the two halves'
    tiles."""
    cu_limit(1)
    _rb_case(Cc, d, dtype, 2, H, T)


@pytest.mark.parametrize('Cc', [4, 32])
@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_residual_block_forward_one_fp32_pointer_misaligned(dtype, Cc, d=2, H=9, T=66):
    """w1, b1, w2, b2 and the skip weights in turn one float off a 16-byte boundary: 4-byte loads, the same bars."""
    for p in ('w1', 'b1', 'w2', 'b2', 'sw'):
        assert _rb_forward(Cc, d, dtype, C.FILL_NAN, 2, H, T, True, skip_B=1, shifts={p: 4}) == 0


# ---- 9. the residual block, backward ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _rbb_setup(Cc, d, dtype, B, H, T, seed=0):
    """Operands of one block backward.  h1 is a free 16-bit operand in +-[0.5, 1] (the backward reads the saved activation as data): its
    gate min(h1 + 1, 1) is exact."""
    gen = _gen('rbb', Cc, d, H, T, seed)
    return dict(x=C.pm16(gen, dtype, B, H, T, Cc), h1=C.pm16(gen, dtype, B, H, T, Cc), dy=C.pm16(gen, dtype, B, H, T, Cc),
                w1=C.exact_weights(gen, 9 * Cc, Cc, Cc, 3, 3), w2=C.exact_weights(gen, Cc, Cc, Cc), b2=C.pm32(gen, Cc),
                dw1=C.pm32(gen, Cc, Cc, 3, 3), db1=C.pm32(gen, Cc), dw2=C.pm32(gen, Cc, Cc), db2=C.pm32(gen, Cc), b1=C.pm32(gen, Cc))


GRADS = ('dw1', 'db1', 'dw2', 'db2')


def _rb_backward_call(entry, s, Cc, d, dtype, fill, B, H, T, dy=None, shifts=None):
    """One tt_wide_rb_bwd / _bwd_onepass call in an arena of its own -> (rc, outputs: dx, the four gradients, and the 16-bit dA1 region of ws
    where the per-stage kernels of C = 32 leave it)."""
    lib, st = _api(dtype)
    shifts = shifts or {}
    dy = s['dy'] if dy is None else dy
    fused = entry == 'tt_wide_rb_bwd_fused'
    A = _arena(fill)
    for n in ('x',) if fused else ('x', 'h1'):
        A.inp(n, s[n])
    A.inp('dy', dy)
    for n in ('w1', 'b1', 'w2', 'b2') if fused else ('w1', 'w2', 'b2'):
        A.inp(n, s[n], shifts.get(n, 0))
    A.out('dx', (B, H, T, Cc), dtype)
    for n in GRADS:
        A.acc(n, s[n], shifts.get(n, 0))
    nbytes = (lib.tt_wide_scratch_bytes(B, Cc, H, T) if entry == 'tt_wide_rb_bwd' else
              lib.tt_wide_fused_scratch_bytes(Cc) if fused else lib.tt_wide_onepass_scratch_bytes(Cc))
    A.scratch('ws', nbytes)
    A.build()
    what = '%s %s C %d d %d plane (%d, %d) B %d %s' % (entry, _tag(dtype), Cc, d, H, T, B, shifts or '')
    if fused:
        rc = lib.tt_wide_rb_bwd_fused(A.ptr('x'), A.ptr('dy'), A.ptr('w1'), A.ptr('b1'), A.ptr('w2'), A.ptr('b2'), A.ptr('dx'), A.ptr('dw1'),
                                      A.ptr('db1'), A.ptr('dw2'), A.ptr('db2'), A.ptr('ws'), B, Cc, H, T, d, st)
    else:
        rc = getattr(lib, entry)(A.ptr('x'), A.ptr('h1'), A.ptr('dy'), A.ptr('w1'), A.ptr('w2'), A.ptr('b2'), A.ptr('dx'), A.ptr('dw1'),
                                 A.ptr('db1'), A.ptr('dw2'), A.ptr('db2'), A.ptr('ws'), B, Cc, H, T, d, st)
    rc = _finish(A, rc, what)
    out = {}
    if rc == 0:
        out = {n: A.get(n) for n in ('dx',) + GRADS}
        if entry == 'tt_wide_rb_bwd' and Cc == 32:
            out['da1'] = A.get('ws')[:B * H * T * Cc * 2].view(dtype).view(B, H, T, Cc)
    return rc, out, what


def _rb_backward(Cc, d, dtype, fill, B, H, T, shifts=None, onepass=False, fused=False):
    """tt_wide_rb_bwd at C = 4, 8 (k_nrb_bwd_fused), C = 16 (the strips, k_wrb_bwds) and C = 32 (k_wrb_bwd_a, k_wrb_dxw) against float64.  From
    the kernels, the same at every width: a2 = W2 h1 + b2 in fp32; dA2 = dy min(exp(a2), 1) in fp32, summed UNROUNDED into db2, rounded to 16 bits as the operand of dW2 and of
    W2^T . (not observable: the restatement rounds its own, bars grow by boundary_spread); dA1 = (W2^T dA2) min(h1 + 1, 1) in fp32, summed
    UNROUNDED into db1, rounded to 16 bits for dx and dW1.  C = 32 stores that dA1 in the first B H T C elements of ws -- observable: held to
    its bar, then the kernel's own tensor feeds dx and dW1; C = 4, 8, 16 keep it in LDS: rounded here at the same place, its spread carried.
    fused = tt_wide_rb_bwd_fused (k_wrb_bwd_fused, C = 16, 32): h1 = ELU(W1 (*) x + b1) is recomputed and rounded to 16 bits inside the kernel
    (not observable: rounded here, its spread carried through W2, through the gate min(h1 + 1, 1) and into dW2), and db1 is summed from the
    ROUNDED dA1 (the centre tap read back from LDS)."""
    s = _rbb_setup(Cc, d, dtype, B, H, T)
    rc, out, what = _rb_backward_call('tt_wide_rb_bwd_fused' if fused else 'tt_wide_rb_bwd', s, Cc, d, dtype, fill, B, H, T, shifts=shifts)
    if rc != 0:
        return rc
    key = 'rb_bwd%s C%d %s' % ('_fused' if fused else '', Cc, _tag(dtype))
    x, dy = C.from_cl(s['x']), C.from_cl(s['dy'])
    if fused:
        hx, a1p, S1, K1 = C.rb_stage1(x, s['w1'].double(), s['b1'].double(), d)
        bar_h = K1 * U * S1 + 3 * U * s['b1'].double().abs().view(1, Cc, 1, 1) + 4 * U * a1p.abs().clamp_min(1.0)
        h1, sph = C.round16(hx, dtype), C.boundary_spread(hx, bar_h, dtype)
    else:
        h1, sph = C.from_cl(s['h1']), None
    W2, b2 = s['w2'].double(), s['b2'].double().view(1, Cc, 1, 1)
    N = B * H * T
    prev = {n: s[n].double() for n in GRADS}
    a2 = torch.einsum('oc,bcht->boht', W2, h1) + b2
    bar_a2 = Cc * U * torch.einsum('oc,bcht->boht', W2.abs(), h1.abs()) + 3 * U * b2.abs()
    if fused:
        bar_a2 = bar_a2 + torch.einsum('oc,bcht->boht', W2.abs(), sph)
    gv = dy * torch.exp(a2).clamp(max=1.0)                       # min(exp, 1) is 1-Lipschitz in a2; __expf to 2u below 1
    bar_gv = dy.abs() * (bar_a2 + 2 * U) + U * gv.abs()
    _hold(key + ' db2', out['db2'], prev['db2'] + gv.sum((0, 2, 3)),
          N * U * gv.abs().sum((0, 2, 3)) + bar_gv.sum((0, 2, 3)) + 3 * U * prev['db2'].abs(), what)
    g16 = C.round16(gv, dtype)
    sp = C.boundary_spread(gv, bar_gv, dtype)
    bar_dw2 = N * U * torch.einsum('boht,bcht->oc', g16.abs(), h1.abs()) + torch.einsum('boht,bcht->oc', sp, h1.abs()) + 3 * U * prev['dw2'].abs()
    if fused:
        bar_dw2 = bar_dw2 + torch.einsum('boht,bcht->oc', g16.abs() + sp, sph)
    _hold(key + ' dw2', out['dw2'], prev['dw2'] + torch.einsum('boht,bcht->oc', g16, h1), bar_dw2, what)
    u = torch.einsum('oc,boht->bcht', W2, g16)
    bar_u = Cc * U * torch.einsum('oc,boht->bcht', W2.abs(), g16.abs()) + torch.einsum('oc,boht->bcht', W2.abs(), sp)
    gate = C.elu_gate(h1)                                        # exact for h1 in +-[0.5, 1]
    a1 = u * gate
    bar_a1 = bar_u * gate + U * a1.abs()
    if fused:                                                    # the gate of a recomputed h1: its own + 1 (<= 2u) and, 1-Lipschitz, the spread of h1
        bar_a1 = bar_a1 + (u.abs() + bar_u) * (sph + 2 * U)
    else:
        _hold(key + ' db1', out['db1'], prev['db1'] + a1.sum((0, 2, 3)),
              N * U * a1.abs().sum((0, 2, 3)) + bar_a1.sum((0, 2, 3)) + 3 * U * prev['db1'].abs(), what)
    geom = dict(KH=3, KW=3, stride_h=1, dil_h=d, dil_w=d, pad_h=d, pad_w=d)
    flip = C.R.dgrad_args('conv', Cc, Cc, 3, 3, 1, d, d, d)
    w1flat = s['w1'].double().reshape(-1)
    if 'da1' in out:
        da1 = C.from_cl(out['da1'])
        _hold16(key + ' dA1', da1, a1, bar_a1, dtype, what)
        carry_w, carry_x = 0.0, 0.0
    else:
        da1 = C.round16(a1, dtype)
        sp1 = C.boundary_spread(a1, bar_a1, dtype)
        carry_w = C.R.conv2d_wgrad(x.abs(), sp1, **geom)[0]
        carry_x = C.R.conv2d(sp1, w1flat.abs(), None, None, Hout=H, **flip)[0]
    if fused:
        _hold(key + ' db1', out['db1'], prev['db1'] + da1.sum((0, 2, 3)),
              N * U * da1.abs().sum((0, 2, 3)) + sp1.sum((0, 2, 3)) + 3 * U * prev['db1'].abs(), what)
    dw1, S, K, _, _ = C.R.conv2d_wgrad(x, da1, **geom)
    bar_dw1 = K.view(1, 1, 3, 3) * U * S + carry_w + 3 * U * prev['dw1'].abs()
    _hold(key + ' dw1', out['dw1'], prev['dw1'] + dw1, bar_dw1, what)
    dx, _, Sx = C.R.conv2d(da1, w1flat, None, dy, Hout=H, **flip)
    beta = Cc * C.R.tap_count(H, H, T, 3, 3, 1, d, d, d, d, 0) * U * Sx + 3 * U * dy.abs() + carry_x
    _hold16(key + ' dx', C.from_cl(out['dx']), dx, beta, dtype, what)
    if onepass:
        # the strips: "dx bit-identical, the fp32 weight / bias gradients equal up to summation order" (include/ttrap.h) -- the same terms, so
        # the same float64 sums and the same bars
        rc1, o1, what1 = _rb_backward_call('tt_wide_rb_bwd_onepass', s, Cc, d, dtype, fill, B, H, T)
        assert rc1 == 0
        assert torch.equal(o1['dx'], out['dx']), what1 + ': dx differs from the per-stage kernels'
        k1 = 'rb_bwd_onepass C%d %s' % (Cc, _tag(dtype))
        _hold(k1 + ' db2', o1['db2'], prev['db2'] + gv.sum((0, 2, 3)),
              N * U * gv.abs().sum((0, 2, 3)) + bar_gv.sum((0, 2, 3)) + 3 * U * prev['db2'].abs(), what1)
        _hold(k1 + ' dw2', o1['dw2'], prev['dw2'] + torch.einsum('boht,bcht->oc', g16, h1),
              N * U * torch.einsum('boht,bcht->oc', g16.abs(), h1.abs()) + torch.einsum('boht,bcht->oc', sp, h1.abs()) + 3 * U * prev['dw2'].abs(),
              what1)
        _hold(k1 + ' db1', o1['db1'], prev['db1'] + a1.sum((0, 2, 3)),
              N * U * a1.abs().sum((0, 2, 3)) + bar_a1.sum((0, 2, 3)) + 3 * U * prev['db1'].abs(), what1)
        _hold(k1 + ' dw1', o1['dw1'], prev['dw1'] + dw1, bar_dw1, what1)
    return 0


@pytest.mark.parametrize('H,T', PLANES)
@pytest.mark.parametrize('d', [1, 2, 3])
@pytest.mark.parametrize('Cc', [4, 8, 16, 32])
@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_residual_block_backward(dtype, Cc, d, H, T, B=2):
    """tt_wide_rb_bwd at every width on all eleven planes, gradients accumulated onto a non-zero pattern, dx written over the guard pattern; on
    C = 16, 32 also tt_wide_rb_bwd_fused against float64 and tt_wide_rb_bwd_onepass: dx equal bit for bit, the four gradients to the same bars."""
    for fill in FILLS:
        assert _rb_backward(Cc, d, dtype, fill, B, H, T, onepass=Cc >= 16 and fill == C.FILL_NAN) == 0
        if Cc >= 16:
            assert _rb_backward(Cc, d, dtype, fill, B, H, T, fused=True) == 0


@pytest.mark.parametrize('d', [1, 2, 3])
@pytest.mark.parametrize('Cc', [4, 8, 16, 32])
@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_residual_block_backward_multitile(dtype, Cc, d, cu_limit, H=17, T=130):
    cu_limit(1)
    assert _rb_backward(Cc, d, dtype, C.FILL_BIG, 2, H, T, onepass=Cc >= 16) == 0
    if Cc >= 16:
        assert _rb_backward(Cc, d, dtype, C.FILL_NAN, 2, H, T, fused=True) == 0


@pytest.mark.parametrize('Cc', [4, 16, 32])
@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_residual_block_backward_one_fp32_pointer_misaligned(dtype, Cc, d=2, H=9, T=66):
    for p in ('w1', 'w2', 'b2') + GRADS:
        assert _rb_backward(Cc, d, dtype, C.FILL_NAN, 2, H, T, shifts={p: 4}) == 0
    if Cc >= 16:
        for p in ('w1', 'b1', 'w2', 'b2') + GRADS:
            assert _rb_backward(Cc, d, dtype, C.FILL_NAN, 2, H, T, shifts={p: 4}, fused=True) == 0


# ---- 10. the level backward: exact equalities, and the gated forms against the plain one ------------------------------------------------
def _level_call(entry, blocks, dils, Cc, dtype, fill, B, H, T, skip=None):
    """One tt_wide_level_bwd* call over ``blocks`` (the _rbb_setup dicts, block 0 first; dy enters the last) -> (rc, outputs)."""
    lib, st = _api(dtype)
    nb = len(blocks)
    A = _arena(fill)
    for i, s in enumerate(blocks):
        for n in ('x', 'h1', 'w1', 'w2', 'b2'):
            A.inp('%s%d' % (n, i), s[n])
        for n in GRADS:
            A.acc('%s%d' % (n, i), s[n])
    A.inp('dy', blocks[-1]['dy'])
    A.out('dx', (B, H, T, Cc), dtype)
    if nb > 1:
        A.scratch('tmp0', B * H * T * Cc * 2)
        A.scratch('tmp1', B * H * T * Cc * 2)
    A.scratch('ws', lib.tt_wide_level_scratch_bytes(nb, B, Cc, H, T))
    if skip is not None:
        A.inp('skip_g', skip['g'])
        A.inp('sw', skip['sw'])
        A.acc('skip_dw', skip['dw'])
    A.build()

    def arr(n):
        return (ctypes.c_void_p * nb)(*[A.ptr('%s%d' % (n, i)) for i in range(nb)])
    d = (ctypes.c_int * nb)(*dils)
    args = [nb, arr('x'), arr('h1'), A.ptr('dy'), arr('w1'), arr('w2'), arr('b2'), A.ptr('dx'), A.ptr('tmp0'), A.ptr('tmp1'), arr('dw1'),
            arr('db1'), arr('dw2'), arr('db2'), A.ptr('ws'), B, Cc, H, T, d]
    if skip is not None:
        args += [A.ptr('skip_g'), skip['g'].size(0), A.ptr('sw'), 1, A.ptr('skip_dw')]
    what = '%s %s C %d dilations %s plane (%d, %d) B %d' % (entry, _tag(dtype), Cc, dils, H, T, B)
    rc = _finish(A, getattr(lib, entry)(*args, st), what)
    out = {}
    if rc == 0:
        out = {'dx': A.get('dx')}
        for i in range(nb):
            for n in GRADS:
                out['%s%d' % (n, i)] = A.get('%s%d' % (n, i))
        if skip is not None:
            out['skip_dw'] = A.get('skip_dw')
    return rc, out, what


LEVEL_DILS = [(1,), (1, 2, 3), (2, 1)]


def _level_case(dtype, Cc, dils, H, T, B=2):
    nb = len(dils)
    blocks = [_rbb_setup(Cc, dils[i], dtype, B, H, T, seed=i) for i in range(nb)]
    e = C.roundoff16(dtype)
    # block by block through tt_wide_rb_bwd, the last block first: every output of the level call is bit-identical (include/ttrap.h)
    g, single = blocks[-1]['dy'], {}
    for i in reversed(range(nb)):
        rc, o, what = _rb_backward_call('tt_wide_rb_bwd', blocks[i], Cc, dils[i], dtype, C.FILL_NAN, B, H, T, dy=g)
        assert rc == 0, what
        for n in GRADS:
            single['%s%d' % (n, i)] = o[n]
        g = o['dx']
    single['dx'] = g
    rc, lev, what = _level_call('tt_wide_level_bwd', blocks, dils, Cc, dtype, C.FILL_BIG, B, H, T)
    assert rc == 0, what
    for n in single:
        assert torch.equal(lev[n], single[n]), '%s: %s differs from the block-by-block calls' % (what, n)
    # gated: dx * ELU'(x[0]); everything else as the plain call
    rc, gat, what = _level_call('tt_wide_level_bwd_gated', blocks, dils, Cc, dtype, C.FILL_NAN, B, H, T)
    assert rc == 0, what
    for n in single:
        if n != 'dx':
            assert torch.equal(gat[n], lev[n]), '%s: %s differs from the plain level call' % (what, n)
    x0 = C.from_cl(blocks[0]['x'])
    gate = C.elu_gate(x0)                                        # exact for x in +-[0.5, 1]
    dx16 = C.from_cl(lev['dx'])
    key = 'level gated C%d %s' % (Cc, _tag(dtype))
    if dils[0] != 1:
        # no gated epilogue at this dilation: the level runs the in-place gate (k_gate_dx, = tt_gate16) on the stored dx -- the product of a
        # 16-bit value and the exact gate fits fp32, so the result is the correctly rounded product, bit for bit
        assert torch.equal(C.from_cl(gat['dx']), C.round16(dx16 * gate, dtype)), what + ': dx is not gate16 of the plain dx'
    else:
        # the gated epilogue multiplies the fp32 sum v, of which the plain call shows the 16-bit rounding: |v - dx16| <= e |v|
        beta = (e * dx16.abs() * (1 + 2 * e) + U * dx16.abs()) * gate
        _hold16(key + ' dx', C.from_cl(gat['dx']), dx16 * gate, beta, dtype, what)
    # the join riding on the gated epilogue
    for reps in (1, 2):
        gen = _gen('skip', Cc, H, T, reps)
        skip = dict(g=C.pm16(gen, dtype, reps, B, H, T, Cc), sw=C.pm32(gen, 3), dw=C.pm32(gen, 3))
        rc, rid, what = _level_call('tt_wide_level_bwd_gated_join', blocks, dils, Cc, dtype, C.FILL_BIG, B, H, T, skip)
        if dils[0] != 1:
            assert rc == UNSUPPORTED, what
            continue
        assert rc == 0, what
        for n in single:
            if n != 'dx':
                assert torch.equal(rid[n], lev[n]), '%s: %s differs from the plain level call' % (what, n)
        t = torch.stack([C.from_cl(skip['g'][r]) for r in range(reps)]).sum(0)          # exact in fp32
        sc = float(skip['sw'][1])
        want = (dx16 + sc * t) * gate
        # v to e |v| as above; sc t, the sum and the product one fp32 rounding each
        beta = (e * dx16.abs() * (1 + 2 * e) + 3 * U * (dx16.abs() + abs(sc) * t.abs())) * gate
        _hold16('level gated_join C%d %s dx' % (Cc, _tag(dtype)), C.from_cl(rid['dx']), want, beta, dtype, what)
        pdw = skip['dw'].double()
        wdw, bar = pdw.clone(), torch.zeros(3, dtype=torch.float64)
        wdw[1] += (t * x0).sum()
        bar[1] = t.numel() * U * (t * x0).abs().sum() + 3 * U * abs(float(pdw[1]))
        _hold('level gated_join C%d %s skip_dw' % (Cc, _tag(dtype)), rid['skip_dw'], wdw, bar, what)


@pytest.mark.parametrize('H,T', [(3, 6), (9, 66), (17, 34)])
@pytest.mark.parametrize('dils', LEVEL_DILS, ids=['d1', 'd123', 'd21'])
@pytest.mark.parametrize('Cc', [4, 8, 16, 32])
@pytest.mark.parametrize('dtype', DTYPES, ids=_tag)
def test_level_backward(dtype, Cc, dils, H, T):
    """tt_wide_level_bwd equals nblocks calls of tt_wide_rb_bwd bit for bit (dx and all 4 nblocks gradients, accumulated onto non-zero
    patterns); _gated and _gated_join (skip_reps 1 and 2) leave every gradient bit-identical to the plain call and dx within a derived bar of
    the plain dx times ELU'(x[0]) (+ the join's share) -- exactly gate16 of it where the first dilation has no gated epilogue; _gated_join
    at dilations (2, 1): TT_E_UNSUPPORTED, nothing written."""
    _level_case(dtype, Cc, dils, H, T)
