"""
The split-operand ("x3") kernels of csrc/conv_x3.hip called through the C ABI of include/ttrap.h, every element held to a derived rounding
bound against the float64 restatements of tests/x3_ref.py (pinned against torch by tests/test_x3_restatement.py).  The models are
tests/test_gpu_conv_parity.py and tests/test_gpu_cl16_parity.py; the bars and their derivation are in the docstring of tests/x3_ref.py
(the pair: max(2^-23 |v|, 2^-36); a three-term product sum: prod_bar; ELU, ELU', the adds as in the fp32 file).

Arena (cl16_ref.Arena).  Every operand of a call -- x3 tensors, fp32 planar tensors, weights, biases, scale, gradients, scratch of exactly
the size the *_scratch_bytes function of that call returns -- is a window of ONE byte buffer with 128 bytes of guard around it.  in:
bit-unchanged afterwards; out: the guard pattern before, every element written and finite afterwards; acc: a non-zero pattern before (the
+= contract of dw1 / db1 / dw2 / db2); scratch: anything inside, nothing behind.  Every case runs with both guard fills (0xFF: NaN in
fp16 and fp32; 0x46: 6.27 / 12689.6, which a halo misread cannot hide from an ELU).  A refused call leaves the whole buffer untouched.

Operands.  An x3 tensor handed to a kernel is made on the host (x3_ref.to_x3) and the restatement takes the values its pairs hold
(x3_ref.from_x3): exactly known, no input-side split term.  What the kernels split themselves -- weights, fp32 planar inputs, the latent
vector -- comes in two kinds: 'exact' (x3_ref.exact_pairs: 22 significant bits, held exactly by a pair, so the split terms vanish and a
lost cross term or lo plane, 2^-11 relative per product, is far outside the bar) and 'general' (uniform in +-[0.5, 1], weights times
1 / sqrt(K), one split term 2^-23 S per such operand).  Intermediates: h1 of tt_x3_rb_fwd_train and g1 at the head of ws of tt_x3_rb_bwd
are stored -- held to their own bars, then the kernel's own tensor feeds the next stage of the restatement; h1 of tt_x3_rb_fwd /
tt_x3n_rb_fwd is not observable -- its pair's bar is carried through |W2|.  No element is excluded anywhere.

Index arithmetic, read from the code (what the planes below are chosen against):
    k_x3_pack / _unpack     one thread per 8 channels of one pixel, ``pix >= npix`` guard; flat pixel -> (b, h t) by division: B = 2, 3 with
                            H T = 1, 2, 6, 12 puts the 256-thread blocks and the division across rows and clips.
    k_x3_conv               tile 6 x 32 (C = 32, 4 waves: 2 column groups x 2 row groups of R = 3 rows) / 8 x 64 (C = 16, 8 waves: 4 x 2, R = 4);
                            halo D staged by LDS-DMA piece by piece, ``ok`` = p < NP and (h, t) inside the image, else the zero piece; a
                            wave whose rows start below the image skips (h0 + r0 >= H), rows stop at h >= H, columns are masked by
                            ``valid`` = t < T only at the stores; persistent walk v += gridDim.x through xcd_order.  Planes smaller than
                            the halo (H <= d, T <= d) make every tap but the centre read zero pieces; T = 15 / 16 / 17 moves the edge of the
                            16-column group; one tile +-1 row / column makes a second tile of one row / column.
    k_x3n_conv              tile 16 x 64, 4 waves x 4 rows walked R = 2 at a time; a matrix column holds S = 16 / C pixels 16 apart
                            (span 32 at C = 8, 64 at C = 4); PIN stages by 4-byte loads with the offset clamped to 0 where not ok, else
                            LDS-DMA with the zero piece; stores masked by t >= T and h >= H.
    k_x3_sconv / _sconv8    no LDS for activations: a wave = 16 frames (t clamped to T - 1 for loads, stores masked by tv), rows outside
                            the input read row 0 and are zeroed; the unit loop runs rch rows per workgroup with a sliding window.
    k_x3_latenc / _latdec   a workgroup = 128 frames (t clamped, stores masked); E steps double-buffered through LDS; the extra input
                            channel of the decode is one fma per output.
    k_x3_absmax / _scale_fin  min(ceil(n / 256), 1024) blocks, grid-stride; the partials in ws, reduced by one block.
    k_x3_bwd_a              one wave per group of 16 consecutive FLAT pixels (``pix < npix`` on loads and the g1 store; invalid lanes carry
                            zeros into the sums); groups straddle rows and clips whenever H T is no multiple of 16.
    k_x3_wgrad              tile 4 x 64 (C = 32) / 8 x 64 (C = 16) + halo D by LDS-DMA under ``ok``; K = 32 pixels per product.
    k_x3_reduce             fixed-order sum of the dumps, ``*dst += s * scale[1]``; dump regions sized by the shape (XBW), not by the grid.
No access outside an operand's window at any of the planes below follows from these guards; the guard bands check it.

Alignment, (entry point, pointer) by what the code issues, read from the kernels; a pointer that needs 16 bytes is
refused with TT_E_BADARG before anything is launched (asserted here with the buffer untouched; such a call is never launched):
    16-byte LDS-DMA         x of tt_x3_rb_fwd / _fwd_train / _level_fwd (x3_in) / tt_x3n_rb_fwd (x3n); both halves of ws of the two level
                            entries; x and the g1 region (head of ws) of tt_x3_rb_bwd (k_x3_wgrad, k_x3_conv MODE 2); the weight image
                            in ws of the latent heads
    16-byte vector access   out of pack, in of unpack; y / h1 / dx as x3 at C = 32; h1 and dy of tt_x3_rb_bwd at C = 32 (k_x3_bwd_a and the
                            MODE 2 epilogue); x3 inputs and outputs of the strided pair (8 bytes at the C = 8 -> 16 output) and of the
                            latent heads; the x3n output at C = 4
    8-byte vector access    the same tensors at C = 16 (e16x4) and the x3n output at C = 8: asked 16 bytes all the same, one rule
    4-byte access           every fp32 planar tensor, w1 / b1 / w2 / b2 / w / bias, scale, dw1 / db1 / dw2 / db2, z, and dy / scale / ws of
                            tt_x3_grad_scale; the dump regions of ws of tt_x3_rb_bwd (behind the 256-byte rounded g1 region).  One float
                            off a 16-byte boundary, ONE pointer per call, with the same bars: x / scale / y of pack and unpack; dy / scale /
                            ws of tt_x3_grad_scale; w1 / b1 / w2 / b2 / planar y of the block forward; w1 / w2 / b2 / scale / planar dx / the
                            four gradients of the block backward; planar x / y and the weights of tt_x3n_rb_fwd; x / w / b / planar y of the
                            strided pair in all three kernels (k_x3_sconv, k_x3_sconv8, the transposed form); w / bias / z of both latent
                            heads and the planar y of the decode; planar x / y and one block's w1 / b1 / w2 / b2 of the two level entries.
The Python layer (framework/ops/x3.py; level16.py has no x3 call) allocates every x3 tensor and every ws as a whole torch.empty (512-byte
aligned by the caching allocator); the only views are the two halves of ws in the instrumented path, split at a multiple of 256 bytes.

Changed in conv_x3.hip with this file (host side only; no kernel changed):
    no entry point of the family tested a pointer (ptrs_aligned was never called): the refusals of the table above were added.
    tt_x3_level_fwd in place (x3_in with y == x) was refused for nblocks == 1 only -- with two or more blocks the last one reads a half
    of ws, so the call was accepted and computed a correct level.  The contract now refuses it at every nblocks, before the first
    launch (test_level_refusals, nb = 1 and 2); the Python layer never calls in place.  A change of contract, not a defect.
No kernel defect showed.

Range.  test_block_forward_range pokes one value beyond 65504 into the x3 input of the wide block (hi = inf): non-finite in the 3 x 3
dilated field of that pixel, finite and in-bar everywhere else.  Not asserted for the narrow C = 8 kernel: there a matrix column holds two
pixels 16 columns apart and the weights are block-diagonal, so 0 x inf makes the partner pixel non-finite too -- read from k_x3n_conv;
still non-finite, never finite and wrong, which is what the header promises.

Worst ratios to the bar measured on an MI355X (177 tests, 8 s for the file, no test above 0.4 s), per family and output:
    pack -> unpack              1.000: the bar IS the pair's half-ulp bound max(2^-23 |v|, 2^-36), which correctly rounded splits of tens of
                                thousands of values reach (tests/test_x3_restatement.py shows the same on the CPU); pack and unpack themselves:
                                bit-exact, scaled forms included
    tt_x3_grad_scale            bit-exact in every case
    tt_x3_rb_fwd                y planar 0.022, y x3 0.031      tt_x3_rb_fwd_train   h1 0.058, y 0.119, y x3 0.151
    tt_x3_rb_bwd                g1 (ws) 0.031, dx planar 0.240, dx x3 0.451, dw1 0.434, db1 0.019, dw2 0.052, db2 0.036; the three dx forms
                                give bit-identical gradients, dx as x3 == split(planar dx * S), scaled dy: bit-identical after rescaling
    level entries               bit-identical to block-by-block calls (wide: all four x3_in / x3_out forms; narrow)
    tt_x3n_rb_fwd               C = 4: planar 0.087, x3n 0.107; C = 8: 0.055 / 0.103
    tt_x3_sconv_fwd             C = 8: planar 0.035, x3 0.056; C = 16: 0.019 / 0.022; C = 32: 0.008 / 0.010
    tt_x3_tconv_fwd             C = 16: 0.138 / 0.130; C = 32: 0.128 / 0.121
    latent heads                encode 0.033 (32, 32), 0.017 (64, 128); decode planar / x3 0.043 / 0.058 and 0.011 / 0.013
    one fp32 pointer off        every pair listed in the alignment table above met the same bars; every x3 / ws pointer off 16 bytes was refused with
                                the buffer untouched
(The bars are dominated by the worst-case terms 2^-22 S and n 2^-23 S, which random signs never add up to: hence ratios well below 1 everywhere but at the pair itself.)

Broken on purpose in scratch copies of conv_x3.hip, ONE library per break, nothing moved outside the arena; each library ran this file
(the *refusals tests left out) and, but for the one noted, the kernel-level tests of tests/test_gpu_x3.py and tests/test_gpu_x3_train.py
(routing and model cases left out):
    cross term             ``Wlo xhi`` of the 3x3 product of k_x3_conv dropped: 37 here -- test_block_forward 12 of 12, _multitile 2, _misaligned
                           2, _range 3, test_block_backward 12 of 12 (dx), its multitile / misaligned / scale cases 6.  Old files: 58 failures.
    halo column            the first halo column of k_x3_conv's staging read one column to the right: 32 here -- test_block_forward 12,
                           test_block_backward 12, the multitile cases 4, misaligned backward 2, _range 2.  Old files: 48.
    ragged edge            ``valid = t <= T`` in k_x3_conv: 41 here -- the guard band behind y / h1 / dx written (the 128 bytes of one C = 32 pixel
                           stay inside the arena's guard) or the next row's first pixel overwritten: test_block_forward 12, test_block_backward
                           12, their multitile / misaligned / scale / range cases 13, test_level_forward_is_block_by_block 4.  Old files: NOT
                           run -- behind an ordinary torch allocation that store can leave mapped memory; by reading, their T = 70 and
                           T = 33 planes overwrite the first pixel of the next row before it is written or after (a race between tiles),
                           and the last row's store lands in allocator slack.
    reduce stores          ``*dst =`` in k_x3_reduce: 18 here -- every test_block_backward case (12), multitile 2, misaligned 2, scale 2.
                           Old files: NOT noticed, 125 of 125 passed (they accumulate onto zeros).
    1 / S left off         db2 in k_x3_reduce: the same 18 here.  Old files: 33.
    mirrored tap           ``8 - k`` -> ``k`` in MODE 2 (both weight reads): the same 18 here (dx).  Old files: 32.
    npix tail              lanes of k_x3_bwd_a's last group past npix read the last pixel instead of zeros: the same 18 here (dw2, db1, db2
                           on every plane whose pixel count is no multiple of 16).  Old files: 20.
    narrow block           the lo plane of W2 lost in k_x3n_conv: test_narrow_block_forward 12 of 12.  Old files: 28.
    strided pair           k_x3_sconv takes the bias of the neighbouring channel: test_sconv 12 (C = 16, 32; C = 8 has its own kernel),
                           test_tconv 18.  Old files: 20.
    latent heads           the extra input channel of the decode always takes ``fill``: test_latent_heads 24 of 24.  Old files: 9.
"""

import ctypes
import math
import zlib

import pytest
import torch

import x3_ref as X

pytestmark = pytest.mark.gpu

U = X.U
BADARG, UNSUPPORTED = -1, -2
F16, F32 = torch.float16, torch.float32
FILLS = [X.FILL_NAN, X.FILL_BIG]
KINDS = ['exact', 'general']


def _api():
    from timbre_trap import _hip
    return _hip.lib(), _hip.stream_ptr()


_worst = {}


def _note(key, ratio):
    _worst[key] = max(_worst.get(key, 0.0), ratio)
    print('ratio to bar: %-40s %.3f (worst so far %.3f)' % (key, ratio, _worst[key]))


def _hold(key, got, want, bar, what=''):
    bar = bar + torch.zeros_like(want)
    e = (got.double() - want).abs()
    assert bool(torch.isfinite(e).all()), '%s %s: non-finite' % (key, what)
    r = torch.where(e > 0, e / bar.clamp_min(1e-300), torch.zeros_like(e)).reshape(-1)
    ratio = float(r.max()) if e.numel() else 0.0
    _note(key, ratio)
    if not bool((e <= bar).all()):
        i = int(r.argmax())
        raise AssertionError('%s %s: %.3f of the bar at element %d (wanted %.9g, off by %.3e; %d of %d elements over)' % (
            key, what, ratio, i, float(want.reshape(-1)[i]), float(e.reshape(-1)[i]), int((e > bar).sum()), e.numel()))


def _biteq(a, b):
    w = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(w), b.contiguous().view(w))


def _gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


def _arena(fill):
    return X.Arena(fill, 'cuda')


def _finish(A, rc, what):
    if rc != 0:
        A.untouched(what + ' (refused with %d)' % rc)
        return rc
    A.verify(what)
    return 0


@pytest.fixture
def cu_limit():
    """Cap the CU count the persistent grids are sized with; restored afterwards."""
    lib, _ = _api()
    prev = lib.tt_set_cu_limit(0)
    yield lib.tt_set_cu_limit
    lib.tt_set_cu_limit(prev)


def _wgen(kind):
    return X.exact_pairs if kind == 'exact' else X.general


def _params(gen, Cn, kind):
    f = _wgen(kind)
    return (f(gen, Cn, Cn, 3, 3, scale=1 / math.sqrt(9 * Cn)), X.general(gen, Cn, scale=0.3),
            f(gen, Cn, Cn, 1, 1, scale=1 / math.sqrt(Cn)), X.general(gen, Cn, scale=0.3))


def _acc_pattern(gen, shape, mag=1.0):
    return X.general(gen, *shape) * mag


# the planes of the issue: smaller than halo and tile, T = 15 / 16 / 17, B H T no multiple of 16
SMALL = [(2, 1, 1), (3, 1, 2), (2, 2, 3), (3, 3, 4), (2, 2, 15), (1, 3, 16), (2, 2, 17)]
TILE = {32: [(1, 6, 32), (2, 5, 31), (1, 7, 33)], 16: [(1, 8, 64), (2, 7, 63), (1, 9, 65)], 8: [(1, 16, 64), (2, 15, 63), (1, 17, 65)],
        4: [(1, 16, 64), (2, 15, 63), (1, 17, 65)]}


def _planes(Cn):
    return SMALL + TILE[Cn]


# ---- 1. pack, unpack, gradient scale ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,H,T', SMALL + [(2, 7, 33)])
@pytest.mark.parametrize('Cn', [16, 32, 64])
def test_pack_unpack(Cn, B, H, T):
    """Bit for bit: the split is restated exactly, the join is exact.  Values span the normal range, fp16's subnormal range (|v| < 2^-14), zeros
    and the last binade below 65504; the scaled forms with S = 2^20 on values of 1e-7."""
    lib, st = _api()
    g = _gen('pack', Cn, H, T)
    x = X.general(g, B, Cn, H, T)
    x.view(-1)[::5] *= 2.0 ** -15
    x.view(-1)[1::7] *= 2.0 ** -22
    x.view(-1)[2::11] *= 40000
    x.view(-1)[3::13] = 0.0
    for fill in FILLS:
        for sc, xx in ((None, x), ((2.0 ** 20, 2.0 ** -20), x * 1e-7)):
            for off in (None, 'x', 'y') + (('scale',) if sc else ()):      # one fp32 pointer one float off a 16-byte boundary, in turn
                A = _arena(fill)
                A.inp('x', xx, 4 if off == 'x' else 0)
                A.inp('t', X.pack(xx, sc))
                if sc:
                    A.inp('scale', torch.tensor(sc, dtype=F32), 4 if off == 'scale' else 0)
                A.out('out', (B, H, T, 2, Cn), F16)
                A.out('y', (B, Cn, H, T), F32, 4 if off == 'y' else 0)
                A.build()
                what = 'pack / unpack C %d (%d, %d, %d) scale %s, misaligned: %s' % (Cn, B, H, T, sc, off)
                if sc:
                    rc = lib.tt_x3_pack_scaled(A.ptr('x'), A.ptr('out'), A.ptr('scale'), B, Cn, H, T, st)
                    rc = rc or lib.tt_x3_unpack_scaled(A.ptr('t'), A.ptr('y'), A.ptr('scale'), B, Cn, H, T, st)
                else:
                    rc = lib.tt_x3_pack(A.ptr('x'), A.ptr('out'), B, Cn, H, T, st) or lib.tt_x3_unpack(A.ptr('t'), A.ptr('y'), B, Cn, H, T, st)
                assert _finish(A, rc, what) == 0
                assert _biteq(A.get('out'), X.pack(xx, sc)), what
                assert _biteq(A.get('y'), X.unpack(X.pack(xx, sc), sc)), what
                if not sc:
                    _hold('pack -> unpack', A.get('y'), xx.double(), X.pair_err(xx.double()), what)


def test_pack_unpack_refusals():
    lib, st = _api()
    B, Cn, H, T = 1, 16, 2, 3
    x = X.general(_gen('packref'), B, Cn, H, T)
    for off in (2, 8):
        A = _arena(X.FILL_BIG)
        A.inp('x', x)
        A.inp('t', X.pack(x), off)
        A.out('out', (B, H, T, 2, Cn), F16, off)
        A.out('y', (B, Cn, H, T), F32)
        A.build()
        assert lib.tt_x3_pack(A.ptr('x'), A.ptr('out'), B, Cn, H, T, st) == BADARG
        assert lib.tt_x3_unpack(A.ptr('t'), A.ptr('y'), B, Cn, H, T, st) == BADARG
        assert lib.tt_x3_pack(A.ptr('x'), A.ptr('out', 0), B, 8, H, T, st) == BADARG          # a width without the layout
        A.untouched('pack / unpack off by %d' % off)


def _grad_scale(fill, dy, off=None):
    """off: which of dy / scale / ws is one float off a 16-byte boundary."""
    lib, st = _api()
    A = _arena(fill)
    A.inp('dy', dy, 4 if off == 'dy' else 0)
    A.out('scale', (2,), F32, 4 if off == 'scale' else 0)
    A.scratch('ws', lib.tt_x3_grad_scale_scratch_bytes(), 4 if off == 'ws' else 0)
    A.build()
    rc = lib.tt_x3_grad_scale(A.ptr('dy'), dy.numel(), A.ptr('scale'), A.ptr('ws'), st)
    assert _finish(A, rc, 'tt_x3_grad_scale n = %d' % dy.numel()) == 0
    return tuple(float(v) for v in A.get('scale'))


@pytest.mark.parametrize('n', [1, 255, 256, 257, 1024 * 256 - 1, 1024 * 256, 1024 * 256 + 1, 2 * 1024 * 256 + 3])
def test_grad_scale_lengths_and_positions(n):
    """S bit-exact for the abs-max in the first, a middle and the last element; n around 256 (one block) and around 1024 x 256, where the
    grid stops growing and the loop strides."""
    g = _gen('gs', n)
    for pos in sorted({0, n // 2, n - 1}):
        for fill in FILLS:
            dy = X.general(g, n) * 1e-9
            dy[pos] = -3.1e-6
            assert _grad_scale(fill, dy) == X.grad_scale(dy) == (2.0 ** 27, 2.0 ** -27), (n, pos)
    for off in ('dy', 'scale', 'ws'):
        assert _grad_scale(X.FILL_BIG, dy, off) == (2.0 ** 27, 2.0 ** -27), (n, off)


@pytest.mark.parametrize('amax', [1.0, 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23, 2.0 - 2.0 ** -23, 256.0, 511.9, 512.0, 2.0 ** -20, 2.0 ** -126, 2.0 ** -127,
                                  2.0 ** -149, 2.0 ** -112, 2.0 ** -111, 3.4e38, 2.0 ** 127, 0.0, float('inf'), float('nan')])
def test_grad_scale_values(amax):
    dy = torch.zeros(300, dtype=F32)
    if amax and math.isfinite(amax):
        dy[:] = min(amax, 1.0) * 0.25
    dy[123] = -amax
    want = X.grad_scale(dy)
    assert _grad_scale(X.FILL_NAN, dy) == want and _grad_scale(X.FILL_BIG, dy) == want, amax


# ---- 2. the wide block, forward --------------------------------------------------------------------------------------------------------
def _rb_fwd(fill, Cn, B, H, T, d, kind, shifts=None, x_special=None):
    """tt_x3_rb_fwd with planar and with x3 output and tt_x3_rb_fwd_train, in one arena.  -> (rc, results)."""
    lib, st = _api()
    shifts = shifts or {}
    g = _gen('rbfwd', Cn, B, H, T, d, kind)
    x32 = X.general(g, B, Cn, H, T)
    if x_special is not None:
        x_special(x32)
    xs = X.to_x3(x32)
    w1, b1, w2, b2 = _params(g, Cn, kind)
    A = _arena(fill)
    A.inp('x', xs, shifts.get('x', 0))
    for n_, v in (('w1', w1), ('b1', b1), ('w2', w2), ('b2', b2)):
        A.inp(n_, v, shifts.get(n_, 0))
    A.out('ypl', (B, Cn, H, T), F32, shifts.get('ypl', 0))
    A.out('yx3', (B, H, T, 2, Cn), F16, shifts.get('yx3', 0))
    A.out('yt', (B, H, T, 2, Cn), F16)
    A.out('ytp', (B, Cn, H, T), F32, shifts.get('ypl', 0))
    A.out('h1', (B, H, T, 2, Cn), F16, shifts.get('h1', 0))
    A.out('h1b', (B, H, T, 2, Cn), F16)
    A.build()
    P = A.ptr
    what = 'rb_fwd C %d (%d, %d, %d) d %d %s' % (Cn, B, H, T, d, kind)
    rcs = [lib.tt_x3_rb_fwd(P('x'), P('w1'), P('b1'), P('w2'), P('b2'), P('ypl'), 1, B, Cn, H, T, d, st),
           lib.tt_x3_rb_fwd(P('x'), P('w1'), P('b1'), P('w2'), P('b2'), P('yx3'), 0, B, Cn, H, T, d, st),
           lib.tt_x3_rb_fwd_train(P('x'), P('w1'), P('b1'), P('w2'), P('b2'), P('yt'), 0, P('h1'), B, Cn, H, T, d, st),
           lib.tt_x3_rb_fwd_train(P('x'), P('w1'), P('b1'), P('w2'), P('b2'), P('ytp'), 1, P('h1b'), B, Cn, H, T, d, st)]
    if any(rcs):
        A.untouched(what + ' (refused %s)' % rcs)
        return rcs, None
    A.verify(what, finite=x_special is None)             # the range case: guards, inputs and "written" all the same
    return rcs, dict(A=A, x=X.from_x3(xs), p=(w1, b1, w2, b2), what=what, **{k: A.get(k) for k in ('ypl', 'yx3', 'yt', 'ytp', 'h1', 'h1b')})


def _check_rb_fwd(r, d, kind, mask=None):
    ns = 0 if kind == 'exact' else 1
    x, (w1, b1, w2, b2), what = r['x'], r['p'], r['what']
    sel = (lambda t: t) if mask is None else (lambda t: (t + torch.zeros_like(x))[mask])
    # x3 and planar output: equal bit for bit before the split
    if mask is None:
        assert _biteq(r['yx3'], X.to_x3(r['ypl'])), what + ': x3 output != split(planar output)'
        assert _biteq(r['yt'], X.to_x3(r['ytp'])) and _biteq(r['h1'], r['h1b']), what + ': training forward, x3 vs planar'
    y, by = X.rb_fwd(x, w1, b1, w2, b2, d, 0, ns)
    _hold('rb_fwd y planar', sel(r['ypl'].double()), sel(y), sel(by), what)
    _hold('rb_fwd y x3', sel(X.from_x3(r['yx3'])), sel(y), sel(X.stored(y, by)), what)
    h1, _, bh = X.rb_stage1(x, w1, b1, d, ns)
    _hold('rb_fwd_train h1', sel(X.from_x3(r['h1'])), sel(h1), sel(X.stored(h1, bh)), what)
    if mask is None:
        y2, _, by2 = X.rb_stage2(X.from_x3(r['h1']), x, w2, b2, None, ns)
        _hold('rb_fwd_train y', r['ytp'].double(), y2, by2, what)
        _hold('rb_fwd_train y x3', X.from_x3(r['yt']), y2, X.stored(y2, by2), what)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('d', [1, 2, 3])
@pytest.mark.parametrize('Cn', [16, 32])
def test_block_forward(Cn, d, kind):
    for B, H, T in _planes(Cn):
        for fill in FILLS:
            rcs, r = _rb_fwd(fill, Cn, B, H, T, d, kind)
            assert rcs == [0, 0, 0, 0]
            _check_rb_fwd(r, d, kind)


@pytest.mark.parametrize('Cn,B,H,T', [(32, 1, 17, 94), (16, 1, 23, 190)])
def test_block_forward_multitile(cu_limit, Cn, B, H, T):
    """3 x 3 tiles on one CU's worth of workgroups (2): every workgroup walks four or five tiles of the persistent loop."""
    cu_limit(1)
    for d in (1, 3):
        rcs, r = _rb_fwd(X.FILL_NAN, Cn, B, H, T, d, 'exact')
        assert rcs == [0, 0, 0, 0]
        _check_rb_fwd(r, d, 'exact')


@pytest.mark.parametrize('Cn', [16, 32])
def test_block_forward_one_fp32_pointer_misaligned(Cn):
    B, H, T = TILE[Cn][1]
    for name in ('w1', 'b1', 'w2', 'b2', 'ypl'):
        rcs, r = _rb_fwd(X.FILL_BIG, Cn, B, H, T, 2, 'general', {name: 4})
        assert rcs == [0, 0, 0, 0], name
        _check_rb_fwd(r, 2, 'general')


@pytest.mark.parametrize('Cn', [16, 32])
def test_block_forward_refusals(Cn):
    lib, st = _api()
    for off in (2, 8):
        assert _rb_fwd(X.FILL_BIG, Cn, 1, 2, 3, 1, 'general', {'x': off})[0] == [BADARG] * 4
    g = _gen('rbref', Cn)
    B, H, T = 1, 2, 3
    xs = X.to_x3(X.general(g, B, Cn, H, T))
    w1, b1, w2, b2 = _params(g, Cn, 'general')
    for off in (2, 8):
        A = _arena(X.FILL_BIG)
        A.inp('x', xs)
        for n_, v in (('w1', w1), ('b1', b1), ('w2', w2), ('b2', b2)):
            A.inp(n_, v)
        A.out('y', (B, H, T, 2, Cn), F16)
        A.out('yo', (B, H, T, 2, Cn), F16, off)
        A.out('h1', (B, H, T, 2, Cn), F16)
        A.out('h1o', (B, H, T, 2, Cn), F16, off)
        A.build()
        P = A.ptr
        W = (P('w1'), P('b1'), P('w2'), P('b2'))
        assert lib.tt_x3_rb_fwd(P('x'), *W, P('yo'), 0, B, Cn, H, T, 1, st) == BADARG
        assert lib.tt_x3_rb_fwd_train(P('x'), *W, P('yo'), 0, P('h1'), B, Cn, H, T, 1, st) == BADARG
        assert lib.tt_x3_rb_fwd_train(P('x'), *W, P('y'), 0, P('h1o'), B, Cn, H, T, 1, st) == BADARG
        assert lib.tt_x3_rb_fwd_train(P('x'), *W, P('y'), 1, P('h1o'), B, Cn, H, T, 1, st) == BADARG
        assert lib.tt_x3_rb_fwd(P('x'), *W, P('x'), 0, B, Cn, H, T, 1, st) == BADARG               # y == x
        assert lib.tt_x3_rb_fwd_train(P('x'), *W, P('y'), 0, P('y'), B, Cn, H, T, 1, st) == BADARG   # h1 == y
        assert lib.tt_x3_rb_fwd(P('x'), *W, P('y'), 0, B, Cn, H, T, 4, st) == UNSUPPORTED          # dilation
        assert lib.tt_x3_rb_fwd(P('x'), *W, P('y'), 0, B, 8, H, T, 1, st) == BADARG                # width
        assert lib.tt_x3_rb_fwd(P('x'), None, P('b1'), P('w2'), P('b2'), P('y'), 0, B, Cn, H, T, 1, st) == BADARG
        A.untouched('rb_fwd refusals')


@pytest.mark.parametrize('Cn,d', [(16, 1), (16, 3), (32, 2)])
def test_block_forward_range(Cn, d):
    """One value beyond 65504 in one pixel: hi = inf.  Non-finite results in its receptive field (the taps of the 3x3 that reach it; the 1x1
    and the residual stay on the pixel), finite and in-bar results everywhere else on the plane."""
    B, H, T = 1, 9, 40
    hp, tp = 4, 21

    def poke(x32):
        x32[0, 3, hp, tp] = 1.0e5
    for fill in FILLS:
        rcs, r = _rb_fwd(fill, Cn, B, H, T, d, 'general', x_special=poke)
        assert rcs == [0, 0, 0, 0]
        field = torch.zeros(B, Cn, H, T, dtype=torch.bool)
        for kh in (-d, 0, d):
            for kw in (-d, 0, d):
                if 0 <= hp + kh < H and 0 <= tp + kw < T:
                    field[:, :, hp + kh, tp + kw] = True
        for k in ('ypl', 'ytp'):
            fin = torch.isfinite(r[k])
            assert not bool(fin[field].any()), r['what'] + ': finite inside the receptive field of an out-of-range value'
            assert bool(fin[~field].all()), r['what'] + ': non-finite outside the receptive field'
        # the restatement on the plane with the value replaced: identical outside the field
        r['x'][0, 3, hp, tp] = 0.0
        _check_rb_fwd(r, d, 'general', mask=~field)


# ---- 3. the wide block, backward -------------------------------------------------------------------------------------------------------
def _rb_bwd(fill, Cn, B, H, T, d, kind, shifts=None, dy_scale=1.0):
    lib, st = _api()
    shifts = shifts or {}
    g = _gen('rbbwd', Cn, B, H, T, d, kind)
    xs, hs = X.to_x3(X.general(g, B, Cn, H, T)), X.to_x3(X.general(g, B, Cn, H, T))
    dy32 = X.general(g, B, Cn, H, T) * dy_scale
    w1, _, w2, b2 = _params(g, Cn, kind)
    sc = X.grad_scale(dy32)
    dys = X.pack(dy32, sc)
    prev = {n_: _acc_pattern(g, s) * dy_scale for n_, s in (('dw1', (Cn, Cn, 3, 3)), ('db1', (Cn,)), ('dw2', (Cn, Cn, 1, 1)), ('db2', (Cn,)))}
    nws = lib.tt_x3_rb_bwd_scratch_bytes(B, Cn, H, T)
    A = _arena(fill)
    for n_, v in (('x', xs), ('h1', hs), ('dy', dys)):
        A.inp(n_, v, shifts.get(n_, 0))
    for n_, v in (('w1', w1), ('w2', w2), ('b2', b2), ('scale', torch.tensor(sc, dtype=F32))):
        A.inp(n_, v, shifts.get(n_, 0))
    A.out('dxp', (B, Cn, H, T), F32, shifts.get('dxp', 0))
    A.out('dxs', (B, H, T, 2, Cn), F16, shifts.get('dxs', 0))
    A.inp('dxn', torch.full((B, Cn, H, T), 7.0, dtype=F32))               # the dx of the call that passes NULL: must stay as it is
    for k in ('a', 'b', 'c'):
        for n_ in prev:
            A.acc(n_ + k, prev[n_], shifts.get(n_, 0) if k == 'a' else 0)
    A.scratch('ws', nws, shifts.get('ws', 0))
    A.build()
    P = A.ptr
    what = 'rb_bwd C %d (%d, %d, %d) d %d %s dy x %g' % (Cn, B, H, T, d, kind, dy_scale)
    call = lambda dx, planar, k: lib.tt_x3_rb_bwd(P('x'), P('h1'), P('dy'), P('w1'), P('w2'), P('b2'), dx, planar, P('dw1' + k), P('db1' + k),
                                                  P('dw2' + k), P('db2' + k), P('scale'), P('ws'), B, Cn, H, T, d, st)
    rc = call(P('dxp'), 1, 'a')
    if rc:
        A.untouched(what + ' (refused with %d)' % rc)
        return rc, None
    torch.cuda.synchronize()
    g1 = A.get('ws')[:B * H * T * Cn * 4].view(F16).view(B, H, T, 2, Cn).clone()
    assert call(P('dxs'), 0, 'b') == 0 and call(None, 0, 'c') == 0
    A.verify(what)
    res = dict(what=what, x=X.from_x3(xs), h1=X.from_x3(hs), dy=X.from_x3(dys), S=sc[0], p=(w1, w2, b2), prev=prev, g1=g1,
               dxp=A.get('dxp'), dxs=A.get('dxs'))
    for k in ('a', 'b', 'c'):
        for n_ in prev:
            res[n_ + k] = A.get(n_ + k)
    return 0, res


def _check_rb_bwd(r, d, kind):
    ns = 0 if kind == 'exact' else 1
    what, S = r['what'], r['S']
    w1, w2, b2 = r['p']
    Cn = w2.size(0)
    # the three calls: the same four gradients bit for bit (dx planar, dx as x3, dx = NULL)
    for n_ in r['prev']:
        assert _biteq(r[n_ + 'a'], r[n_ + 'b']) and _biteq(r[n_ + 'a'], r[n_ + 'c']), what + ': %s differs between the dx forms' % n_
    # dx planar (times 1 / S) and dx as x3 (carrying S): the same value before the split, S a power of two
    assert _biteq(r['dxs'], X.to_x3((r['dxp'].double() * S).float())), what + ': dx as x3 != split(planar dx * S)'
    assert _biteq(X.unpack(r['dxs'], (S, 1.0 / S)), (X.from_x3(r['dxs']) / S).float())
    own = X.rb_bwd(r['x'], r['h1'], r['dy'], w1, w2, b2, d, None, ns)
    g1v, bg1 = own['g1']
    fin = bool(torch.isfinite(r['g1'].float()).all())
    assert fin, what + ': g1 in ws not finite'
    _hold('rb_bwd g1 (ws)', X.from_x3(r['g1']) / S, g1v / S, X.stored(g1v, bg1) / S, what)
    out = X.rb_bwd(r['x'], r['h1'], r['dy'], w1, w2, b2, d, X.from_x3(r['g1']), ns)
    _hold('rb_bwd dx planar', r['dxp'].double(), out['dx'][0] / S, out['dx'][1] / S, what)
    _hold('rb_bwd dx x3', X.from_x3(r['dxs']) / S, out['dx'][0] / S, X.stored(*out['dx']) / S, what)
    for n_ in ('dw1', 'db1', 'dw2', 'db2'):
        prev = r['prev'][n_].double()
        want = prev + (out[n_][0] / S).reshape(prev.shape)
        bar = (out[n_][1] / S).reshape(prev.shape) + U * (prev.abs() + want.abs())
        _hold('rb_bwd ' + n_, r[n_ + 'a'].double(), want, bar, what)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('d', [1, 2, 3])
@pytest.mark.parametrize('Cn', [16, 32])
def test_block_backward(Cn, d, kind):
    for B, H, T in _planes(Cn):
        for fill in FILLS:
            rc, r = _rb_bwd(fill, Cn, B, H, T, d, kind)
            assert rc == 0
            _check_rb_bwd(r, d, kind)


@pytest.mark.parametrize('Cn,B,H,T', [(32, 1, 17, 94), (16, 1, 23, 190)])
def test_block_backward_multitile(cu_limit, Cn, B, H, T):
    cu_limit(1)
    for d in (1, 3):
        rc, r = _rb_bwd(X.FILL_NAN, Cn, B, H, T, d, 'exact')
        assert rc == 0
        _check_rb_bwd(r, d, 'exact')


@pytest.mark.parametrize('Cn', [16, 32])
def test_block_backward_scale_never_shows(Cn):
    """dy times 2^-30 and 2^10 (and the previous content of the gradients with it): the x3 form of dy is the same bits, S differs, and every
    gradient and dx equal the unscaled ones bit for bit after the power of two is taken out."""
    B, H, T = TILE[Cn][1]
    _, base = _rb_bwd(X.FILL_NAN, Cn, B, H, T, 2, 'general')
    _check_rb_bwd(base, 2, 'general')
    for k in (-30, 10):
        rc, r = _rb_bwd(X.FILL_NAN, Cn, B, H, T, 2, 'general', dy_scale=2.0 ** k)
        assert rc == 0 and r['S'] == base['S'] * 2.0 ** -k
        assert _biteq(r['dxs'], base['dxs']) and _biteq(r['g1'], base['g1'])
        for n_ in ('dxp', 'dw1a', 'db1a', 'dw2a', 'db2a'):
            assert _biteq(r[n_], base[n_] * 2.0 ** k), '%s at 2^%d' % (n_, k)


@pytest.mark.parametrize('Cn', [16, 32])
def test_block_backward_one_fp32_pointer_misaligned(Cn):
    B, H, T = TILE[Cn][1]
    for name in ('w1', 'w2', 'b2', 'scale', 'dxp', 'dw1', 'db1', 'dw2', 'db2'):
        rc, r = _rb_bwd(X.FILL_BIG, Cn, B, H, T, 1, 'general', {name: 4})
        assert rc == 0, name
        _check_rb_bwd(r, 1, 'general')


@pytest.mark.parametrize('Cn', [16, 32])
def test_block_backward_refusals(Cn):
    lib, st = _api()
    for name in ('x', 'h1', 'dy', 'ws'):
        for off in (8,) if name != 'ws' else (4, 8):
            rc, _ = _rb_bwd(X.FILL_BIG, Cn, 1, 2, 3, 1, 'general', {name: off})
            assert rc == BADARG, (name, off)
    g = _gen('bwdref', Cn)
    B, H, T = 1, 2, 3
    xs = X.to_x3(X.general(g, B, Cn, H, T))
    w1, _, w2, b2 = _params(g, Cn, 'general')
    A = _arena(X.FILL_BIG)
    for n_ in ('x', 'h1', 'dy'):
        A.inp(n_, xs)
    for n_, v in (('w1', w1), ('w2', w2), ('b2', b2), ('scale', torch.tensor([1.0, 1.0]))):
        A.inp(n_, v)
    A.out('dxo', (B, H, T, 2, Cn), F16, 8)
    for n_, s in (('dw1', (Cn, Cn, 3, 3)), ('db1', (Cn,)), ('dw2', (Cn, Cn)), ('db2', (Cn,))):
        A.acc(n_, torch.ones(s))
    A.scratch('ws', lib.tt_x3_rb_bwd_scratch_bytes(B, Cn, H, T))
    A.build()
    P = A.ptr
    G = (P('dw1'), P('db1'), P('dw2'), P('db2'), P('scale'), P('ws'))
    assert lib.tt_x3_rb_bwd(P('x'), P('h1'), P('dy'), P('w1'), P('w2'), P('b2'), P('dxo'), 0, *G, B, Cn, H, T, 1, st) == BADARG
    assert lib.tt_x3_rb_bwd(P('x'), P('h1'), P('dy'), P('w1'), P('w2'), P('b2'), P('dy'), 0, *G, B, Cn, H, T, 1, st) == BADARG      # dx == dy
    assert lib.tt_x3_rb_bwd(P('x'), P('h1'), P('dy'), P('w1'), P('w2'), P('b2'), None, 0, *G, B, Cn, H, T, 4, st) == BADARG         # dilation
    assert lib.tt_x3_rb_bwd(P('x'), P('h1'), P('dy'), P('w1'), P('w2'), P('b2'), None, 0, *G, B, 8, H, T, 1, st) == BADARG          # width
    assert lib.tt_x3_rb_bwd(P('x'), P('h1'), P('dy'), P('w1'), P('w2'), P('b2'), None, 0, P('dw1'), P('db1'), P('dw2'), P('db2'), None, P('ws'),
                            B, Cn, H, T, 1, st) == BADARG                                                                         # scale
    assert lib.tt_x3_rb_bwd_scratch_bytes(B, 8, H, T) == -1
    A.untouched('rb_bwd refusals')


# ---- 4. the level entries --------------------------------------------------------------------------------------------------------------
def _ptr_array(A, names):
    return (ctypes.c_void_p * len(names))(*[A.ptr(n_).value for n_ in names])


@pytest.mark.parametrize('B,H,T', [(2, 2, 3), (1, 9, 65)])
@pytest.mark.parametrize('Cn', [16, 32])
def test_level_forward_is_block_by_block(Cn, B, H, T, nb=3):
    """tt_x3_level_fwd over all four x3_in / x3_out combinations: bit-equal to tt_x3_pack + nb calls of tt_x3_rb_fwd (held by the block tests)."""
    lib, st = _api()
    g = _gen('level', Cn, B, H, T)
    x32 = X.general(g, B, Cn, H, T)
    ps = [_params(g, Cn, 'general') for _ in range(nb)]
    dil = [1, 2, 3]
    # both fills; then one fp32 pointer one float off a 16-byte boundary in turn: planar x, planar y, the second block's weights and biases
    for fill, off in [(f, None) for f in FILLS] + [(X.FILL_BIG, o) for o in ('xp', 'yp', 'w1_1', 'b1_1', 'w2_1', 'b2_1')]:
        A = _arena(fill)
        A.inp('xp', x32, 4 if off == 'xp' else 0)
        A.inp('xs', X.to_x3(x32))
        for i, p in enumerate(ps):
            for n_, v in zip(('w1', 'b1', 'w2', 'b2'), p):
                A.inp('%s_%d' % (n_, i), v, 4 if off == '%s_%d' % (n_, i) else 0)
        for k in ('00', '01', '10', '11'):
            A.out('y' + k, (B, H, T, 2, Cn) if k[1] == '1' else (B, Cn, H, T), F16 if k[1] == '1' else F32, 4 if off == 'yp' and k[1] == '0' else 0)
        A.out('t0', (B, H, T, 2, Cn), F16)
        A.out('t1', (B, H, T, 2, Cn), F16)
        A.out('rp', (B, Cn, H, T), F32)
        A.out('rs', (B, H, T, 2, Cn), F16)
        A.scratch('ws', lib.tt_x3_level_scratch_bytes(B, Cn, H, T))
        A.build()
        P = A.ptr
        arrs = [_ptr_array(A, ['%s_%d' % (n_, i) for i in range(nb)]) for n_ in ('w1', 'b1', 'w2', 'b2')]
        da = (ctypes.c_int * nb)(*dil)
        for k in ('00', '01', '10', '11'):
            assert lib.tt_x3_level_fwd(nb, P('xs') if k[0] == '1' else P('xp'), int(k[0]), P('y' + k), int(k[1]), *arrs, da, P('ws'), B, Cn, H, T, st) == 0
        W = lambda i: tuple(P('%s_%d' % (n_, i)) for n_ in ('w1', 'b1', 'w2', 'b2'))
        assert lib.tt_x3_rb_fwd(P('xs'), *W(0), P('t0'), 0, B, Cn, H, T, dil[0], st) == 0
        assert lib.tt_x3_rb_fwd(P('t0'), *W(1), P('t1'), 0, B, Cn, H, T, dil[1], st) == 0
        assert lib.tt_x3_rb_fwd(P('t1'), *W(2), P('rp'), 1, B, Cn, H, T, dil[2], st) == 0
        assert lib.tt_x3_rb_fwd(P('t1'), *W(2), P('rs'), 0, B, Cn, H, T, dil[2], st) == 0
        A.verify('tt_x3_level_fwd')
        for k in ('00', '01', '10', '11'):
            assert _biteq(A.get('y' + k), A.get('rs' if k[1] == '1' else 'rp')), 'level x3_in %s x3_out %s, misaligned: %s' % (k[0], k[1], off)


def test_level_refusals():
    lib, st = _api()
    B, Cn, H, T, nb = 1, 16, 2, 3, 2
    g = _gen('levelref')
    x32 = X.general(g, B, Cn, H, T)
    p = _params(g, Cn, 'general')
    for ws_off, xs_off in ((0, 0), (8, 0), (0, 8)):
        A = _arena(X.FILL_BIG)
        A.inp('xp', x32)
        A.acc('xs', X.to_x3(x32), xs_off)                 # x3_in with y == x: x is also the output, so not an 'in' window
        for n_, v in zip(('w1', 'b1', 'w2', 'b2'), p):
            A.inp(n_, v)
        A.out('y', (B, H, T, 2, Cn), F16)
        A.out('yo', (B, H, T, 2, Cn), F16, 8)
        A.scratch('ws', lib.tt_x3_level_scratch_bytes(B, Cn, H, T), ws_off)
        A.build()
        P = A.ptr
        arrs = [_ptr_array(A, [n_] * nb) for n_ in ('w1', 'b1', 'w2', 'b2')]
        da, bad = (ctypes.c_int * nb)(1, 2), (ctypes.c_int * nb)(1, 4)
        if ws_off or xs_off:
            assert lib.tt_x3_level_fwd(nb, P('xs'), 1, P('y'), 1, *arrs, da, P('ws'), B, Cn, H, T, st) == BADARG
        else:
            for n in (1, 2):                                 # in place: refused at every nblocks, before anything is launched
                assert lib.tt_x3_level_fwd(n, P('xs'), 1, P('xs'), 1, *arrs, da, P('ws'), B, Cn, H, T, st) == BADARG
                assert lib.tt_x3_level_fwd(n, P('xs'), 1, P('xs'), 0, *arrs, da, P('ws'), B, Cn, H, T, st) == BADARG
            assert lib.tt_x3_level_fwd(nb, P('xp'), 0, P('yo'), 1, *arrs, da, P('ws'), B, Cn, H, T, st) == BADARG
            assert lib.tt_x3_level_fwd(nb, P('xp'), 0, P('y'), 1, *arrs, bad, P('ws'), B, Cn, H, T, st) == BADARG
            assert lib.tt_x3_level_fwd(0, P('xp'), 0, P('y'), 1, *arrs, da, P('ws'), B, Cn, H, T, st) == BADARG
            assert lib.tt_x3_level_fwd(nb, P('xp'), 0, P('y'), 1, *arrs, da, None, B, Cn, H, T, st) == BADARG
            assert lib.tt_x3_level_fwd(nb, P('xp'), 0, P('y'), 1, *arrs, da, P('ws'), B, 8, H, T, st) == BADARG
            assert lib.tt_x3n_level_fwd(nb, P('xp'), P('y'), *arrs, da, P('ws'), B, 16, H, T, st) == BADARG
        assert lib.tt_x3_level_scratch_bytes(B, 8, H, T) == -1 and lib.tt_x3n_level_scratch_bytes(B, 16, H, T) == -1
        A.untouched('level refusals')


@pytest.mark.parametrize('Cn', [4, 8])
def test_narrow_level_refusals(Cn, B=1, H=2, T=3, nb=2):
    """ws of tt_x3n_level_fwd holds the x3n tensors between the blocks (LDS-DMA): off its 16 bytes it is refused with nothing touched."""
    lib, st = _api()
    g = _gen('nlevelref', Cn)
    x32 = X.general(g, B, Cn, H, T)
    p = _params(g, Cn, 'general')
    for ws_off in (4, 8):
        A = _arena(X.FILL_BIG)
        A.inp('x', x32)
        for n_, v in zip(('w1', 'b1', 'w2', 'b2'), p):
            A.inp(n_, v)
        A.out('y', (B, Cn, H, T), F32)
        A.scratch('ws', lib.tt_x3n_level_scratch_bytes(B, Cn, H, T), ws_off)
        A.build()
        P = A.ptr
        arrs = [_ptr_array(A, [n_] * nb) for n_ in ('w1', 'b1', 'w2', 'b2')]
        da = (ctypes.c_int * nb)(1, 2)
        assert lib.tt_x3n_level_fwd(nb, P('x'), P('y'), *arrs, da, P('ws'), B, Cn, H, T, st) == BADARG
        assert lib.tt_x3n_level_fwd(3, P('x'), P('y'), *[_ptr_array(A, [n_] * 3) for n_ in ('w1', 'b1', 'w2', 'b2')], (ctypes.c_int * 3)(1, 2, 3),
                                    P('ws'), B, Cn, H, T, st) == BADARG
        A.untouched('tt_x3n_level_fwd, ws off by %d' % ws_off)


# ---- 5. the narrow block and level -----------------------------------------------------------------------------------------------------
def _x3n(fill, Cn, B, H, T, d, kind, shifts=None, calls=('00', '01', '10', '11')):
    """tt_x3n_rb_fwd over the four planar_in / planar_out combinations (``calls``: which of them) in one arena."""
    lib, st = _api()
    shifts = shifts or {}
    g = _gen('x3n', Cn, B, H, T, d, kind)
    xp = _wgen(kind)(g, B, Cn, H, T)                     # the planar input is split by the kernel
    xs = X.to_x3(X.general(g, B, Cn, H, T))
    w1, b1, w2, b2 = _params(g, Cn, kind)
    A = _arena(fill)
    A.inp('xp', xp, shifts.get('xp', 0))
    A.inp('xs', xs, shifts.get('xs', 0))
    for n_, v in (('w1', w1), ('b1', b1), ('w2', w2), ('b2', b2)):
        A.inp(n_, v, shifts.get(n_, 0))
    for k in calls:                                      # planar_in, planar_out
        A.out('y' + k, (B, Cn, H, T) if k[1] == '1' else (B, H, T, 2, Cn), F32 if k[1] == '1' else F16,
              shifts.get('yp' if k[1] == '1' else 'ys', 0))
    A.build()
    P = A.ptr
    what = 'x3n_rb_fwd C %d (%d, %d, %d) d %d %s' % (Cn, B, H, T, d, kind)
    rcs = [lib.tt_x3n_rb_fwd(P('xp') if k[0] == '1' else P('xs'), int(k[0]), P('w1'), P('b1'), P('w2'), P('b2'), P('y' + k), int(k[1]), B, Cn, H, T, d, st)
           for k in calls]
    if any(rcs):
        A.untouched(what + ' refused %s' % rcs)
        return rcs
    A.verify(what)
    ns = 0 if kind == 'exact' else 1
    for k in calls:
        x = xp.double() if k[0] == '1' else X.from_x3(xs)
        y, by = X.rb_fwd(x, w1, b1, w2, b2, d, ns if k[0] == '1' else 0, ns)
        if k[1] == '1':
            _hold('x3n_rb_fwd C %d planar out' % Cn, A.get('y' + k).double(), y, by, what + ' ' + k)
        else:
            _hold('x3n_rb_fwd C %d x3n out' % Cn, X.from_x3(A.get('y' + k)), y, X.stored(y, by), what + ' ' + k)
    if len(calls) == 4:
        assert _biteq(A.get('y00'), X.to_x3(A.get('y01'))) and _biteq(A.get('y10'), X.to_x3(A.get('y11'))), what + ': x3n output != split(planar output)'
    return rcs


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('d', [1, 2, 3])
@pytest.mark.parametrize('Cn', [4, 8])
def test_narrow_block_forward(Cn, d, kind):
    for B, H, T in _planes(Cn):
        for fill in FILLS:
            assert _x3n(fill, Cn, B, H, T, d, kind) == [0, 0, 0, 0]


@pytest.mark.parametrize('Cn', [4, 8])
def test_narrow_block_multitile_misaligned_and_refusals(cu_limit, Cn):
    for name in ('xp', 'w1', 'b1', 'w2', 'b2', 'yp'):
        assert _x3n(X.FILL_BIG, Cn, 2, 15, 63, 2, 'general', {name: 4}) == [0, 0, 0, 0], name
    assert _x3n(X.FILL_BIG, Cn, 1, 2, 3, 1, 'general', {'xs': 8}, calls=('00', '01')) == [BADARG, BADARG]
    assert _x3n(X.FILL_BIG, Cn, 1, 2, 3, 1, 'general', {'ys': 8}, calls=('00', '10')) == [BADARG, BADARG]
    # 4 x 3 tiles of 16 x 64 on one CU's worth of workgroups -- 4 at C = 4, 3 at C = 8 (launch_x3n: per_cu; the LDS of D = 3 allows 6 / 3):
    # workgroup w takes tiles w, w + grid, ...: three tiles each at C = 4, four each at C = 8 (xcd_order is the identity at 12 tiles)
    cu_limit(1)
    assert _x3n(X.FILL_NAN, Cn, 1, 63, 190, 3, 'exact') == [0, 0, 0, 0]


@pytest.mark.parametrize('Cn', [4, 8])
def test_narrow_level_is_block_by_block(Cn, B=2, H=5, T=17, nb=3):
    lib, st = _api()
    g = _gen('nlevel', Cn)
    x32 = X.general(g, B, Cn, H, T)
    ps = [_params(g, Cn, 'general') for _ in range(nb)]
    dil = [1, 2, 3]
    for fill, off in [(f, None) for f in FILLS] + [(X.FILL_BIG, o) for o in ('x', 'y', 'w1_1', 'b1_1', 'w2_1', 'b2_1')]:
        A = _arena(fill)
        A.inp('x', x32, 4 if off == 'x' else 0)
        for i, p in enumerate(ps):
            for n_, v in zip(('w1', 'b1', 'w2', 'b2'), p):
                A.inp('%s_%d' % (n_, i), v, 4 if off == '%s_%d' % (n_, i) else 0)
        A.out('y', (B, Cn, H, T), F32, 4 if off == 'y' else 0)
        A.out('r', (B, Cn, H, T), F32)
        A.out('t0', (B, H, T, 2, Cn), F16)
        A.out('t1', (B, H, T, 2, Cn), F16)
        A.scratch('ws', lib.tt_x3n_level_scratch_bytes(B, Cn, H, T))
        A.build()
        P = A.ptr
        arrs = [_ptr_array(A, ['%s_%d' % (n_, i) for i in range(nb)]) for n_ in ('w1', 'b1', 'w2', 'b2')]
        assert lib.tt_x3n_level_fwd(nb, P('x'), P('y'), *arrs, (ctypes.c_int * nb)(*dil), P('ws'), B, Cn, H, T, st) == 0
        W = lambda i: tuple(P('%s_%d' % (n_, i)) for n_ in ('w1', 'b1', 'w2', 'b2'))
        assert lib.tt_x3n_rb_fwd(P('x'), 1, *W(0), P('t0'), 0, B, Cn, H, T, dil[0], st) == 0
        assert lib.tt_x3n_rb_fwd(P('t0'), 0, *W(1), P('t1'), 0, B, Cn, H, T, dil[1], st) == 0
        assert lib.tt_x3n_rb_fwd(P('t1'), 0, *W(2), P('r'), 1, B, Cn, H, T, dil[2], st) == 0
        A.verify('tt_x3n_level_fwd')
        assert _biteq(A.get('y'), A.get('r')), 'narrow level, misaligned: %s' % off


# ---- 6. the strided pair ---------------------------------------------------------------------------------------------------------------
def _stride(fill, layer, Cn, pin, B, H, T, kind, out_pad=0, shifts=None, calls=('p', 's')):
    lib, st = _api()
    shifts = shifts or {}
    g = _gen(layer, Cn, pin, B, H, T, kind, out_pad)
    Cin, Cout = (Cn, 2 * Cn) if layer == 'sconv' else (2 * Cn, Cn)
    Hout = (H - 4) // 2 + 1 if layer == 'sconv' else 2 * H + 2 + out_pad
    xp = _wgen(kind)(g, B, Cin, H, T)
    xin = xp if pin else X.to_x3(xp)
    xv = xp.double() if pin else X.from_x3(xin)
    w = _wgen(kind)(g, 2 * Cn, Cn, 4, 1, scale=1 / math.sqrt((4 if layer == 'sconv' else 2) * Cin))
    b = X.general(g, Cout, scale=0.3)
    A = _arena(fill)
    A.inp('x', xin, shifts.get('x', 0))
    A.inp('w', w, shifts.get('w', 0))
    A.inp('b', b, shifts.get('b', 0))
    A.out('yp', (B, Cout, Hout, T), F32, shifts.get('yp', 0))
    A.out('ys', (B, Hout, T, 2, Cout), F16, shifts.get('ys', 0))
    A.build()
    P = A.ptr
    what = '%s C %d pin %d (%d, %d, %d) out_pad %d %s' % (layer, Cn, pin, B, H, T, out_pad, kind)
    if layer == 'sconv':
        rcs = [lib.tt_x3_sconv_fwd(P('x'), int(pin), P('w'), P('b'), P('y' + k), int(k == 'p'), B, Cn, H, T, st) for k in calls]
    else:
        rcs = [lib.tt_x3_tconv_fwd(P('x'), int(pin), P('w'), P('b'), P('y' + k), int(k == 'p'), B, Cn, H, T, out_pad, st) for k in calls]
    if any(rcs):
        A.untouched(what + ' refused %s' % rcs)
        return rcs
    A.verify(what)
    ns = 0 if kind == 'exact' else (2 if pin else 1)
    y, v, beta = X.stride_fwd(layer, Cn, xv, w, b, out_pad, ns)
    _hold('%s C %d planar out' % (layer, Cn), A.get('yp').double(), y, beta, what)
    _hold('%s C %d x3 out' % (layer, Cn), X.from_x3(A.get('ys')), y, X.stored(y, beta), what)
    assert _biteq(A.get('ys'), X.to_x3(A.get('yp'))), what + ': x3 output != split(planar output)'
    return rcs


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('T', [1, 15, 17])
@pytest.mark.parametrize('Cn,pin', [(16, 0), (32, 0), (8, 1)])
def test_sconv(Cn, pin, T, kind):
    for H in (4, 5, 6, 11):
        for fill in FILLS:
            assert _stride(fill, 'sconv', Cn, pin, 2, H, T, kind) == [0, 0]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('T', [1, 15, 17])
@pytest.mark.parametrize('Cn,pin', [(16, 0), (32, 0), (32, 1)])
def test_tconv(Cn, pin, T, kind):
    for H in (1, 2):
        for op in (0, 1):
            for fill in FILLS:
                assert _stride(fill, 'tconv', Cn, pin, 2, H, T, kind, op) == [0, 0]


def test_strided_pair_long_runs_misaligned_and_refusals(cu_limit):
    lib, st = _api()
    for name in ('w', 'b', 'yp'):                        # k_x3_sconv (down, up from x3, up from planar) and k_x3_sconv8
        assert _stride(X.FILL_BIG, 'sconv', 16, 0, 2, 6, 17, 'general', shifts={name: 4}) == [0, 0], name
        assert _stride(X.FILL_BIG, 'sconv', 8, 1, 2, 6, 17, 'general', shifts={name: 4}) == [0, 0], name
        assert _stride(X.FILL_BIG, 'tconv', 16, 0, 2, 2, 17, 'general', 1, shifts={name: 4}) == [0, 0], name
        assert _stride(X.FILL_BIG, 'tconv', 32, 1, 2, 2, 17, 'general', 1, shifts={name: 4}) == [0, 0], name
    assert _stride(X.FILL_BIG, 'sconv', 8, 1, 2, 6, 17, 'general', shifts={'x': 4}) == [0, 0]
    assert _stride(X.FILL_BIG, 'tconv', 32, 1, 2, 2, 17, 'general', shifts={'x': 4}) == [0, 0]
    for layer, Cn, H in (('sconv', 16, 6), ('tconv', 16, 2)):
        assert _stride(X.FILL_BIG, layer, Cn, 0, 1, H, 3, 'general', shifts={'x': 8}) == [BADARG, BADARG]
        assert _stride(X.FILL_BIG, layer, Cn, 0, 1, H, 3, 'general', shifts={'ys': 8}, calls=('s',)) == [BADARG]
    assert _stride(X.FILL_BIG, 'sconv', 16, 0, 1, 3, 3, 'general') == [BADARG, BADARG]             # H < 4
    assert _stride(X.FILL_BIG, 'sconv', 16, 1, 1, 6, 3, 'general') == [UNSUPPORTED, UNSUPPORTED]   # planar input only at C = 8
    assert _stride(X.FILL_BIG, 'sconv', 8, 0, 1, 6, 3, 'general') == [UNSUPPORTED, UNSUPPORTED]    # x3 input only at C = 16, 32
    assert _stride(X.FILL_BIG, 'tconv', 16, 1, 1, 2, 3, 'general') == [UNSUPPORTED, UNSUPPORTED]   # planar input only at C = 32
    assert _stride(X.FILL_BIG, 'tconv', 8, 0, 1, 2, 3, 'general') == [UNSUPPORTED, UNSUPPORTED]
    assert _stride(X.FILL_BIG, 'tconv', 16, 0, 1, 2, 3, 'general', out_pad=2) == [BADARG, BADARG]
    cu_limit(1)                                          # one CU: runs of many rows per workgroup, the sliding window at work
    assert _stride(X.FILL_NAN, 'sconv', 32, 0, 1, 41, 70, 'exact') == [0, 0]
    assert _stride(X.FILL_NAN, 'sconv', 8, 1, 1, 41, 70, 'exact') == [0, 0]
    assert _stride(X.FILL_NAN, 'tconv', 16, 0, 1, 19, 70, 'exact', 1) == [0, 0]


# ---- 7. the latent heads ---------------------------------------------------------------------------------------------------------------
def _latent(fill, Cn, D, E, B, T, kind, bias, shifts=None, ws_shift=0, calls=('enc', '1p', '1s', '0p', '0s')):
    lib, st = _api()
    shifts = shifts or {}
    g = _gen('lat', Cn, D, E, T, kind, bias)
    xs = X.to_x3(X.general(g, B, Cn, E, T))                 # (B, E, T, 2, C)
    we = _wgen(kind)(g, D, Cn, E, 1, scale=1 / math.sqrt(Cn * E))
    be = X.general(g, D, scale=0.3) if bias else None
    wd = _wgen(kind)(g, D + 1, Cn, E, 1, scale=1 / math.sqrt(D))
    bd = X.general(g, Cn, scale=0.3) if bias else None
    zz = _wgen(kind)(g, B, D + 1, T)
    nws = lib.tt_x3_latent_scratch_bytes(Cn, E, D)
    assert nws > 0
    fillv = 0.75
    A = _arena(fill)
    A.inp('x', xs, shifts.get('x', 0))
    A.inp('we', we, shifts.get('we', 0))
    A.inp('wd', wd, shifts.get('wd', 0))
    if bias:
        A.inp('be', be, shifts.get('be', 0))
        A.inp('bd', bd, shifts.get('bd', 0))
    A.inp('z1', zz, shifts.get('z', 0))
    A.inp('z0', zz[:, :D].contiguous(), shifts.get('z', 0))
    A.out('z', (B, D, T), F32, shifts.get('zo', 0))
    for k in ('1p', '1s', '0p', '0s'):
        A.out('y' + k, (B, Cn, E, T) if k[1] == 'p' else (B, E, T, 2, Cn), F32 if k[1] == 'p' else F16, shifts.get('y' + k[1], 0))
    A.scratch('ws', nws, ws_shift)
    A.build()
    P = A.ptr
    what = 'latent C %d D %d E %d (%d, %d) %s bias %s' % (Cn, D, E, B, T, kind, bias)
    rcs = [lib.tt_x3_latent_encode(P('x'), P('we'), P('be'), P('z'), P('ws'), B, Cn, E, D, T, st)] if 'enc' in calls else []
    for k in calls:
        if k == 'enc':
            continue
        Dz = D + 1 if k[0] == '1' else D
        rcs.append(lib.tt_x3_latent_decode(P('z' + k[0]), Dz, fillv, P('wd'), P('bd'), P('y' + k), int(k[1] == 'p'), P('ws'), B, Cn, E, D, T, st))
    if any(rcs):
        A.untouched(what + ' refused %s' % rcs)
        return rcs
    A.verify(what)
    ns = 0 if kind == 'exact' else 1
    z, bz = X.lat_encode(X.from_x3(xs), we, be, ns)
    _hold('latent_encode (%d, %d)' % (Cn, D), A.get('z').double(), z, bz, what)
    for k in ('1', '0'):
        Dz = D + 1 if k == '1' else D
        y, v, by = X.lat_decode(zz[:, :Dz], Dz, fillv, wd, bd, 2 * ns)
        _hold('latent_decode (%d, %d) planar' % (Cn, D), A.get('y' + k + 'p').double(), y, by, what + ' Dz %d' % Dz)
        _hold('latent_decode (%d, %d) x3' % (Cn, D), X.from_x3(A.get('y' + k + 's')), y, X.stored(y, by), what + ' Dz %d' % Dz)
        assert _biteq(A.get('y' + k + 's'), X.to_x3(A.get('y' + k + 'p'))), what + ': x3 output != split(planar output)'
    return rcs


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('bias', [True, False])
@pytest.mark.parametrize('Cn,D,E', [(64, 128, 1), (64, 128, 3), (64, 128, 31), (32, 32, 1), (32, 32, 3), (32, 32, 31)])
def test_latent_heads(Cn, D, E, bias, kind):
    """E = 31: the model's own (540 bins through four strided layers: 540 -> 269 -> 133 -> 65 -> 31, Encoder.__init__); ws is exactly
    tt_x3_latent_scratch_bytes."""
    for T in (1, 15, 17, 33):
        for fill in FILLS:
            assert _latent(fill, Cn, D, E, 2, T, kind, bias) == [0] * 5


def test_latent_heads_many_frames_misaligned_and_refusals():
    lib, st = _api()
    assert _latent(X.FILL_NAN, 32, 32, 3, 2, 131, 'exact', True) == [0] * 5       # two workgroups per clip, the second ragged
    for name in ('we', 'wd', 'be', 'bd', 'z', 'zo', 'yp'):
        assert _latent(X.FILL_BIG, 32, 32, 3, 2, 17, 'general', True, {name: 4}) == [0] * 5, name
    assert _latent(X.FILL_BIG, 32, 32, 3, 1, 5, 'general', True, {'x': 8}, calls=('enc',)) == [BADARG]
    assert _latent(X.FILL_BIG, 32, 32, 3, 1, 5, 'general', True, {'ys': 8}, calls=('1s', '0s')) == [BADARG, BADARG]
    assert _latent(X.FILL_BIG, 32, 32, 3, 1, 5, 'general', True, ws_shift=8) == [BADARG] * 5
    assert lib.tt_x3_latent_scratch_bytes(32, 3, 64) == -1 and lib.tt_x3_latent_scratch_bytes(16, 3, 32) == -1
    assert lib.tt_x3_latent_scratch_bytes(32, 0, 32) == -1
    # the 160 KB of LDS: E C 4 + 2 (D / 32) (C / 16) 2048 bytes; (64, 128) leaves 96 KB = 384 rows
    g = _gen('latlds')
    for Cn, D, E in ((64, 128, 385), (32, 32, 1217)):
        A = _arena(X.FILL_BIG)
        A.inp('z', X.general(g, 1, D + 1, 2))
        A.inp('w', X.general(g, D + 1, Cn, E, 1))
        A.out('y', (1, Cn, E, 2), F32)
        A.scratch('ws', lib.tt_x3_latent_scratch_bytes(Cn, E, D))
        A.build()
        assert lib.tt_x3_latent_decode(A.ptr('z'), D + 1, 0.0, A.ptr('w'), None, A.ptr('y'), 1, A.ptr('ws'), 1, Cn, E, D, 2, st) == UNSUPPORTED
        assert lib.tt_x3_latent_decode(A.ptr('z'), D + 2, 0.0, A.ptr('w'), None, A.ptr('y'), 1, A.ptr('ws'), 1, Cn, E, D, 2, st) == BADARG
        assert lib.tt_x3_latent_decode(A.ptr('z'), D + 1, 0.0, A.ptr('w'), None, A.ptr('y'), 1, A.ptr('ws'), 1, Cn, E, D + 32, 2, st) != 0
        A.untouched('latent decode LDS refusal')
