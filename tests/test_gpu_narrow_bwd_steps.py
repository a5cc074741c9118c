"""
GPU checks of phase 1 and the tile staging of k_nrb_bwd_fused (csrc/conv_wide_bf16.hip) where they take a path of their own: the steps of
phase 1 that hold only halo pixels run the pointwise chain without the sums (db1, db2, dW2), and interior tiles are staged with a scalar
base and 32-bit lane offsets.

Through the C ABI (tt_wide_rb_bwd, tt_wide_level_bwd_gated, tt_wide_level_bwd_gated_join), C = 4 and 8, dilation 1, 2, 3 plain, dilation 1
gated and riding, bf16 and fp16, at three shapes (the tile is 16 rows x 64 frames):
    (1, 5, 8)      the image is smaller than the halo: one border tile, every halo-only step wholly outside the image
    (2, 17, 66)    one tile boundary on each axis: halo-only steps of one tile hold real pixels of its neighbour, the last row and the
                   last two frames are a partial tile
    (1, 40, 136)   the smallest image with an interior tile (h0 = 16, t0 = 64): the scalar-base staging next to border tiles
dx, dW1, db1, dW2, db2 against the float64 restatement with the kernel's roundings of tests/test_gpu_bwd_loops.py (its code, run at these
shapes) at that file's bars, and every output bit-identical between two calls.

One non-finite case: an inf in dy at a pixel that one tile owns and that lies in a halo-only step of the tile above must reach db2 and
dW2 as it reaches the restatement's -- the skipped sums of the upper tile must not be what carried it.
"""

import pytest
import torch
import torch.nn.functional as F

import test_gpu_bwd_loops as base
from test_gpu_bwd_loops import _unit_loss_scale  # noqa: F401  (autouse: the weight-gradient reduces divide by the thread's loss scale)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5, 8), (2, 17, 66), (1, 40, 136)]
FORMS = [(1, 'plain'), (2, 'plain'), (3, 'plain'), (1, 'gated'), (1, 'riding')]
GRAD_SHAPES = lambda C: ((C, C, 3, 3), (C,), (C, C, 1, 1), (C,))

_CASES = {}


def _case(C, d, elt, shape):
    """base._case (inputs, the kernel's own forward, the float64 restatement) at one of this file's shapes; computed once, never modified.
    base._case takes its shape from base.SHAPES[C] and keeps its results in base._CASES: both are exchanged for the call and put back."""
    key = (C, d, elt, shape)
    if key not in _CASES:
        saved = base.SHAPES, base._CASES
        base.SHAPES, base._CASES = {C: shape}, {}
        try:
            _CASES[key] = base._case(C, d, elt)
        finally:
            base.SHAPES, base._CASES = saved
    return _CASES[key]


def _run(c, C, d, form, gb=None):
    """one call of the form's entry point: (dx, [dW1, db1, dW2, db2] on top of 0.5, the skip weights' gradient or None)"""
    from timbre_trap._hip import check, ptr, stream_ptr
    lib, st, B, H, T = c['lib'], stream_ptr(), c['B'], c['H'], c['T']
    dx = torch.empty((B, H, T, C), dtype=c['ELT'], device='cuda')
    grads = [torch.full(s, 0.5, dtype=torch.float32, device='cuda') for s in GRAD_SHAPES(C)]
    ds = None
    cc = dict(c, gb=gb) if gb is not None else c
    if form == 'plain':
        ws = torch.zeros(lib.tt_wide_scratch_bytes(B, C, H, T), dtype=torch.uint8, device='cuda')
        check(lib.tt_wide_rb_bwd(ptr(cc['xb']), ptr(cc['hb']), ptr(cc['gb']), ptr(cc['w1d']), ptr(cc['w2d']), ptr(cc['b2d']), ptr(dx), ptr(grads[0]),
                                 ptr(grads[1]), ptr(grads[2]), ptr(grads[3]), ptr(ws), B, C, H, T, d, st), 'bwd')
    else:
        ws = torch.zeros(lib.tt_wide_level_scratch_bytes(1, B, C, H, T), dtype=torch.uint8, device='cuda')
        args = base._level_args(cc, C, d, dx, grads, ws)
        if form == 'gated':
            check(lib.tt_wide_level_bwd_gated(*args, st), 'level gated')
        else:
            ds = torch.full((5,), 3.0, device='cuda')
            rc = lib.tt_wide_level_bwd_gated_join(*args, ptr(c['sgb']), 2, ptr(c['sw']), 3, ptr(ds), st)
            assert rc == 0, 'the narrow widths have a riding form (rc %d)' % rc
    torch.cuda.synchronize()
    return dx, grads, ds


def _riding_operands(c, C):
    """the join's gradient (two batches) and the skip weights, once per case"""
    if 'sgb' not in c:
        from timbre_trap._hip import check, ptr, stream_ptr
        B, H, T = c['B'], c['H'], c['T']
        sg = base._rand(2 * B, C, H, T, seed=7, scale=0.7)
        sgb = torch.empty((2 * B, H, T, C), dtype=c['ELT'], device='cuda')
        check(c['lib'].tt_wide_pack(ptr(sg.cuda().contiguous()), ptr(sgb), 2 * B, C, H, T, stream_ptr()), 'pack')
        torch.cuda.synchronize()
        c['sg'], c['sgb'], c['sw'] = sg, sgb, torch.tensor([0.5, -1.25, 2.0, 0.75, 1.5]).cuda()


@pytest.mark.parametrize('elt', ['bf16', 'fp16'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('d,form', FORMS, ids=lambda v: str(v))
@pytest.mark.parametrize('C', [4, 8])
def test_narrow_backward_values(C, d, form, shape, elt):
    c = _case(C, d, elt, shape)
    B, H, T = shape
    if form == 'riding':
        _riding_operands(c, C)
    out = [_run(c, C, d, form) for _ in range(2)]
    assert torch.equal(out[0][0], out[1][0]), 'dx differs between two calls in %d elements' % int((out[0][0] != out[1][0]).sum())
    for k, name in enumerate(('dW1', 'db1', 'dW2', 'db2')):
        assert torch.equal(out[0][1][k], out[1][1][k]), '%s differs between two calls' % name
    ref = c['ref']
    want = ref['dx']
    if form == 'gated':
        want = ref['dx'] * ref['gate']
    elif form == 'riding':
        sgr = c['sg'].float().to(c['ELT']).double().view(2, B, C, H, T)
        tsum = sgr[0] + sgr[1]
        want = (ref['dx'] + 0.75 * tsum) * ref['gate']
        ds = out[0][2].cpu().double()                        # (an atomic sum over the waves: held against float64, not between calls)
        dot = float((tsum * base._planar(c['xb'])).sum())
        assert torch.equal(ds[[0, 1, 2, 4]], torch.full((4,), 3.0, dtype=torch.float64))
        assert abs(float(ds[3]) - 3.0 - dot) <= 1e-3 * abs(dot) + 1e-3, (float(ds[3]) - 3.0, dot)
    base._close16(base._planar(out[0][0]), want, '%s dx C=%d d=%d %s %s' % (form, C, d, shape, elt), elt)
    base._weight_grads(C, out[0][1], ref, 0.5)


@pytest.mark.parametrize('elt', ['bf16', 'fp16'])
@pytest.mark.parametrize('C', [4, 8])
def test_inf_in_a_halo_only_step_reaches_the_sums(C, elt):
    """(2, 17, 66), dilation 3: row 16 is the second tile row's own and lies in the first tile row's bottom halo; frame 40 puts the pixel
    into a step of the upper tile that holds halo pixels only (chunk 21 of 25 at C = 8, 22 of 25 at C = 4), which runs no sums.  db2 and
    dW2 must be non-finite exactly where the restatement's are: in the planted channel."""
    shape, d, ch = (2, 17, 66), 3, 1
    c = _case(C, d, elt, shape)
    r16 = lambda t: t.float().to(c['ELT']).double()
    gb = c['gb'].clone()
    gb[0, 16, 40, ch] = float('inf')
    h_k, gr = base._planar(c['hb']), base._planar(gb)
    w2r = r16(c['w2d'].cpu())
    a2 = F.conv2d(h_k, w2r, c['b2d'].cpu().double())
    dA2 = gr * torch.where(a2 > 0, torch.ones_like(a2), torch.exp(a2))
    db2_ref, dw2_ref = dA2.sum((0, 2, 3)), torch.einsum('bohw,bihw->oi', r16(dA2), h_k)
    assert not bool(torch.isfinite(db2_ref[ch])) and not bool(torch.isfinite(dw2_ref[ch]).any()), 'the restatement carries the inf'
    _, grads, _ = _run(c, C, d, 'plain', gb=gb)
    db2, dw2 = grads[3].cpu(), grads[2].cpu().view(C, C)
    print('db2', db2.tolist(), 'restatement', db2_ref.tolist())
    assert torch.equal(torch.isfinite(db2), torch.isfinite(db2_ref)), (db2, db2_ref)
    assert torch.equal(torch.isfinite(dw2), torch.isfinite(dw2_ref)), (dw2, dw2_ref)
