"""
GPU checks of the block-backward loops whose global operands are requested a pixel group ahead and waited for by count
(csrc/wide_common.h gload_ahead; step d. of the C = 16 strips in csrc/conv_level_bf16.hip, the dx loop of k_wrb_dxw and phase 1 of
k_nrb_bwd_fused in csrc/conv_wide_bf16.hip).

VALUES, through the C ABI (tt_wide_rb_bwd, tt_wide_level_bwd_gated, tt_wide_level_bwd_gated_join), at the smallest shapes that cross every
boundary of those loops:
    strips, C = 16   8-row steps, 32-column strips   B = 2, H = 19 (two steps and a partial one), T = 40 (a full strip and one whose last
                                                     groups are partly and wholly beside the image)
    dxw, C = 32      8 x 32 tiles                    B = 2, H = 11, T = 40
    narrow, C = 4    16 x 64 tiles                   B = 2, H = 21, T = 72
dilations 1, 2, 3; plain and gated; the riding join forms at dilation 1; bf16 and the fp16 (_h) build.  dx, dW1, dW2, db1, db2
against the float64 restatement with the kernels' roundings, at the bars of tests/test_gpu_wide_bf16.py's stage-wise tests (a stored
element: one rounding + a small absolute term; dW1 2e-4, the others 2e-3), and dx bit-identical between two calls.  An operand that
arrived late or a request that left the tensor's row shows as O(1) errors in the last rows / columns of a tile -- the partial ones here.

RESOURCES, through tt_wide_bwd_kernel_attr (runtime metadata of the loaded code object, no launch): no private memory and the register
caps that give four / three / four workgroups per CU.
"""

import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ELTS = {'bf16': torch.bfloat16, 'fp16': torch.float16}
REL16 = {'bf16': 2.0 ** -8, 'fp16': 2.0 ** -11}          # one rounding of a stored element
ABS16 = {'bf16': 2e-3, 'fp16': 2.5e-4}                   # absolute slack, relative to the tensor's scale
SHAPES = {16: (2, 19, 40), 32: (2, 11, 40), 4: (2, 21, 72)}


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def _planar(t_nhwc):
    return t_nhwc.float().permute(0, 3, 1, 2).contiguous().cpu().double()


def _close16(got, want, name, elt):
    scale = float(want.abs().max())
    tol = REL16[elt] * want.abs() + ABS16[elt] * scale + 1e-30
    err = (got - want).abs()
    print('%s: worst |got - want| %.3e at scale %.3e' % (name, float(err.max()), scale))
    bad = err > tol
    assert not bool(bad.any()), '%s: %d of %d outside one rounding, worst %.3e (scale %.3e)' % (name, int(bad.sum()), bad.numel(), float(err.max()), scale)


def _rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.fixture(autouse=True)
def _unit_loss_scale():
    """The weight-gradient reduces divide by the calling thread's loss scale (fp16 training): 1 here, whatever ran before."""
    from timbre_trap import _hip
    prev = _hip.lib().tt_set_loss_scale(1.0)
    yield
    _hip.lib().tt_set_loss_scale(prev)


_CASES = {}


def _case(C, d, elt):
    """Inputs on the device, the kernel's own forward (h1 as stored), and the float64 restatement of the backward: computed once per
    (C, dilation, element type), shared by the plain, gated and riding tests, never modified."""
    key = (C, d, elt)
    if key in _CASES:
        return _CASES[key]
    from timbre_trap._hip import check, ptr, stream_ptr
    from timbre_trap.framework import ops
    ELT = ELTS[elt]
    lib, st = ops.lib16(ELT), stream_ptr()
    B, H, T = SHAPES[C]
    r16 = lambda t: t.float().to(ELT).double()
    x = _rand(B, C, H, T, seed=1)
    w1 = _rand(C, C, 3, 3, seed=2, scale=1.0 / (3 * C ** 0.5))
    b1 = _rand(C, seed=3, scale=0.3)
    w2 = _rand(C, C, 1, 1, seed=4, scale=1.0 / C ** 0.5)
    b2 = _rand(C, seed=5, scale=0.3)
    gy = _rand(B, C, H, T, seed=6)
    xd, w1d, b1d, w2d, b2d, gyd = (t.cuda().contiguous() for t in (x, w1, b1, w2, b2, gy))
    nhwc = lambda b=B: torch.empty((b, H, T, C), dtype=ELT, device='cuda')
    xb, gb, yb, hb = nhwc(), nhwc(), nhwc(), nhwc()
    check(lib.tt_wide_pack(ptr(xd), ptr(xb), B, C, H, T, st), 'pack')
    check(lib.tt_wide_pack(ptr(gyd), ptr(gb), B, C, H, T, st), 'pack')
    check(lib.tt_wide_rb_fwd(ptr(xb), ptr(w1d), ptr(b1d), ptr(w2d), ptr(b2d), ptr(yb), ptr(hb), B, C, H, T, d, st), 'fwd')
    torch.cuda.synchronize()
    # the restatement of tests/test_gpu_wide_bf16.py::_stagewise: every stage from the kernel's own stored input, dA2 and dA1 rounded where
    # the kernels round them.  The one-pass kernels keep dA1 in LDS: the restatement's own rounded dA1 stands in; the per-stage path (C = 32)
    # stores dA1 at the head of its workspace: that tensor, held against the restatement first, feeds the dx and dW1 references
    xr, gr, w1r, w2r = r16(x), r16(gy), r16(w1), r16(w2)
    h_k = _planar(hb)
    a2 = F.conv2d(h_k, w2r, b2.double())
    dA2 = gr * torch.where(a2 > 0, torch.ones_like(a2), torch.exp(a2))
    dA2r = r16(dA2)
    dh1 = F.conv2d(dA2r, w2r.transpose(0, 1).contiguous())
    dA1 = dh1 * torch.where(h_k > 0, torch.ones_like(h_k), h_k + 1)
    da1r = r16(dA1)
    if C >= 16 and not lib.tt_wide_rb_bwd_is_onepass(C, d):
        ws = torch.zeros(lib.tt_wide_scratch_bytes(B, C, H, T), dtype=torch.uint8, device='cuda')
        dx0 = nhwc()
        g0 = [torch.zeros(s_, dtype=torch.float32, device='cuda') for s_ in ((C, C, 3, 3), (C,), (C, C, 1, 1), (C,))]
        check(lib.tt_wide_rb_bwd(ptr(xb), ptr(hb), ptr(gb), ptr(w1d), ptr(w2d), ptr(b2d), ptr(dx0), ptr(g0[0]), ptr(g0[1]), ptr(g0[2]), ptr(g0[3]),
                                 ptr(ws), B, C, H, T, d, st), 'bwd')
        torch.cuda.synchronize()
        da1r = _planar(ws[:B * H * T * C * 2].view(ELT).view(B, H, T, C))
        _close16(da1r, dA1, 'dA1 C=%d d=%d %s' % (C, d, elt), elt)
    dx_ref = gr + F.conv_transpose2d(da1r, w1r, padding=d, dilation=d)
    xp = F.pad(xr, (d, d, d, d))
    dw1_ref = torch.stack([torch.stack([
        torch.einsum('bohw,bihw->oi', da1r, xp[:, :, kh * d: kh * d + H, kw * d: kw * d + T]) for kw in range(3)], -1)
        for kh in range(3)], -2)
    ref = dict(dx=dx_ref, gate=torch.where(xr > 0, torch.ones_like(xr), xr + 1), dw1=dw1_ref, dw2=torch.einsum('bohw,bihw->oi', dA2r, h_k),
               db1=dA1.sum((0, 2, 3)), db2=dA2.sum((0, 2, 3)))
    _CASES[key] = dict(lib=lib, B=B, H=H, T=T, ELT=ELT, xb=xb, hb=hb, gb=gb, w1d=w1d, w2d=w2d, b2d=b2d, ref=ref)
    return _CASES[key]


def _weight_grads(C, grads, ref, base):
    got = [g.cpu().double() - base for g in grads]
    assert _rel(got[0], ref['dw1']) < 2e-4, 'dw1 %.3e' % _rel(got[0], ref['dw1'])
    assert _rel(got[2].view(C, C), ref['dw2']) < 2e-3, 'dw2 %.3e' % _rel(got[2].view(C, C), ref['dw2'])
    assert _rel(got[1], ref['db1']) < 2e-3, 'db1 %.3e' % _rel(got[1], ref['db1'])
    assert _rel(got[3], ref['db2']) < 2e-3, 'db2 %.3e' % _rel(got[3], ref['db2'])


def _level_args(c, C, d, dx, grads, ws):
    from timbre_trap._hip import ptr
    one = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
    return (1, one(c['xb']), one(c['hb']), ptr(c['gb']), one(c['w1d']), one(c['w2d']), one(c['b2d']), ptr(dx), None, None,
            one(grads[0]), one(grads[1]), one(grads[2]), one(grads[3]), ptr(ws), c['B'], C, c['H'], c['T'], (ctypes.c_int * 1)(d))


@pytest.mark.parametrize('elt', ['bf16', 'fp16'])
@pytest.mark.parametrize('d', [1, 2, 3])
@pytest.mark.parametrize('C', [16, 32, 4])
def test_plain_backward_values(C, d, elt):
    """tt_wide_rb_bwd: the strips (C = 16), k_wrb_bwd_a + k_wrb_dxw (C = 32), k_nrb_bwd_fused (C = 4) on the default dispatch."""
    from timbre_trap._hip import check, ptr, stream_ptr
    c = _case(C, d, elt)
    lib, st, B, H, T = c['lib'], stream_ptr(), c['B'], c['H'], c['T']
    if C >= 16:
        assert lib.tt_wide_rb_bwd_is_onepass(C, d) == (1 if C == 16 else 0), 'the default dispatch: strips at C = 16, per-stage kernels at C = 32'
    shapes = ((C, C, 3, 3), (C,), (C, C, 1, 1), (C,))
    ws = torch.zeros(lib.tt_wide_scratch_bytes(B, C, H, T), dtype=torch.uint8, device='cuda')
    out = []
    for _ in range(2):
        dx = torch.empty((B, H, T, C), dtype=c['ELT'], device='cuda')
        grads = [torch.full(s, 0.5, dtype=torch.float32, device='cuda') for s in shapes]
        check(lib.tt_wide_rb_bwd(ptr(c['xb']), ptr(c['hb']), ptr(c['gb']), ptr(c['w1d']), ptr(c['w2d']), ptr(c['b2d']), ptr(dx), ptr(grads[0]),
                                 ptr(grads[1]), ptr(grads[2]), ptr(grads[3]), ptr(ws), B, C, H, T, d, st), 'bwd')
        torch.cuda.synchronize()
        out.append((dx, grads))
    assert torch.equal(out[0][0], out[1][0]), 'dx differs between two calls in %d elements' % int((out[0][0] != out[1][0]).sum())
    _close16(_planar(out[0][0]), c['ref']['dx'], 'dx C=%d d=%d %s' % (C, d, elt), elt)
    _weight_grads(C, out[0][1], c['ref'], 0.5)


@pytest.mark.parametrize('elt', ['bf16', 'fp16'])
@pytest.mark.parametrize('d', [1, 2, 3])
@pytest.mark.parametrize('C', [16, 32, 4])
def test_gated_backward_values(C, d, elt):
    """tt_wide_level_bwd_gated on a level of one block: dx * ELU'(x).  At dilation 1 the block's own kernel gates in its epilogue (one rounding);
    at dilation 2, 3 the plain kernel runs and the gate follows as a stage of its own."""
    from timbre_trap._hip import check, stream_ptr
    c = _case(C, d, elt)
    lib, st, B, H, T = c['lib'], stream_ptr(), c['B'], c['H'], c['T']
    shapes = ((C, C, 3, 3), (C,), (C, C, 1, 1), (C,))
    ws = torch.zeros(lib.tt_wide_level_scratch_bytes(1, B, C, H, T), dtype=torch.uint8, device='cuda')
    out = []
    for _ in range(2):
        dx = torch.empty((B, H, T, C), dtype=c['ELT'], device='cuda')
        grads = [torch.full(s, 0.5, dtype=torch.float32, device='cuda') for s in shapes]
        check(lib.tt_wide_level_bwd_gated(*_level_args(c, C, d, dx, grads, ws), st), 'level gated')
        torch.cuda.synchronize()
        out.append((dx, grads))
    assert torch.equal(out[0][0], out[1][0]), 'dx differs between two calls in %d elements' % int((out[0][0] != out[1][0]).sum())
    stage_in = c['ref']['dx']
    if d > 1:
        # the gate is a stage of its own behind the plain kernel: fed, like every stage of the restatement, with the kernel's own stored input
        # -- the plain dx, which test_plain_backward_values holds against the restatement
        from timbre_trap._hip import ptr
        dxp = torch.empty((B, H, T, C), dtype=c['ELT'], device='cuda')
        gp = [torch.zeros(s, dtype=torch.float32, device='cuda') for s in shapes]
        wsp = torch.zeros(lib.tt_wide_scratch_bytes(B, C, H, T), dtype=torch.uint8, device='cuda')
        check(lib.tt_wide_rb_bwd(ptr(c['xb']), ptr(c['hb']), ptr(c['gb']), ptr(c['w1d']), ptr(c['w2d']), ptr(c['b2d']), ptr(dxp), ptr(gp[0]),
                                 ptr(gp[1]), ptr(gp[2]), ptr(gp[3]), ptr(wsp), B, C, H, T, d, st), 'bwd')
        torch.cuda.synchronize()
        stage_in = _planar(dxp)
    _close16(_planar(out[0][0]), stage_in * c['ref']['gate'], 'gated dx C=%d d=%d %s' % (C, d, elt), elt)
    _weight_grads(C, out[0][1], c['ref'], 0.5)


@pytest.mark.parametrize('elt', ['bf16', 'fp16'])
@pytest.mark.parametrize('reps', [1, 2])
@pytest.mark.parametrize('C', [16, 32, 4])
def test_riding_join_values(C, reps, elt):
    """tt_wide_level_bwd_gated_join at dilation 1 -- C = 16: k_wrb_bwds_sj (three operands per group requested ahead), C = 32: the riding
    k_wrb_dxw (the current group's operands at the top of the iteration), C = 4: the riding k_nrb_bwd_fused (phase-1 keys per step):
    dx = (dy + W1^T (*) dA1 + w (g0 + g1)) ELU'(x) against the restatement, the skip weight's gradient <g0 + g1, x> against float64."""
    from timbre_trap._hip import check, ptr, stream_ptr
    d = 1
    c = _case(C, d, elt)
    lib, st, B, H, T = c['lib'], stream_ptr(), c['B'], c['H'], c['T']
    sg = _rand(reps * B, C, H, T, seed=7, scale=0.7)
    sgb = torch.empty((reps * B, H, T, C), dtype=c['ELT'], device='cuda')
    check(lib.tt_wide_pack(ptr(sg.cuda().contiguous()), ptr(sgb), reps * B, C, H, T, st), 'pack')
    w = torch.tensor([0.5, -1.25, 2.0, 0.75, 1.5]).cuda()
    shapes = ((C, C, 3, 3), (C,), (C, C, 1, 1), (C,))
    ws = torch.zeros(lib.tt_wide_level_scratch_bytes(1, B, C, H, T), dtype=torch.uint8, device='cuda')
    out = []
    for _ in range(2):
        dx = torch.empty((B, H, T, C), dtype=c['ELT'], device='cuda')
        grads = [torch.full(s, 0.5, dtype=torch.float32, device='cuda') for s in shapes]
        ds = torch.full((5,), 3.0, device='cuda')
        rc = lib.tt_wide_level_bwd_gated_join(*_level_args(c, C, d, dx, grads, ws), ptr(sgb), reps, ptr(w), 3, ptr(ds), st)
        assert rc == 0, 'every width has a riding form on the default dispatch (rc %d)' % rc
        torch.cuda.synchronize()
        out.append((dx, grads, ds))
    assert torch.equal(out[0][0], out[1][0]), 'dx differs between two calls in %d elements' % int((out[0][0] != out[1][0]).sum())
    sgr = sg.float().to(c['ELT']).double().view(reps, B, C, H, T)
    tsum = sgr[0] + sgr[1] if reps == 2 else sgr[0]
    xr = _planar(c['xb'])
    want = (c['ref']['dx'] + 0.75 * tsum) * c['ref']['gate']
    _close16(_planar(out[0][0]), want, 'riding dx reps=%d %s' % (reps, elt), elt)
    _weight_grads(C, out[0][1], c['ref'], 0.5)
    ds = out[0][2].cpu().double()
    assert torch.equal(ds[[0, 1, 2, 4]], torch.full((4,), 3.0, dtype=torch.float64))
    dot = float((tsum * xr).sum())
    assert abs(float(ds[3]) - 3.0 - dot) <= 1e-3 * abs(dot) + 1e-3, (float(ds[3]) - 3.0, dot)


def _attr(lib, half, kernel, C, d, form):
    fn = lib.tt_wide_bwd_kernel_attr_h if half else lib.tt_wide_bwd_kernel_attr
    local, regs = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = fn(kernel, C, d, form, ctypes.byref(local), ctypes.byref(regs))
    return rc, local.value, regs.value


@pytest.mark.parametrize('half', [False, True], ids=['bf16', 'fp16'])
def test_backward_kernels_keep_everything_in_registers(half):
    """No private memory (a stack object or a spill: either is a vector-memory round trip with a full vmcnt(0) behind it, inside loops that
    count their own requests) and the register caps of the occupancy each kernel is launched for: strips C = 16 <= 128 (four workgroups
    per CU), k_wrb_dxw C = 32 <= 168 (three), k_nrb_bwd_fused C = 4 <= 128 (four).  The riding forms are reported, not bounded."""
    from timbre_trap import _hip
    lib = _hip.lib()
    STRIPS, DXW, NARROW = 0, 1, 2
    bad = []
    for kernel, C, cap, name in ((STRIPS, 16, 128, 'k_wrb_bwds<16>'), (DXW, 32, 168, 'k_wrb_dxw<32>'), (NARROW, 4, 128, 'k_nrb_bwd_fused<4>')):
        for d, form in ((1, 0), (2, 0), (3, 0), (1, 1)):
            rc, local, regs = _attr(lib, half, kernel, C, d, form)
            print('%s dilation %d %s: private %d bytes, %d registers' % (name, d, ('plain', 'gated')[form], local, regs))
            assert rc == 0, (name, d, form, rc)
            if local != 0 or regs > cap:
                bad.append((name, d, form, local, regs))
        rc, local, regs = _attr(lib, half, kernel, C, 1, 2)
        assert rc == 0
        print('%s dilation 1 riding: private %d bytes, %d registers' % (name, local, regs))
    assert not bad, bad
    # combinations that are not compiled say so and leave the outputs alone
    assert _attr(lib, half, STRIPS, 16, 2, 1)[0] == -2 and _attr(lib, half, STRIPS, 32, 1, 2)[0] == -2 and _attr(lib, half, NARROW, 16, 1, 0)[0] == -2
    assert _attr(lib, half, 3, 16, 1, 0)[0] == -2 and _attr(lib, half, STRIPS, 16, 1, 3)[0] == -1
