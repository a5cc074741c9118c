"""
GPU tests of the split-operand TRAINING of the wide residual levels (csrc/conv_x3.hip "training"; ops.X3_TRAIN, ops.X3LevelTrainFn;
reference modules.py:721-777 and the autograd backward of those lines).

Forward with saved activations and backward run on (hi, lo) fp16 pairs -- three 16-bit matrix products per fp32 product, the two weight
gradients (K = pixels) included -- so every result must agree with a float64 evaluation at fp32-arithmetic level.  The measure is
max |diff| / max |float64 tensor|; the bar per tensor is max(2e-6, 4 x the same measure of tt_resblock_fwd / tt_resblock_bwd with
flags 0 -- the exact-fp32 kernels -- on the same inputs): 2e-6 is the bar of tests/test_gpu_x3.py, the factor 4 the two bits a pair of
halves (22) has less than fp32 (24).  An indexing error of any kind shows at O(1), a lost cross term at 2^-11 = 5e-4, a lost gradient scale
as a handful of bits.  The gradient scale is a power of two, so it must never show in a result: the scale-invariance test is bitwise.
"""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BAR = 2e-6
SHAPES = [(2, 13, 70), (1, 37, 33), (3, 16, 64)]
NAMES = ('y', 'h1', 'dx', 'dw1', 'db1', 'dw2', 'db2')


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def _params(C, seed=0):
    w1 = _rand(C, C, 3, 3, seed=seed + 2, scale=1.0 / (3 * C ** 0.5))
    b1 = _rand(C, seed=seed + 3, scale=0.3)
    w2 = _rand(C, C, 1, 1, seed=seed + 4, scale=1.0 / C ** 0.5)
    b2 = _rand(C, seed=seed + 5, scale=0.3)
    return w1, b1, w2, b2


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def _biteq(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _inputs(C, shape):
    B, H, T = shape
    return _rand(B, C, H, T, seed=1), _params(C), _rand(B, C, H, T, seed=9)


@functools.lru_cache(maxsize=None)
def _block64(C, d, shape):
    """float64 autograd of one block on the CPU with dy of unit scale: (y, h1, dx, dw1, db1, dw2, db2).  Computed once per case; the
    gradients are linear in dy, so the tests that scale dy scale these."""
    x, params, dy = _inputs(C, shape)
    x = x.double().requires_grad_(True)
    p = [t.double().requires_grad_(True) for t in params]
    h1 = F.elu(F.conv2d(x, p[0], p[1], padding=d, dilation=d))
    y = F.elu(F.conv2d(h1, p[2], p[3])) + x
    g = torch.autograd.grad(y, [x, p[0], p[1], p[2], p[3]], dy.double())
    return tuple(t.detach() for t in (y, h1) + g)


def _x3_buf(B, C, H, T):
    return torch.empty((B, H, T, 2, C), dtype=torch.float16, device='cuda')


def _run_x3_block(x, params, dy, d):
    """Training forward + backward of one block through the C ABI -> (y, h1, dx, dw1, db1, dw2, db2) as fp32 tensors on the GPU."""
    from timbre_trap._hip import check, lib, ptr, stream_ptr
    L, st = lib(), stream_ptr()
    B, C, H, T = x.shape
    xd, dyd = x.cuda().contiguous(), dy.cuda().contiguous()
    w1, b1, w2, b2 = [p.cuda().contiguous() for p in params]
    xs, ys, hs, gs = (_x3_buf(B, C, H, T) for _ in range(4))
    check(L.tt_x3_pack(ptr(xd), ptr(xs), B, C, H, T, st), 'tt_x3_pack')
    check(L.tt_x3_rb_fwd_train(ptr(xs), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(ys), 0, ptr(hs), B, C, H, T, d, st), 'tt_x3_rb_fwd_train')
    y, h1 = torch.empty_like(xd), torch.empty_like(xd)
    check(L.tt_x3_unpack(ptr(ys), ptr(y), B, C, H, T, st), 'tt_x3_unpack')
    check(L.tt_x3_unpack(ptr(hs), ptr(h1), B, C, H, T, st), 'tt_x3_unpack')
    scale = torch.empty(2, dtype=torch.float32, device='cuda')
    sws = torch.empty(L.tt_x3_grad_scale_scratch_bytes(), dtype=torch.uint8, device='cuda')
    check(L.tt_x3_grad_scale(ptr(dyd), dyd.numel(), ptr(scale), ptr(sws), st), 'tt_x3_grad_scale')
    check(L.tt_x3_pack_scaled(ptr(dyd), ptr(gs), ptr(scale), B, C, H, T, st), 'tt_x3_pack_scaled')
    ws = torch.empty(L.tt_x3_rb_bwd_scratch_bytes(B, C, H, T), dtype=torch.uint8, device='cuda')
    dx = torch.empty_like(xd)
    dw1, db1, dw2, db2 = (torch.zeros_like(t) for t in (w1, b1, w2, b2))
    check(L.tt_x3_rb_bwd(ptr(xs), ptr(hs), ptr(gs), ptr(w1), ptr(w2), ptr(b2), ptr(dx), 1, ptr(dw1), ptr(db1), ptr(dw2), ptr(db2), ptr(scale),
                         ptr(ws), B, C, H, T, d, st), 'tt_x3_rb_bwd')
    # the x3 form of dx (what the next block's backward reads), unpacked with the scale: the same values before the split
    dxs = _x3_buf(B, C, H, T)
    t1, t2, t3, t4 = (torch.zeros_like(t) for t in (w1, b1, w2, b2))
    check(L.tt_x3_rb_bwd(ptr(xs), ptr(hs), ptr(gs), ptr(w1), ptr(w2), ptr(b2), ptr(dxs), 0, ptr(t1), ptr(t2), ptr(t3), ptr(t4), ptr(scale),
                         ptr(ws), B, C, H, T, d, st), 'tt_x3_rb_bwd')
    dx2 = torch.empty_like(xd)
    check(L.tt_x3_unpack_scaled(ptr(dxs), ptr(dx2), ptr(scale), B, C, H, T, st), 'tt_x3_unpack_scaled')
    torch.cuda.synchronize()
    fin = torch.isfinite(dx)
    assert torch.equal(fin, torch.isfinite(dx2))
    assert bool(((dx2 - dx).abs() <= dx.abs() * 2.0 ** -21 + float(dx[fin].abs().max() if fin.any() else 0) * 2.0 ** -40)[fin].all())
    assert _biteq(dw1, t1) and _biteq(db1, t2) and _biteq(dw2, t3) and _biteq(db2, t4)
    return y, h1, dx, dw1, db1, dw2, db2


def _run_fp32_block(x, params, dy, d):
    """The same through the exact-fp32 kernels (tt_resblock_fwd / tt_resblock_bwd, flags 0)."""
    from timbre_trap._hip import check, lib, ptr, stream_ptr
    L, st = lib(), stream_ptr()
    B, C, H, T = x.shape
    xd, dyd = x.cuda().contiguous(), dy.cuda().contiguous()
    w1, b1, w2, b2 = [p.cuda().contiguous() for p in params]
    y, h1, dx = torch.empty_like(xd), torch.empty_like(xd), torch.empty_like(xd)
    check(L.tt_resblock_fwd(ptr(xd), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(y), ptr(h1), B, C, H, T, d, 0, st), 'tt_resblock_fwd')
    dw1, db1, dw2, db2 = (torch.zeros_like(t) for t in (w1, b1, w2, b2))
    ws = torch.empty(xd.numel() + L.tt_wgrad_scratch_floats(), dtype=torch.float32, device='cuda')
    check(L.tt_resblock_bwd(ptr(xd), ptr(h1), ptr(dyd), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(dx), ptr(dw1), ptr(db1), ptr(dw2), ptr(db2),
                            ptr(ws), B, C, H, T, d, 0, st), 'tt_resblock_bwd')
    torch.cuda.synchronize()
    return y, h1, dx, dw1, db1, dw2, db2


def _check_against(got, base, want, tag):
    """got (x3) and base (fp32 kernels) against want (float64): per tensor, measure < max(2e-6, 4 x the fp32 kernels' measure)."""
    bad = []
    for name, g, b, w in zip(NAMES, got, base, want):
        e, e32 = _rel(g, w), _rel(b, w)
        print('%s %-3s x3 %.3e  fp32 %.3e  bar %.3e' % (tag, name, e, e32, max(BAR, 4 * e32)))
        if not e < max(BAR, 4 * e32):
            bad.append((name, e, e32))
    assert not bad, bad


@pytest.mark.parametrize('C', [16, 32])
@pytest.mark.parametrize('d', [1, 2, 3])
@pytest.mark.parametrize('shape', SHAPES)
def test_block_forward_and_backward_match_float64(C, d, shape):
    """Measured worst case per tensor over these cases (x3 / the fp32 kernels), also in DESIGN.md section 6b --
    C = 16: y 1.48e-7 / 1.35e-7, h1 2.47e-7 / 3.96e-7, dx 1.21e-7 / 1.71e-7, dw1 2.64e-7 / 1.49e-7, db1 3.06e-7 / 2.53e-7, dw2 2.37e-7 / 2.31e-7,
    db2 2.57e-7 / 1.55e-7;  C = 32: y 1.52e-7 / 1.51e-7, h1 3.41e-7 / 5.20e-7, dx 1.59e-7 / 3.12e-7, dw1 2.48e-7 / 2.04e-7, db1 2.89e-7 / 1.17e-7,
    dw2 2.39e-7 / 3.02e-7, db2 2.16e-7 / 1.66e-7."""
    x, params, dy = _inputs(C, shape)
    want = _block64(C, d, shape)
    _check_against(_run_x3_block(x, params, dy, d), _run_fp32_block(x, params, dy, d), want, 'C%d d%d %s' % (C, d, shape))


@pytest.fixture
def cu_limit():
    from timbre_trap import _hip
    lib = _hip.lib()
    prev = lib.tt_set_cu_limit(0)
    yield lib.tt_set_cu_limit
    lib.tt_set_cu_limit(prev)


@pytest.mark.parametrize('C', [16, 32])
@pytest.mark.parametrize('d', [1, 2, 3])
@pytest.mark.parametrize('shape', [(2, 13, 70), (3, 16, 64)])
def test_block_with_a_capped_grid_matches_float64(C, d, shape, cu_limit):
    """One CU's worth of workgroups (tt_set_cu_limit): every persistent loop of the training kernels runs several iterations per
    workgroup, as at the bench's sizes -- k_x3_conv MODE 1 / 2 and k_x3_wgrad walk 3 to 18 tiles each (restaging, accumulators carried
    across tiles, the bias re-read), k_x3_bwd_a 4 to 6 pixel groups per wave (prefetch hand-over, reuse of the transposition buffers), and
    the reduce sums dumps that hold several tiles.  Same bars as the uncapped test."""
    x, params, dy = _inputs(C, shape)
    want = _block64(C, d, shape)
    base = _run_fp32_block(x, params, dy, d)
    cu_limit(1)
    _check_against(_run_x3_block(x, params, dy, d), base, want, 'capped C%d d%d %s' % (C, d, shape))


@pytest.mark.parametrize('C', [16, 32])
def test_block_backward_with_gradients_of_realistic_size(C):
    """dy ~ 1e-9 (a mean-reduced loss): without the device-side gradient scale the pairs would keep a handful of bits."""
    d, shape = 2, (2, 13, 70)
    x, params, dy = _inputs(C, shape)
    s = 1e-9
    want = _block64(C, d, shape)
    want = want[:2] + tuple(t * s for t in want[2:])
    dys = dy * s
    _check_against(_run_x3_block(x, params, dys, d), _run_fp32_block(x, params, dys, d), want, 'C%d dy 1e-9' % C)


def _level(C, shape, seed=0, dilations=(1, 2, 3)):
    B, H, T = shape
    x = _rand(B, C, H, T, seed=seed + 1)
    params = []
    for i in range(len(dilations)):
        params += list(_params(C, seed=seed + 10 * i))
    dy = _rand(B, C, H, T, seed=seed + 7)
    return x, params, dy


def _run_level_fn(x, params, dy, dilations=(1, 2, 3)):
    """ops.X3LevelTrainFn forward + backward -> (y, [dx, 12 parameter gradients])."""
    from timbre_trap.framework import ops
    xd = x.cuda().requires_grad_(True)
    pd = [p.cuda().requires_grad_(True) for p in params]
    y = ops.X3LevelTrainFn.apply(xd, tuple(dilations), *pd)
    grads = torch.autograd.grad(y, [xd] + pd, dy.cuda())
    torch.cuda.synchronize()
    return y.detach(), [g.detach() for g in grads]


def test_gradient_scale_never_shows_in_a_result():
    """dy, dy 2^-30 and dy 2^10 give gradients that are BITWISE 2^-30 and 2^10 times the first run's (where the scaled value is a normal
    fp32 number): the scale is a power of two derived from abs-max(dy), every multiplication by it is exact."""
    C, shape = 32, (2, 13, 70)
    x, params, dy = _level(C, shape)
    _, base = _run_level_fn(x, params, dy)
    tiny = float(torch.finfo(torch.float32).tiny)
    for k in (2.0 ** -30, 2.0 ** 10):
        _, got = _run_level_fn(x, params, dy * k)
        for i, (g, b) in enumerate(zip(got, base)):
            want = b * k
            normal = (want.abs() >= tiny) | (want == 0)
            assert _biteq(g[normal], want[normal]), (k, i, float((g - want).abs().max()))
            assert int(normal.sum()) > 0.99 * normal.numel()


def test_zero_gradient_gives_exact_zeros():
    C, shape = 16, (1, 37, 33)
    x, params, dy = _level(C, shape)
    _, got = _run_level_fn(x, params, torch.zeros_like(dy))
    for g in got:
        assert bool((g == 0).all())


@pytest.mark.parametrize('cus', [0, 2])
def test_level_backward_is_bit_reproducible(cus, cu_limit):
    """cus = 2: two CUs' worth of workgroups, every kernel walks several tiles / groups per workgroup (0: the whole chip)."""
    C, shape = 32, (3, 16, 64)
    x, params, dy = _level(C, shape)
    cu_limit(cus)
    y1, g1 = _run_level_fn(x, params, dy)
    y2, g2 = _run_level_fn(x, params, dy)
    assert _biteq(y1, y2)
    for a, b in zip(g1, g2):
        assert _biteq(a, b)


@pytest.mark.parametrize('C', [16, 32])
def test_level_function_equals_three_blocks_on_the_fp32_kernels(C, monkeypatch):
    """X3LevelTrainFn with dilations (1, 2, 3) against ResBlockFn three times on the exact-fp32 kernels: output and all 13 gradients at the
    bars of the block test -- per tensor max(2e-6, 4 x the fp32 kernels' own distance from float64)."""
    from timbre_trap.framework import ops
    monkeypatch.setattr(ops, 'PRECISION', 'fp32')
    shape = (2, 16, 64)
    x, params, dy = _level(C, shape, seed=40)
    y, grads = _run_level_fn(x, params, dy)
    xd = x.cuda().requires_grad_(True)
    pd = [p.cuda().requires_grad_(True) for p in params]
    cur = xd
    for i, d in enumerate((1, 2, 3)):
        cur = ops.ResBlockFn.apply(cur, *pd[4 * i:4 * i + 4], d)
    ref = torch.autograd.grad(cur, [xd] + pd, dy.cuda())
    # float64 on the CPU: only to size the bars
    x64 = x.double().requires_grad_(True)
    p64 = [p.double().requires_grad_(True) for p in params]
    c64 = x64
    for i, d in enumerate((1, 2, 3)):
        h = F.elu(F.conv2d(c64, p64[4 * i], p64[4 * i + 1], padding=d, dilation=d))
        c64 = F.elu(F.conv2d(h, p64[4 * i + 2], p64[4 * i + 3])) + c64
    g64 = torch.autograd.grad(c64, [x64] + p64, dy.double())
    bad = []
    for name, a, b, w in zip(['y', 'dx'] + ['p%d' % i for i in range(12)], [y] + grads, [cur.detach()] + list(ref), [c64.detach()] + list(g64)):
        e, e32 = _rel(a, b), _rel(b, w)
        print('C%d %-3s x3 vs fp32 %.3e  fp32 vs f64 %.3e' % (C, name, e, e32))
        if not e < max(BAR, 4 * e32):
            bad.append((name, e, e32))
    assert not bad, bad


def _blocks(C):
    from timbre_trap.framework.modules import ResidualConv2dBlock
    torch.manual_seed(0)
    return tuple(ResidualConv2dBlock(C, C, 3, d).cuda() for d in (1, 2, 3))


def test_routing(monkeypatch):
    """residual_level reaches the new Function only with X3_TRAIN on, in fp32 mode, under grad."""
    from timbre_trap.framework import ops
    calls = []
    real = ops.x3_level_train
    monkeypatch.setattr(ops, 'x3_level_train', lambda x, blocks: (calls.append(x.size(1)), real(x, blocks))[1])
    blocks = _blocks(16)
    x = _rand(1, 16, 9, 40, seed=3).cuda()
    monkeypatch.setattr(ops, 'PRECISION', 'fp32')
    monkeypatch.setattr(ops, 'X3_TRAIN', False)
    y_off = ops.residual_level(x, blocks)
    assert calls == [] and y_off.requires_grad
    monkeypatch.setattr(ops, 'X3_TRAIN', True)
    y_on = ops.residual_level(x, blocks)
    assert calls == [16] and y_on.requires_grad and y_on.dtype == torch.float32 and y_on.shape == x.shape
    assert _rel(y_on.detach(), y_off.detach()) < 1e-5
    with torch.no_grad():
        y_ng = ops.residual_level(x, blocks)                      # the inference route stays as it is
    assert calls == [16] and not y_ng.requires_grad
    monkeypatch.setattr(ops, 'PRECISION', 'bf16')
    ops.residual_level(x, blocks)
    assert calls == [16]
    monkeypatch.setattr(ops, 'PRECISION', 'fp32')
    narrow = _blocks(8)
    ops.residual_level(_rand(1, 8, 9, 40, seed=3).cuda(), narrow)   # narrow levels stay on the fp32 kernels
    assert calls == [16]
    monkeypatch.setattr(ops, 'X3_TRAIN_CHANNELS', (32,))            # a width taken off the route
    ops.residual_level(x, blocks)
    assert calls == [16]


def _model_grads(x3_train, skip, monkeypatch):
    from timbre_trap.framework import TimbreTrap, compute_consistency_loss, compute_reconstruction_loss, compute_transcription_loss, ops
    monkeypatch.setattr(ops, 'PRECISION', 'fp32')
    monkeypatch.setattr(ops, 'X3_TRAIN', x3_train)
    torch.manual_seed(5)
    model = TimbreTrap(22050, 9, 60, 3, latent_size=128, model_complexity=2, skip_connections=skip).cuda()
    c = _rand(2, 2, 540, 48, seed=21).cuda()
    gt = (_rand(2, 540, 48, seed=22) > 0.9).float().cuda()

    def skips(emb):
        return model.skip_joins(emb, defer=True) or model.apply_skip_connections(emb)
    latents, emb, _ = model.encoder(c)
    rec, trn = model.decode_pair(latents, skips(emb))
    lat2, emb2, _ = model.encoder(trn)
    trn_rec, trn_scr = model.decode_pair(lat2, skips(emb2))
    l_rec = compute_reconstruction_loss(rec, c)
    l_trn = compute_transcription_loss(model.to_activations(trn), gt, True)
    l_sp, l_sc = compute_consistency_loss(trn_rec, trn_scr, trn)
    total = l_rec + l_trn + (l_sp + l_sc)
    assert bool(torch.isfinite(total))
    names, ps = zip(*model.named_parameters())
    grads = torch.autograd.grad(total, ps)
    torch.cuda.synchronize()
    return float(total.detach()), dict(zip(names, (g.detach() for g in grads)))


@pytest.mark.parametrize('skip', [False, True])
def test_model_parameter_gradients_with_the_switch_on_and_off(skip, monkeypatch):
    """encoder -> decode_pair -> the three losses in fp32 mode: every parameter gradient with X3_TRAIN on against off, 1e-4 of each
    tensor's max (the project's bar for fp32-class paths).  Measured worst (two boxes): 2.5e-6 / 2.8e-6 without skip connections
    (encoder.convin.0.weight), 5.0e-7 / 8.9e-7 with (decoder.convout.weight); also in DESIGN.md section 6b."""
    from timbre_trap.framework import ops
    seen = []
    real = ops.x3_level_train
    monkeypatch.setattr(ops, 'x3_level_train', lambda x, blocks: (seen.append(x.size(1)), real(x, blocks))[1])
    l_off, g_off = _model_grads(False, skip, monkeypatch)
    assert seen == []
    l_on, g_on = _model_grads(True, skip, monkeypatch)
    assert sorted(set(seen)) == [16, 32] and len(seen) >= 8          # two wide levels each in encoder and decoder, two passes of either
    assert abs(l_on - l_off) <= 1e-5 * abs(l_off)
    worst = max((_rel(g_on[n], g_off[n]), n) for n in g_off)
    print('skip=%s worst parameter-gradient distance %.3e (%s)' % (skip, worst[0], worst[1]))
    assert worst[0] < 1e-4, worst


def test_values_out_of_range_come_out_non_finite():
    """One activation at 1e5 (beyond fp16's 65504): the training forward's output is non-finite there, never finite and wrong; a NaN in
    dy gives a non-finite dx.  Plain values: nothing here faults."""
    C, d, shape = 16, 1, (1, 9, 40)
    x, params, dy = _inputs(C, shape)
    xb = x.clone()
    xb[0, 3, 4, 5] = 1e5
    y = _run_x3_block(xb, params, dy, d)[0]
    assert not bool(torch.isfinite(y[0, 3, 4, 5]))
    dyb = dy.clone()
    dyb[0, 2, 3, 7] = float('nan')
    dx = _run_x3_block(x, params, dyb, d)[2]
    assert not bool(torch.isfinite(dx[0, 2, 3, 7]))
