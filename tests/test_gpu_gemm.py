"""
tt_gemm (csrc/gemm.hip) called directly, against a float64 einsum over the same strided storage, and the small helpers at the bottom
of csrc/conv_generic.hip (tt_dot, tt_scaled_add, tt_elu_bwd, tt_act_bwd) against float64.

tt_gemm is a general batched GEMM (transposes, leading dimensions, batch strides, bias modes, beta, reduce_batch, ELU) whose operands
are staged four ways -- 16 bytes along m / n (``avec`` / ``bvec``), 16 bytes along k (``akvec`` / ``bkvec``), or scalar -- decided per
workgroup from strides, pointer alignment and whether the tile is interior.  The model reaches it at a handful of shapes; here every
staging path, launches that mix them (interior tiles vector, edge tile scalar), misaligned bases and partial batch groups run on
their own.  reduce_batch at batch 65 and 130 makes the last group of batches partial (2 x 32 + 1, 3 x 43 + 1): a kernel that
did not clamp the group to the batch would add the finite matrix product that the test lays behind the last batch, at least 0.25
per term where the bar is at most 0.02.

Entries are uniform in +-[0.5, 1]: every product is at least 0.25, and the elementwise bar is the textbook bound of a length-K dot
product, K 2^-24 sum_k |a_mk| |b_kn| (at most 0.017 for K <= 528) -- a derivation, far below one dropped or doubled product.

Every check prints its ratio to the bar (pytest -rP).  Worst ones measured on an MI355X (matrix-instruction kernel): transposes 0.12,
mixed staging 0.06, k-contiguous 0.005, batch 0.08, alpha / beta / ldc 0.07, bias and ELU 0.33, reduce_batch 0.18, K = 1984 0.07;
tt_dot 0.04, tt_scaled_add 1.00 (its bar is the one rounding of the fma, which the worst element takes in full), tt_elu_bwd 0.29,
tt_act_bwd 0.42.
"""

import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
UNSUPPORTED = -2
ACT_NONE, ACT_ELU, ACT_RELU, ACT_SIGMOID = 0, 1, 2, 3
PAD = 8
VALU = os.environ.get('TTRAP_GEMM_VALU', '0') not in ('', '0')       # csrc/gemm.hip: the LDS-tiled kernel without matrix instructions


def _api():
    from timbre_trap import _hip
    return _hip.lib(), _hip.ptr, _hip.check, _hip.stream_ptr()


_worst = {}


def _note(key, ratio):
    _worst[key] = max(_worst.get(key, 0.0), ratio)
    print('ratio to bar: %-24s %.3f (worst so far %.3f)' % (key, ratio, _worst[key]))


def _pm(gen, *shape):
    """uniform in +-[0.5, 1]"""
    return (0.5 + 0.5 * torch.rand(*shape, generator=gen)) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)


class _Operand:
    """``vals`` (nb, rows, cols) laid out in a flat NaN-filled buffer: element (i, r, c) at off + i stride + r rs + c cs with
    (rs, cs) = (1, ld) if trans else (ld, 1) -- the addressing of include/ttrap.h.  stride 0: one matrix shared by the batch.
    The reference reads the SAME buffer through the same strides (as_strided on its float64 copy)."""

    def __init__(self, vals, trans, ld, stride, off, batch):
        nb, rows, cols = vals.shape
        self.rs, self.cs = (1, ld) if trans else (ld, 1)
        per = (cols if trans else rows) * ld
        assert ld >= (rows if trans else cols) and (stride >= per or (stride == 0 and nb == 1))
        buf = torch.full((off + (nb - 1) * stride + per,), float('nan'))
        torch.as_strided(buf, (nb, rows, cols), (stride, self.rs, self.cs), off).copy_(vals)
        self.logical = torch.as_strided(buf.double(), (batch, rows, cols), (stride, self.rs, self.cs), off)
        self.dev = buf.cuda()
        self.ptr = ctypes.c_void_p(self.dev.data_ptr() + 4 * off)
        self.host = buf


def _gemm(M, N, K, ta=0, tb=0, lda=None, ldb=None, ldc=None, batch=1, share_a=False, share_b=False, slack=0, a_off=0, b_off=0,
          reduce=0, alpha=1.0, beta=0.0, bias_mode=0, bias_div=0, act=ACT_NONE, seed=0, key='gemm', bar_rel_max=None):
    """One tt_gemm call checked elementwise; returns the result (batch or 1, M, N) for bitwise comparisons between variants."""
    lib, ptr, check, st = _api()
    gen = torch.Generator().manual_seed(seed)
    lda = lda or (M if ta else K)
    ldb = ldb or (K if tb else N)
    ldc = ldc or N
    guard = 1 if reduce else 0                           # a finite matrix behind the last batch: a group that runs past the batch adds it
    va = _pm(gen, 1 if share_a else batch + guard, M, K)
    vb = _pm(gen, 1 if share_b else batch + guard, K, N)
    sa = 0 if share_a else (K if ta else M) * lda + slack
    sb = 0 if share_b else (N if tb else K) * ldb + slack
    A = _Operand(va, ta, lda, sa, a_off, batch)
    B = _Operand(vb, tb, ldb, sb, b_off, batch)
    nc = 1 if reduce else batch
    sc = M * ldc + slack
    c0 = _pm(gen, nc, M, N)
    cbuf = torch.full(((nc - 1) * sc + M * ldc + PAD,), float('nan'))
    cview = torch.as_strided(cbuf, (nc, M, ldc), (sc, ldc, 1))
    if beta != 0.0:
        cview[:, :, :N] = c0
    cdev = cbuf.cuda()
    nbias = 0 if not bias_mode else (M if bias_mode == 1 else (M + bias_div - 1) // bias_div)
    bias = _pm(gen, nbias) if nbias else None
    bdev = bias.cuda() if nbias else None

    check(lib.tt_gemm(A.ptr, B.ptr, ptr(cdev), ptr(bdev), M, N, K, ta, tb, lda, ldb, ldc, batch, sa, sb, 0 if reduce else sc, reduce,
                      alpha, beta, bias_mode, bias_div, act, st), 'tt_gemm')
    torch.cuda.synchronize()

    acc = torch.einsum('bmk,bkn->bmn', A.logical, B.logical)
    S = torch.einsum('bmk,bkn->bmn', A.logical.abs(), B.logical.abs())
    c064 = c0.double() if beta != 0.0 else torch.zeros(nc, M, N, dtype=torch.float64)
    if reduce:
        groups = batch if VALU else -(-batch // -(-batch // 64))
        St = S.sum(0, keepdim=True)
        want = c064 + alpha * acc.sum(0, keepdim=True)
        # one dot product of length K batch in some order, the roundings of alpha and of the sum with what C held, and the atomics
        # of the groups, whose arrival order varies: 4 2^-24 |want| each
        bar = abs(alpha) * K * batch * U * St + 3 * U * (abs(alpha) * St + c064.abs()) + groups * 4 * U * want.abs()
    else:
        bterm = torch.zeros(M, dtype=torch.float64)
        if bias_mode == 1:
            bterm = bias.double()
        elif bias_mode == 2:
            bterm = bias.double()[torch.arange(M) // bias_div]
        bterm = bterm.view(1, M, 1)
        want = alpha * acc + bterm + beta * c064
        # the dot product, then one rounding each for alpha, the bias and beta C, each of a value no larger than the sum of the sizes
        bar = abs(alpha) * K * U * S + 3 * U * (abs(alpha) * S + bterm.abs() + abs(beta) * c064.abs())
        if act == ACT_ELU:
            want = torch.where(want > 0, want, torch.expm1(want))
            bar = bar + 4 * U * want.abs().clamp_min(1.0)      # 4 ulp of exp(v) <= 1 (its difference with 1 is exact or one more), or of v
    if bar_rel_max is not None:
        bar = torch.full_like(want, bar_rel_max * float(want.abs().max()))

    out = torch.as_strided(cdev.cpu(), (nc, M, ldc), (sc, ldc, 1))
    got = out[:, :, :N]
    assert bool(torch.isfinite(got).all()), 'non-finite result (beta = 0 must not read C)'
    assert bool(torch.isnan(out[:, :, N:]).all()), 'the padding columns of C were written'
    mask = torch.ones(cbuf.numel(), dtype=torch.bool)
    torch.as_strided(mask, (nc, M, N), (sc, ldc, 1)).fill_(False)
    assert bool(torch.isnan(cdev.cpu()[mask]).all()), 'wrote outside C'
    assert torch.equal(A.dev.cpu().nan_to_num(7.0), A.host.nan_to_num(7.0)) and torch.equal(B.dev.cpu().nan_to_num(7.0), B.host.nan_to_num(7.0))
    e = (got.double() - want).abs()
    ratio = float((e / bar).max())
    _note(key, ratio)
    assert bool((e <= bar).all()), '%s: %.3f of the bar (worst element off by %.3e)' % (key, ratio, float(e.max()))
    return got.clone()


@pytest.mark.parametrize('ta,tb', [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize('M,N,K', [(129, 130, 17), (64, 128, 16), (70, 200, 528), (1, 1, 1), (16, 257, 33)])
def test_transposes(M, N, K, ta, tb):
    """All four operand orders at tight leading dimensions: edge tiles in m, n and k; one exact tile (every staging path that the
    order allows: avec / bvec at (64, 128, 16), akvec / bkvec at K = 528); a single element; three column tiles."""
    _gemm(M, N, K, ta, tb, seed=M + N + K, key='transposes')


@pytest.mark.parametrize('N', [200, 260])
@pytest.mark.parametrize('tb', [0, 1])
def test_mixed_staging_of_b(N, tb, M=70):
    """ldb % 4 == 0 and N % 128 != 0: the interior column tiles stage B as vectors (along n for tb = 0, along k for tb = 1), the
    last tile as scalars -- in ONE launch.  The same operands with an odd ldb, and from a base pointer off by one float, stage
    everything as scalars; all three meet the same bar and the two scalar runs are bitwise equal."""
    K = 48 if tb else 50                                 # staging along k needs K % 16 == 0; along n the last k stage is partial
    tight = K if tb else N
    ld4 = (tight + 3) // 4 * 4
    v = _gemm(M, N, K, 0, tb, ldb=ld4, seed=N, key='mixed staging')
    s1 = _gemm(M, N, K, 0, tb, ldb=ld4 + 1, seed=N, key='mixed staging')
    s2 = _gemm(M, N, K, 0, tb, ldb=ld4, b_off=1, seed=N, key='mixed staging')
    assert torch.equal(s1, s2)
    del v


@pytest.mark.parametrize('M', [200, 260])
@pytest.mark.parametrize('ta', [0, 1])
def test_mixed_staging_of_a(M, ta, N=130):
    """The same for A: interior row tiles as vectors (along m for ta = 1, along k for ta = 0), the last row tile as scalars."""
    K = 50 if ta else 48
    tight = M if ta else K
    ld4 = (tight + 3) // 4 * 4
    _gemm(M, N, K, ta, 0, lda=ld4, seed=M, key='mixed staging')
    s1 = _gemm(M, N, K, ta, 0, lda=ld4 + 1, seed=M, key='mixed staging')
    s2 = _gemm(M, N, K, ta, 0, lda=ld4, a_off=1, seed=M, key='mixed staging')
    assert torch.equal(s1, s2)


@pytest.mark.parametrize('K', [528, 520])
def test_k_contiguous_operands(K, M=134, N=260):
    """A (M, K) and B (N, K) both k-contiguous, the weight-gradient form: K = 528 stages interior tiles 16 bytes along k and transposes
    on the LDS write; K = 520 (no multiple of 16) falls back to scalars.  Also with batch strides that are no multiple of 4."""
    _gemm(M, N, K, 0, 1, seed=K, key='k-contiguous')
    _gemm(M, N, K, 0, 1, batch=2, slack=2, seed=K, key='k-contiguous')


@pytest.mark.parametrize('share', ['a', 'b', 'none'])
def test_batch_strides(share, M=70, N=130, K=33):
    """Batch 3: one A for all batches (sa = 0), one B (sb = 0), and every stride set (with slack between the matrices)."""
    _gemm(M, N, K, 0, 0, batch=3, share_a=share == 'a', share_b=share == 'b', slack=8 if share == 'none' else 0, seed=3, key='batch')
    _gemm(M, N, K, 1, 1, batch=3, share_a=share == 'a', share_b=share == 'b', slack=8 if share == 'none' else 0, seed=4, key='batch')


@pytest.mark.parametrize('beta', [0.0, 1.0, 0.5])
def test_alpha_beta_and_ldc(beta, M=70, N=130, K=33):
    """alpha = 0.5 and beta C into a prefilled C; beta = 0 must not read C (it holds NaN); with ldc > N the padding columns keep
    their NaN."""
    _gemm(M, N, K, alpha=0.5, beta=beta, seed=5, key='alpha beta ldc')
    _gemm(M, N, K, alpha=0.5, beta=beta, ldc=N + 3, batch=2, slack=4, seed=6, key='alpha beta ldc')


@pytest.mark.parametrize('act', [ACT_NONE, ACT_ELU])
@pytest.mark.parametrize('bias_mode', [0, 1, 2])
def test_bias_and_elu(bias_mode, act, M=4 * 31, N=130, K=5):
    """bias per row, bias per group of 31 rows (the latent heads: one bias per channel, 31 rows each), ELU after the bias; K = 5 keeps
    the pre-activations of order 1, about half of them negative."""
    _gemm(M, N, K, bias_mode=bias_mode, bias_div=31 if bias_mode == 2 else 0, act=act, beta=1.0 if bias_mode == 1 else 0.0, seed=7 + bias_mode,
          key='bias elu')


@pytest.mark.parametrize('batch', [1, 3, 64, 65, 130])
def test_reduce_batch(batch, M=70, N=130, K=5):
    """C += sum over the batch, into a non-zero C.  The matrix-instruction kernel sums ceil(batch / 64) consecutive batches per
    workgroup: at 65 and 130 the last group is partial.  A finite matrix lies behind the last batch of A and of B, so a group that
    ran past the batch would add its product (at least 0.25 per term) instead of faulting."""
    _gemm(M, N, K, batch=batch, reduce=1, beta=1.0, seed=batch, key='reduce_batch')
    _gemm(M, N, K, 1, 1, batch=batch, reduce=1, beta=1.0, alpha=0.5, seed=batch + 1, key='reduce_batch')


def test_reduce_batch_with_three_k_stages(M=70, N=130, K=33):
    _gemm(M, N, K, batch=65, reduce=1, beta=1.0, seed=11, key='reduce_batch')


def test_reduce_batch_refuses_what_it_cannot_do(M=8, N=8, K=8):
    lib, ptr, check, st = _api()
    a, b, c, bias = (torch.ones(2, 8, 8, device='cuda') for _ in range(4))
    before = c.clone()

    def call(beta=1.0, bias_mode=0, act=ACT_NONE):
        return lib.tt_gemm(ptr(a), ptr(b), ptr(c), ptr(bias), M, N, K, 0, 0, K, N, N, 2, M * K, K * N, 0, 1, 1.0, beta, bias_mode, 1, act, st)
    assert call(bias_mode=1) == UNSUPPORTED
    assert call(bias_mode=2) == UNSUPPORTED
    assert call(act=ACT_ELU) == UNSUPPORTED
    assert call(beta=0.0) == UNSUPPORTED
    assert call(beta=0.5) == UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(c, before)
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(c[0], before[0] + 16.0)


def test_model_depth(M=128, N=130, K=1984):
    """The encoder head's depth, K = 1984 = 31 * 64, at the bar of test_latent_layers: 2e-5 of the largest output."""
    _gemm(M, N, K, 0, 0, ldb=132, seed=12, key='K = 1984', bar_rel_max=2e-5)


def _pytest_subprocess(env_extra, selection):
    """The kernel switch is read once per process: the other kernel runs in a child pytest."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-m', 'gpu', '-p', 'no:cacheprovider'] + selection, cwd=root, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    return r.stdout


@pytest.mark.slow          # the A/B kernel of the same entry point; the default kernel runs in the default selection
@pytest.mark.skipif(os.environ.get('TT_CHILD_PYTEST') == '1', reason='already inside the child run')
def test_valu_kernel_passes_the_same_tests():
    """TTRAP_GEMM_VALU=1: k_gemm, the LDS-tiled kernel without matrix instructions, against the same references and bars."""
    out = _pytest_subprocess(dict(TTRAP_GEMM_VALU='1', TT_CHILD_PYTEST='1'), ['tests/test_gpu_gemm.py'])
    assert ' passed' in out


# ---- the helpers at the bottom of csrc/conv_generic.hip -------------------------------------------------------------------------------
HELPER_SIZES = [1, 3, 4, 5, 1027, 4096 * 256 + 7]


def _check_elem(key, got, n, want, bar, what):
    torch.cuda.synchronize()
    assert bool(torch.isnan(got[n:]).all()), '%s: wrote past the end' % what
    got = got[:n].cpu()
    assert bool(torch.isfinite(got).all())
    e = (got.double() - want).abs()
    ratio = float((e / bar.clamp_min(1e-300)).max())
    _note(key, ratio)
    assert bool((e <= bar).all()), '%s: %.3f of the bar' % (what, ratio)


@pytest.mark.parametrize('n', HELPER_SIZES)
def test_dot_adds_to_out(n):
    """out += a . b within the textbook bound of a dot product.  What ``out`` held is one more term of the sum (the partial sums of the
    workgroups meet in it by atomic adds, each rounded at the size of the running total), so the bound is that of n + 1 terms:
    (n + 1) 2^-24 (sum |a| |b| + |out|).  That bound grows with n; a single non-zero product at either end of the vectors must come
    out exactly."""
    lib, ptr, check, st = _api()
    gen = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    out0 = 3.25
    out = torch.full((1 + PAD,), float('nan'), device='cuda')
    out[0] = out0
    ad, bd = a.cuda(), b.cuda()
    check(lib.tt_dot(ptr(ad), ptr(bd), ptr(out), n, st), 'tt_dot')
    want = torch.tensor([out0 + float((a.double() * b.double()).sum())], dtype=torch.float64)
    bar = torch.tensor([(n + 1) * U * (float((a.double() * b.double()).abs().sum()) + out0)], dtype=torch.float64)
    _check_elem('dot', out, 1, want, bar, 'tt_dot n %d' % n)
    for hot in {0, n - 1}:
        a1, b1 = torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
        a1[hot], b1[hot] = 3.0, -1.5
        out[0] = out0
        check(lib.tt_dot(ptr(a1), ptr(b1), ptr(out), n, st), 'tt_dot')
        torch.cuda.synchronize()
        assert float(out[0]) == out0 - 4.5, 'element %d of %d' % (hot, n)


@pytest.mark.parametrize('n', HELPER_SIZES)
def test_scaled_add(n):
    """y = a + s[idx] b in one fused multiply-add: one rounding, 2^-24 |want|; s NULL is 1, a NULL is 0."""
    lib, ptr, check, st = _api()
    gen = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    s = torch.tensor([float('nan'), float('nan'), 0.3, float('nan')])           # idx 2 of a 4-vector; no other entry may be read
    ad, bd, sd = a.cuda(), b.cuda(), s.cuda()
    for has_a, has_s in ((True, True), (True, False), (False, True), (False, False)):
        y = torch.full((n + PAD,), float('nan'), device='cuda')
        check(lib.tt_scaled_add(ptr(ad) if has_a else None, ptr(bd), ptr(sd) if has_s else None, 2, ptr(y), n, st), 'tt_scaled_add')
        want = (a.double() if has_a else 0.0) + (float(s[2]) if has_s else 1.0) * b.double()
        _check_elem('scaled_add', y, n, want, U * want.abs(), 'a %s s %s' % (has_a, has_s))
    assert torch.equal(ad.cpu(), a) and torch.equal(bd.cpu(), b)


def _saved_output(n, act, gen):
    """What the forward pass saved: y = act(x), with the values at which the derivative changes form."""
    x = 3.0 * torch.randn(n, generator=gen)
    if act == ACT_ELU:
        y = torch.where(x > 0, x, torch.expm1(x))
        y[0::7] = -1.0                                   # y -> -1: the derivative y + 1 goes to 0
        y[1::7] = -1.0 + 2.0 ** -24
        y[2::7] = 0.0
    elif act == ACT_RELU:
        y = torch.relu(x)                                # exact zeros in about half of the places
    elif act == ACT_SIGMOID:
        y = torch.sigmoid(x)
    else:
        y = x
    return y


def _act_grad64(dy, y, act):
    dy, y = dy.double(), y.double()
    if act == ACT_ELU:
        return dy * torch.where(y > 0, torch.ones_like(y), y + 1)
    if act == ACT_RELU:
        return torch.where(y > 0, dy, torch.zeros_like(dy))
    if act == ACT_SIGMOID:
        return dy * (1 - y) * y
    return dy


@pytest.mark.parametrize('act', [ACT_NONE, ACT_ELU, ACT_RELU, ACT_SIGMOID])
@pytest.mark.parametrize('n', HELPER_SIZES)
def test_act_bwd_from_the_saved_output(n, act):
    """tt_act_bwd (and tt_elu_bwd for ELU): dy act'(a) through the saved y = act(a) within 4e-7 relative of float64 from the same y."""
    lib, ptr, check, st = _api()
    gen = torch.Generator().manual_seed(n + act)
    y = _saved_output(n, act, gen)
    dy = torch.randn(n, generator=gen)
    want = _act_grad64(dy, y, act)
    if act == ACT_RELU and n >= 1027:
        assert int((y == 0).sum()) > 0
    yd, dd = y.cuda(), dy.cuda()
    g = torch.full((n + PAD,), float('nan'), device='cuda')
    check(lib.tt_act_bwd(ptr(dd), ptr(yd), ptr(g), n, act, st), 'tt_act_bwd')
    _check_elem('act_bwd', g, n, want, 4e-7 * want.abs(), 'tt_act_bwd act %d n %d' % (act, n))
    if act == ACT_ELU:
        g2 = torch.full((n + PAD,), float('nan'), device='cuda')
        check(lib.tt_elu_bwd(ptr(dd), ptr(yd), ptr(g2), n, st), 'tt_elu_bwd')
        _check_elem('elu_bwd', g2, n, want, 4e-7 * want.abs(), 'tt_elu_bwd n %d' % n)
    assert torch.equal(yd.cpu(), y) and torch.equal(dd.cpu(), dy)
