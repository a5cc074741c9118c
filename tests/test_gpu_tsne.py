"""
Exact t-SNE on the MI355X (csrc/tsne.hip: tt_tsne_affinities, tt_tsne_run; timbre_trap.utils.tsne_joint_probabilities / tsne /
latent_codes / plot_latents_device) against the NumPy restatement of tests/tsne_ref.py, which tests/test_tsne_restatement.py pins to
scikit-learn on the CPU.

The device adds in a fixed order of its own and uses its own exp / log, so it agrees with the restatement to float64 rounding, not bit
for bit; every bar below is derived from that rounding or from the restatement's own sensitivity (tests/test_tsne_restatement.py),
never from what the kernels give.  What the device promises about ITSELF -- symmetry of P, continuation, determinism -- is compared
with ``==``.  Wherever the C ABI is called directly every operand sits in the guarded arena of tests/cl16_ref.py.
"""

import numpy as np
import pytest
import torch

from timbre_trap import _hip
from timbre_trap.utils import TSNEResult, latent_codes, plot_latents_device, tsne, tsne_joint_probabilities

import tsne_ref as R
from cl16_ref import Arena

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F64 = torch.float64
P_BAR = 10 * R.AFFINITY_DEV_WORST            # elementwise relative, P and beta (test_tsne_restatement.test_affinity_bar: 3.5e-10)
EXPLORE, EXAGGERATION = 250, 12.0


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)             # a writable, contiguous copy (the cached operands are read-only)


def rel_dev(a, b):
    m = np.maximum(np.abs(a), np.abs(b))
    return float(np.max(np.abs(a - b) / np.where(m > 0, m, 1.0)))


# ---- the C ABI through the arena --------------------------------------------------------------------------------------------------------

def affinities_abi(x, perplexity, n=None, d=None):
    """tt_tsne_affinities on operands in the arena; (rc, arena).  ``n`` / ``d``: the sizes passed, where they are not x's own."""
    rows, cols = x.shape
    n, d = rows if n is None else n, cols if d is None else d
    nbytes = _hip.lib().tt_tsne_scratch_bytes(rows)
    a = Arena(device=DEV)
    a.inp('x', torch.from_numpy(np.array(x)))
    a.out('P', (rows, rows), F64)
    a.out('beta', (rows,), F64)
    a.scratch('scratch', max(nbytes, 64))
    a.build()
    rc = _hip.lib().tt_tsne_affinities(a.ptr('x'), int(x.dtype == np.float64), n, d, float(perplexity), a.ptr('P'), a.ptr('beta'),
                                      a.ptr('scratch'), _hip.stream_ptr())
    return rc, a


def run_abi(P, Y, U, gains, it0, it1, lr, n=None):
    """tt_tsne_run on operands in the arena; (rc, arena): Y, U, gains are in and out."""
    rows = Y.shape[0]
    n = rows if n is None else n
    a = Arena(device=DEV)
    a.inp('P', torch.from_numpy(np.array(P)))
    for name, v in (('Y', Y), ('U', U), ('gains', gains)):
        a.acc(name, torch.from_numpy(np.array(v)))
    a.out('kl', (1,), F64)
    a.out('gnorm', (1,), F64)
    a.scratch('scratch', max(_hip.lib().tt_tsne_scratch_bytes(rows), 64))
    a.build()
    rc = _hip.lib().tt_tsne_run(a.ptr('P'), n, a.ptr('Y'), a.ptr('U'), a.ptr('gains'), it0, it1, EXPLORE, EXAGGERATION, float(lr),
                               R.MOMENTA[0], R.MOMENTA[1], R.MIN_GAIN, a.ptr('kl'), a.ptr('gnorm'), a.ptr('scratch'), _hip.stream_ptr())
    return rc, a


# ---- affinities -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(R.affinity_cases()))
def test_affinities(name):
    """P and beta against the restatement at ten times the deviation one ulp in exp's argument causes in the restatement itself
    (P_BAR = 3.5e-10, elementwise relative); P symmetric bit for bit, zero diagonal, total 1 within N^2 ulp."""
    x, perp = R.affinity_cases()[name]
    want_P, want_beta, _ = R.affinity_want(name)
    rc, a = affinities_abi(x, perp)
    assert rc == 0
    a.verify(name)
    P, beta = a.get('P').numpy(), a.get('beta').numpy()
    n = len(P)
    print(name, 'P %.3e beta %.3e of the bar %.1e' % (rel_dev(P, want_P), rel_dev(beta, want_beta), P_BAR))
    assert rel_dev(beta, want_beta) <= P_BAR
    assert rel_dev(P, want_P) <= P_BAR
    assert np.array_equal(P, P.T)
    assert not P.diagonal().any() and (P[~np.eye(n, dtype=bool)] >= R.EPS).all()
    assert abs(P.sum() - 1.0) <= n * n * R.EPS


def test_affinities_python_surface():
    x, perp = R.affinity_cases()['N130_D3_p5_float32']
    _, a = affinities_abi(x, perp)
    P, beta = tsne_joint_probabilities(dev(x), perp)
    assert P.is_cuda and P.dtype == F64 and P.shape == (130, 130) and beta.dtype == F64 and beta.shape == (130,)
    assert torch.equal(P.cpu(), a.get('P')) and torch.equal(beta.cpu(), a.get('beta'))
    # 16-bit points are upcast to fp32
    P16, _ = tsne_joint_probabilities(dev(x).half(), perp)
    assert torch.equal(P16, tsne_joint_probabilities(dev(x).half().float(), perp)[0])
    with pytest.raises(RuntimeError):
        tsne_joint_probabilities(torch.from_numpy(np.array(x)), perp)
    with pytest.raises(RuntimeError):
        tsne(torch.from_numpy(np.array(x)))


def test_bad_arguments():
    lib = _hip.lib()
    assert lib.tt_version() >= 25
    assert lib.tt_tsne_scratch_bytes(1) == -1 and lib.tt_tsne_scratch_bytes(16385) == -1
    assert lib.tt_tsne_scratch_bytes(2) > 0 and lib.tt_tsne_scratch_bytes(16384) > 0
    x = R.gaussian(5, 3, 0)
    for perp, n, d in ((5.0, None, None), (7.0, None, None), (0.0, None, None), (float('nan'), None, None), (2.0, 1, None),
                       (2.0, 16385, None), (2.0, None, 0)):
        rc, a = affinities_abi(x, perp, n, d)
        assert rc == -1 and lib.tt_error_string(rc) == b'ttrap: bad argument', (perp, n, d)
        a.untouched((perp, n, d))
    P = R.joint_probabilities(x, 2)[0]
    Y = R.random_init(5, 0)
    for it0, it1, n in ((0, 1, 1), (0, 1, 16385), (2, 1, None), (-1, 1, None)):
        rc, a = run_abi(P, Y, np.zeros_like(Y), np.ones_like(Y), it0, it1, 50.0, n)
        assert rc == -1, (it0, it1, n)
        a.untouched((it0, it1, n))
    for perp in (5, 6.5, 0):
        with pytest.raises(ValueError):
            tsne_joint_probabilities(dev(x), perp)
        with pytest.raises(ValueError):
            tsne(dev(x), perplexity=perp)
    with pytest.raises(ValueError):
        tsne_joint_probabilities(dev(x[:1]), 2)
    with pytest.raises(ValueError):
        tsne_joint_probabilities(torch.zeros(16385, 1, device=DEV), 2)
    with pytest.raises(ValueError):
        tsne(dev(x), perplexity=2, init='spectral')


# ---- one step from a realistic state ----------------------------------------------------------------------------------------------------

def realistic_state(n):
    """Y of scale 10, a non-zero update, gains at the 0.01 floor, below 1 and above 1."""
    rs = np.random.RandomState(17 + n)
    return (10.0 * rs.standard_normal((n, 2)), 0.5 * rs.standard_normal((n, 2)),
            rs.choice([R.MIN_GAIN, R.MIN_GAIN, 0.4, 1.0, 1.8, 3.2], size=(n, 2)))


def step_bars(P, Y, e):
    """(gradient, its bar) at Y: what float64 rounding allows between two evaluations of grad_i = 4 sum_j (e p_ij - q_ij) w_ij
    (y_i - y_j) that add in different orders.  With u = EPS, a sum of n terms in any order is within n u sum |t| of the exact one; every
    term carries at most 16 roundings of its own; Z, a sum of N^2 positive terms, is within N^2 u relative, and that reaches the
    repulsive terms only: bar_i = 4 u ((N + 16) sum_j (|attractive_ij| + |repulsive_ij|) + N^2 sum_j |repulsive_ij|)."""
    n = len(Y)
    grad, w, z = R.kl_grad(P, Y, e, parts=True)
    distance = [np.abs(Y[:, None, k] - Y[None, :, k]) for k in range(2)]
    attractive = np.stack([((e * P * w) * d).sum(1) for d in distance], axis=1)
    repulsive = np.stack([((w / z * w) * d).sum(1) for d in distance], axis=1)
    return grad, 4.0 * R.EPS * ((n + 16) * (attractive + repulsive) + n * n * repulsive)


def check_step(P, lr, before, after, it, what):
    """``after`` = the device's (Y, U, gains) one iteration ``it`` after ``before``, against the restatement from the same ``before``.
    A gain hangs on the sign of U grad: the few components whose gradient lies within its own bar of 0 (none at the small shapes; at
    most 1 % allowed) are left out of the comparison, since rounding decides them."""
    e = EXAGGERATION if it < EXPLORE else 1.0
    grad, gbar = step_bars(P, before[0], e)
    sure = np.abs(grad) > gbar
    assert sure.mean() >= 0.99 and (sure.all() or len(P) > 1000) and (np.abs(before[1]) > 0).all()
    Y, U, gains = (v.copy() for v in before)
    R.step(P, Y, U, gains, it, EXPLORE, EXAGGERATION, lr)
    assert (gains == R.MIN_GAIN).any() and (gains > 1).any()
    assert np.abs(after[2] - gains)[sure].max() <= 2 * R.EPS * gains.max(), what
    ubar = lr * gains * gbar + 4 * R.EPS * (np.abs(U) + np.abs(before[1]))
    ybar = ubar + 4 * R.EPS * np.abs(Y)
    print(what, 'U %.3g Y %.3g of their bars' % ((np.abs(after[1] - U) / ubar)[sure].max(), (np.abs(after[0] - Y) / ybar)[sure].max()))
    assert (np.abs(after[1] - U) <= ubar)[sure].all(), what
    assert (np.abs(after[0] - Y) <= ybar)[sure].all(), what
    assert np.abs(U).max() > 1e3 * ubar.max()                                     # the bar is far below the step itself


def check_scalars(P, Y, got_kl, got_gnorm, what):
    """kl_out and gnorm_out against the restatement's KL and gradient at the same Y, at the float64 bar: KL is a sum of N^2 terms
    t = p log(p / q) whose q carries Z's N^2 u: (N^2 + 16) u (sum |t| + sum p); the norm: the norm of step_bars' bar plus 4 u of itself."""
    n = len(Y)
    kl, grad, terms = R.kl_grad(P, Y, terms=True)
    kl_bar = (n * n + 16) * R.EPS * (np.abs(terms).sum() + P.sum())
    gnorm = float(np.sqrt(np.sum(grad * grad)))
    gnorm_bar = float(np.sqrt(np.sum(step_bars(P, Y, 1.0)[1] ** 2))) + 4 * R.EPS * gnorm
    print(what, 'KL %.12f (device %.12f, bar %.2e); gradient norm %.6e (device %.6e, bar %.2e)' % (kl, got_kl, kl_bar, gnorm, got_gnorm, gnorm_bar))
    assert abs(got_kl - kl) <= kl_bar and kl_bar < 1e-6 * abs(kl), what
    assert abs(got_gnorm - gnorm) <= gnorm_bar and gnorm_bar < 1e-6 * gnorm, what


def state_of(a):
    return tuple(a.get(k).numpy() for k in ('Y', 'U', 'gains'))


@pytest.mark.parametrize('n', (64, 130, 300))
def test_one_step(n):
    """One iteration below the exploration boundary (exaggeration 12, momentum 0.5) and one above it (1, 0.8) at the float64 bar of
    step_bars; then iterations 249 and 250 in one call: equal, bit for bit, to the two made one by one, each of which is held to the
    restatement from the state the device itself started it from.  N = 130: three row tiles and three ranges of j; N = 300: two groups of
    256 rows in the sum that gives Z."""
    _, P, lr, _ = R.trajectory_operands(n)
    before = realistic_state(n)
    for it in (100, 300):
        rc, a = run_abi(P, *before, it, it + 1, lr)
        assert rc == 0
        a.verify(('step', n, it))
        check_step(P, lr, before, state_of(a), it, 'N %d iteration %d' % (n, it))
    _, a1 = run_abi(P, *before, 249, 250, lr)
    mid = state_of(a1)
    check_step(P, lr, before, mid, 249, 'N %d iteration 249' % n)
    _, a2 = run_abi(P, *mid, 250, 251, lr)
    check_step(P, lr, mid, state_of(a2), 250, 'N %d iteration 250' % n)
    rc, both = run_abi(P, *before, 249, 251, lr)
    assert rc == 0
    both.verify(('boundary', n))
    for k in ('Y', 'U', 'gains', 'kl', 'gnorm'):
        assert torch.equal(both.get(k), a2.get(k)), k


def test_one_step_many_ranges():
    """N = 4160 = 64 * 65: the first size with the full 64 ranges of more than 64 columns (65), 65 row tiles and 17 groups of rows.  P is a
    random symmetric matrix of the right kind (zero diagonal, sum 1, a wide spread of values), not an affinity matrix: the iteration
    does not care.  One iteration at the bar of step_bars, and the two scalars of that call at the bar of check_scalars."""
    n = 4160
    rs = np.random.RandomState(4160)
    P = rs.random_sample((n, n)) ** 8
    P = P + P.T
    np.fill_diagonal(P, 0.0)
    P = np.maximum(P / P.sum(), R.EPS)
    np.fill_diagonal(P, 0.0)
    before, lr = realistic_state(n), R.auto_learning_rate(n)
    rc, a = run_abi(P, *before, 100, 101, lr)
    assert rc == 0
    a.verify('many ranges')
    after = state_of(a)
    check_step(P, lr, before, after, 100, 'N %d iteration 100' % n)
    check_scalars(P, after[0], float(a.get('kl')), float(a.get('gnorm')), 'N %d' % n)


# ---- trajectory, continuation, determinism ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', R.TRAJECTORY_N)
def test_trajectory(n):
    """K = TRAJECTORY_K iterations from init='random' against the restatement at 1e-9 of max |Y|: the trajectory is chaotic, and K is
    the count at which the restatement's own response to a 1e-13 perturbation stays below that (test_tsne_restatement.test_sensitivity)."""
    x, P, lr, Y = R.trajectory_operands(n)
    Y, U, gains = Y.copy(), np.zeros_like(Y), np.ones_like(Y)
    R.run(P, Y, U, gains, 0, R.TRAJECTORY_K, EXPLORE, EXAGGERATION, lr)
    got = tsne(dev(x), perplexity=5, n_iter=R.TRAJECTORY_K, seed=0, init='random')
    assert isinstance(got, TSNEResult) and got.n_iter == R.TRAJECTORY_K and got.state.learning_rate == lr == 50.0
    assert got.embedding.is_cuda and got.embedding.dtype == F64 and got.embedding.shape == (n, 2)
    bar = 1e-9 * np.abs(Y).max()
    for name, want in (('Y', Y), ('U', U), ('gains', gains)):
        dev_v = getattr(got.state, name).cpu().numpy()
        print(n, name, '%.3e of max |Y|' % (np.abs(dev_v - want).max() / np.abs(Y).max()))
        assert np.abs(dev_v - want).max() <= bar, name
    assert torch.equal(got.embedding, got.state.Y)


def same_result(a, b):
    return all(torch.equal(u, v) for u, v in ((a.embedding, b.embedding), (a.state.U, b.state.U), (a.state.gains, b.state.gains),
                                              (a.kl_divergence, b.kl_divergence), (a.grad_norm, b.grad_norm)))


def test_continuation():
    """run(0, 10) then run(10, 20) equals run(0, 20) bit for bit; the state passed in is left as it was."""
    x = dev(R.trajectory_operands(130)[0])
    first = tsne(x, n_iter=10, init='random')
    kept = first.state.Y.clone()
    second = tsne(None, n_iter=20, state=first.state)
    whole = tsne(x, n_iter=20, init='random')
    assert second.n_iter == whole.n_iter == 20 and same_result(second, whole)
    assert torch.equal(first.state.Y, kept) and not torch.equal(kept, second.embedding)
    assert same_result(tsne(None, n_iter=20, state=second.state), second)        # nothing left to run: the same map and scalars
    with pytest.raises(ValueError):
        tsne(None, n_iter=5, state=first.state)


def test_determinism():
    x = dev(R.trajectory_operands(130)[0])
    a, b = tsne(x, n_iter=300), tsne(x, n_iter=300)
    assert same_result(a, b) and bool(torch.isfinite(a.embedding).all())
    assert float(a.embedding.abs().max()) > 1.0                                   # 300 iterations moved the 1e-4 start


# ---- 1000 iterations: KL, gradient norm, end to end -------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def embedded():
    x, labels = R.clusters(64)
    xd = dev(x)
    result = tsne(xd)                                                             # the defaults: perplexity 5, 1000 iterations, PCA start
    return x, labels, result


def test_kl_and_gradient_norm(embedded):
    """kl_out and gnorm_out after 1000 iterations against the restatement's KL and gradient at the DEVICE's final map (so the chaos of
    the trajectory does not enter), at the float64 bar of check_scalars."""
    _, _, result = embedded
    assert result.kl_divergence.is_cuda and result.kl_divergence.dim() == 0 and result.n_iter == 1000
    check_scalars(result.state.P.cpu().numpy(), result.embedding.cpu().numpy(), float(result.kl_divergence), float(result.grad_norm), 'N 64')


def test_end_to_end(embedded):
    """Four Gaussian clusters in 128 dimensions, N = 64: every point's three nearest neighbours in the map carry its label, and the final
    KL is at most the largest of the five restatement runs from starts perturbed by 1e-13 (E2E_KL = 0.350673, 0.302625, 0.335321, 0.335813,
    0.345824; test_tsne_restatement.test_end_to_end_cpu) plus 10 % for the spread the chaos allows."""
    x, labels, result = embedded
    P_want = R.joint_probabilities(x, 5)[0]
    assert rel_dev(result.state.P.cpu().numpy(), P_want) <= P_BAR
    assert R.neighbour_purity(result.embedding.cpu().numpy(), labels) == 1.0
    print('final KL %.6f' % float(result.kl_divergence))
    assert float(result.kl_divergence) <= 1.1 * max(R.E2E_KL)


# ---- surface ----------------------------------------------------------------------------------------------------------------------------

def test_latent_codes():
    from timbre_trap.framework import TimbreTrap
    torch.manual_seed(0)
    model = TimbreTrap(22050, 9, 60, 3, latent_size=None, model_complexity=1).to(DEV).eval()
    audio = torch.rand(2, 1, 30000, generator=torch.Generator().manual_seed(1)).to(DEV) * 2 - 1
    with torch.no_grad():
        latents = model.encode(model.sliCQ.pad_to_block_length(audio[:1]))[0]
        both = model.encode(model.sliCQ.pad_to_block_length(audio))[0]
    one = latent_codes(model, audio[:1])
    assert one.shape == (1, latents.shape[1]) and not one.requires_grad and torch.equal(one, latents.mean(-1))
    B, D, T = both.shape
    codes, clip = latent_codes(model, audio, pool=False)
    assert codes.shape == (B * T, D) and clip.dtype == torch.int64 and clip.tolist() == [0] * T + [1] * T
    assert torch.equal(codes[T + 3], both[1, :, 3]) and torch.equal(codes[T - 1], both[0, :, T - 1])


def test_plot_latents_device(tmp_path):
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    x, labels = R.clusters(40)
    names = np.array(['Violin', 'Clarinet', 'Saxophone', 'Bassoon'])[labels]
    path = tmp_path / 'latents.png'
    fig = plot_latents_device(dev(x).float(), list(names), save_path=str(path))
    try:
        assert path.stat().st_size > 0
        assert fig.get_suptitle() == 't-SNE Visualization of Latents Averaged Over Stems'
        assert sorted(t.get_text() for t in fig.gca().get_legend().get_texts()) == sorted(set(names))
        assert sum(len(c.get_offsets()) for c in fig.gca().collections) == 40
    finally:
        plt.close(fig)
