"""
Float64 NumPy restatement of exact t-SNE as include/ttrap.h states it (tt_tsne_affinities, tt_tsne_run; csrc/tsne.hip) and of the PCA
start of timbre_trap.utils.embedding.  Plain loops and matrix expressions, nothing chunked, scikit-learn's clamps kept.
tests/test_tsne_restatement.py pins this file to scikit-learn on the CPU; tests/test_gpu_tsne.py holds the kernels to it.

Where the device adds in a fixed order this file uses ``np.sum``: the two agree to float64 rounding, not bit for bit, and the bars of
the GPU file are derived from that.
"""

import functools

import numpy as np

EPS = np.finfo(np.float64).eps               # scikit-learn's MACHINE_EPSILON, DBL_EPSILON in the kernels
STEPS = 128                                  # evaluations of the perplexity search (TS_STEPS in csrc/tsne.hip)
MOMENTA = (0.5, 0.8)
MIN_GAIN = 0.01


def squared_distances(x):
    """d_ij = sum over d ascending of (x_id - x_jd)^2, each operation rounded on its own: symmetric bit for bit, zero diagonal."""
    x = np.asarray(x, dtype=np.float64)
    dist = np.zeros((x.shape[0], x.shape[0]))
    for d in range(x.shape[1]):
        t = x[:, None, d] - x[None, :, d]
        dist += t * t
    return dist


def search_row(d, target, steps=STEPS, exp=np.exp, tol=None):
    """scikit-learn's search for beta on the distances ``d`` of one row to the OTHER points: ``steps`` evaluations; ``tol``: scikit-learn's
    exit on |H - target| <= tol (None: the fixed-step form of the kernels).  Returns (beta, s, e) of the last evaluation."""
    beta, lo, hi = 1.0, -np.inf, np.inf
    for step in range(steps):
        e = exp(-(d * beta))
        s = np.sum(e)
        if s == 0.0:
            s = 1e-8
        if step == steps - 1:
            break
        h = np.log(s) + beta * (np.sum(d * e) / s)
        if tol is not None and abs(h - target) <= tol:
            break
        if h - target > 0.0:
            lo = beta
            beta = beta * 2.0 if hi == np.inf else (beta + hi) / 2.0
        else:
            hi = beta
            beta = beta / 2.0 if lo == -np.inf else (beta + lo) / 2.0
    return beta, s, e


def joint_probabilities(x, perplexity, steps=STEPS, exp=np.exp, tol=None, dist=None):
    """(P, beta, s): tt_tsne_affinities.  ``dist``: squared distances to use instead of those of ``x``."""
    dist = squared_distances(x) if dist is None else np.asarray(dist, dtype=np.float64)
    n = dist.shape[0]
    target = np.log(perplexity)
    cond = np.zeros((n, n))
    beta, s = np.zeros(n), np.zeros(n)
    for i in range(n):
        others = np.arange(n) != i
        beta[i], s[i], e = search_row(dist[i, others], target, steps, exp, tol)
        cond[i, others] = e / s[i]
    P = cond + cond.T
    total = max(np.sum(P), EPS)
    P = np.maximum(P / total, EPS)
    np.fill_diagonal(P, 0.0)
    return P, beta, s


def kl_grad(P, Y, e=1.0, parts=False, terms=False):
    """(KL, grad, Z) at Y with P exaggerated by ``e``, as scikit-learn's _kl_divergence forms them (Q clamped at EPS in both).
    ``parts``: (grad, w, Z) instead; ``terms``: (KL, grad, the N (N - 1) terms of KL) instead -- for the bars of the GPU file."""
    diff = Y[:, None, :] - Y[None, :, :]
    w = 1.0 / (1.0 + np.sum(diff * diff, axis=2))
    np.fill_diagonal(w, 0.0)
    z = np.sum(w)
    Q = np.maximum(w / z, EPS)
    off = ~np.eye(len(Y), dtype=bool)
    Pe = e * P
    pqd = np.where(off, (Pe - Q) * w, 0.0)
    grad = 4.0 * np.einsum('ij,ijk->ik', pqd, diff)
    if parts:
        return grad, w, z
    kl_terms = Pe[off] * np.log(np.maximum(Pe[off], EPS) / Q[off])
    kl = np.sum(kl_terms)
    return (kl, grad, kl_terms) if terms else (kl, grad, z)


def step(P, Y, U, gains, it, explore_iters, exaggeration, learning_rate, momenta=MOMENTA, min_gain=MIN_GAIN):
    """One iteration of scikit-learn's _gradient_descent, in place on Y, U, gains."""
    explore = it < explore_iters
    grad = kl_grad(P, Y, exaggeration if explore else 1.0, parts=True)[0]
    inc = U * grad < 0.0
    gains[inc] += 0.2
    gains[~inc] *= 0.8
    np.clip(gains, min_gain, np.inf, out=gains)
    U[...] = (momenta[0] if explore else momenta[1]) * U - learning_rate * (grad * gains)
    Y += U
    return grad


def run(P, Y, U, gains, it0, it1, explore_iters, exaggeration, learning_rate, momenta=MOMENTA, min_gain=MIN_GAIN):
    """tt_tsne_run: iterations it0 .. it1 - 1 in place, then (KL, gradient norm) of the final Y without exaggeration."""
    for it in range(it0, it1):
        step(P, Y, U, gains, it, explore_iters, exaggeration, learning_rate, momenta, min_gain)
    kl, grad, _ = kl_grad(P, Y)
    return kl, float(np.sqrt(np.sum(grad * grad)))


def auto_learning_rate(n, early_exaggeration=12.0):
    return max(n / early_exaggeration / 4.0, 50.0)


def random_init(n, seed):
    return (1e-4 * np.random.RandomState(seed).standard_normal((n, 2)).astype(np.float32)).astype(np.float64)


def pca_init(x):
    """The two leading principal components of ``x`` by numpy.linalg.svd of the centred data in float64.  Sign rule: in each of the two
    right singular vectors the entry of largest magnitude (the first of them on a tie) is positive.  Scaled so that the first column
    has standard deviation 1e-4 (numpy's default, ddof = 0)."""
    x = np.asarray(x, dtype=np.float64)
    xc = x - x.mean(axis=0)
    _, _, vt = np.linalg.svd(xc, full_matrices=False)
    k = min(2, vt.shape[0])
    v = vt[:k].copy()
    for r in range(k):
        if v[r, np.argmax(np.abs(v[r]))] < 0:
            v[r] = -v[r]
    y = np.zeros((x.shape[0], 2))
    y[:, :k] = xc @ v.T
    sd = np.std(y[:, 0])
    return y / sd * 1e-4 if sd > 0 else y


# ---- operands and constants shared by tests/test_tsne_restatement.py (which derives them) and tests/test_gpu_tsne.py -------------------

SHAPES = (40, 64, 200)                      # the reference's use and two sizes around it
P_GAP_WORST = 2.9e-6                        # measured by test_joint_probabilities_against_sklearn, relative to max(P)
TRAJECTORY_N = (64, 130)                    # the shapes of the GPU trajectory test
TRAJECTORY_K = 10                           # its iteration count: the largest of {5, 10, 20} that test_sensitivity lets through
AFFINITY_DEV_WORST = 3.5e-11                 # measured by test_affinity_bar; the GPU file asserts ten times this
MIN_S = 1e-250                              # every row of every GPU case ends its search with s above this (test_affinity_bar)
E2E_KL = (0.350673, 0.302625, 0.335321, 0.335813, 0.345824)      # the five restatement runs of test_end_to_end_cpu


def gaussian(n, d, seed):
    return np.random.RandomState(seed).standard_normal((n, d))


# ---- operands of the GPU affinity cases -------------------------------------------------------------------------------------------------

def spread_points(n, d, seed):
    """n points in d dimensions whose pairwise distances spread widely: a two-dimensional cloud mapped into d dimensions plus a tenth
    of its scale in every coordinate.  Independent Gaussian coordinates would not do at d = 128: their distances concentrate (256 +- 23),
    the search at perplexity 2 then ends where exp(-beta d) is subnormal, and there the result hangs on the last subnormal bit of exp --
    one ulp in its argument moved P by 28 % -- so that no bar can be derived from rounding (scikit-learn's search has the same property)."""
    rs = np.random.RandomState(seed)
    z = rs.standard_normal((n, min(d, 2)))
    return z @ rs.standard_normal((min(d, 2), d)) + 0.1 * rs.standard_normal((n, d))


@functools.lru_cache(maxsize=None)
def affinity_cases():
    """name -> (x, perplexity): N in {5, 64, 65, 130} x D in {1, 3, 128} x perplexity in {2, 5} (perplexity < N) x fp32 / fp64, one case
    with two identical points and one with an outlier 1e3 away, whose row sees exp underflow to 0 for the first ten halvings."""
    out = {}
    for n in (5, 64, 65, 130):
        for d in (1, 3, 128):
            for perp in (2, 5):
                if perp >= n:
                    continue
                for dt in (np.float32, np.float64):
                    out['N%d_D%d_p%d_%s' % (n, d, perp, dt.__name__)] = (spread_points(n, d, 1000 * n + 10 * d + perp).astype(dt), perp)
    x = spread_points(64, 3, 5)
    x[7] = x[3]
    out['identical'] = (x, 5)
    x = 30.0 * gaussian(64, 3, 6)
    x[0] = (1e3, 0.0, 0.0)
    out['outlier'] = (x, 5)
    for v in out.values():
        v[0].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def affinity_want(name):
    x, perp = affinity_cases()[name]
    return joint_probabilities(x, perp)


def trajectory_operands(n):
    """(P, learning rate, start) of the GPU trajectory test at N = n: perplexity 5, the automatic learning rate (50), init='random'."""
    x = gaussian(n, 16, n)
    return x, joint_probabilities(x, 5)[0], auto_learning_rate(n), random_init(n, 0)


def clusters(n):
    """Four Gaussian clusters in 128 dimensions: centres 2 N(0, 1), unit noise, RandomState(0); labels i mod 4."""
    rs = np.random.RandomState(0)
    centres = 2.0 * rs.standard_normal((4, 128))
    labels = np.arange(n) % 4
    return centres[labels] + rs.standard_normal((n, 128)), labels


def neighbour_purity(Y, labels, k=3):
    d = squared_distances(Y)
    np.fill_diagonal(d, np.inf)
    near = np.argsort(d, axis=1)[:, :k]
    return float((labels[near] == labels[:, None]).mean())
