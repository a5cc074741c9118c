"""
Latent codes in two dimensions: exact t-SNE on the device (csrc/tsne.hip), which is what ``experiments/latents.py`` asks of
scikit-learn through ``plot_latents`` (reference utils/visualization.py:139-144) -- a call the installed scikit-learn (>= 1.7) refuses,
because ``TSNE`` lost its ``n_iter`` keyword -- and what the host route does not reach: the thousands of per-frame codes of a few
tracks, which are on the device already.

  tsne_joint_probabilities   the symmetric joint probabilities P and the per-point precisions beta      (tt_tsne_affinities)
  tsne                       scikit-learn's ``method='exact'`` gradient descent on P                     (tt_tsne_run)
  latent_codes               the codes of a model for a batch of clips, time-averaged or per frame
  plot_latents_device        the reference figure, embedded with ``tsne``; only the N x 2 map is downloaded

The arithmetic is stated in include/ttrap.h and restated in NumPy by tests/tsne_ref.py: float64 throughout, every sum in an order that
depends on N alone, so equal inputs give equal bits and a run continued from its ``state`` equals the run made in one piece.
Differences from scikit-learn: the perplexity search runs a fixed 128 steps instead of stopping at an entropy error of
1e-5; it sees float64 distances, not float32; the descent has no early stop and runs exactly the iterations asked for; the 'pca' start
is the full SVD with a fixed sign rule, not the randomized solver; ``kl_divergence`` belongs to the final map, not the one before the
last update.
"""

from collections import namedtuple

import numpy as np
import torch

from .. import _hip

__all__ = ['TSNEResult', 'TSNEState', 'tsne_joint_probabilities', 'tsne', 'latent_codes', 'plot_latents_device']

MAX_POINTS = 16384
MOMENTA = (0.5, 0.8)
MIN_GAIN = 0.01

TSNEState = namedtuple('TSNEState', ('P', 'Y', 'U', 'gains', 'n_iter', 'learning_rate', 'early_exaggeration', 'exploration_iters'))
TSNEState.__doc__ = """What ``tsne(..., state=...)`` continues from: the joint probabilities ``P`` (N x N), the map ``Y``, the update ``U``
and the ``gains`` (each N x 2), float64 device tensors; the number of iterations done, and the three settings the run was started with."""
TSNEResult = namedtuple('TSNEResult', ('embedding', 'kl_divergence', 'grad_norm', 'n_iter', 'state'))
TSNEResult.__doc__ = """``embedding``: N x 2 float64 device tensor.  ``kl_divergence``, ``grad_norm``: 0-dim float64 device tensors, KL(P || Q)
and the norm of its gradient at ``embedding``, both without exaggeration (no value is downloaded to form them).  ``n_iter``: iterations
done in total.  ``state``: a ``TSNEState``."""


def _points(x):
    _hip.require_cuda(x)
    if x.dim() != 2:
        raise ValueError('expected points as an (N, D) tensor, got shape %s' % (tuple(x.shape),))
    if x.dtype != torch.float64:
        x = x.float()
    return x.detach().contiguous()


def _check_n(n):
    if n < 2 or n > MAX_POINTS:
        raise ValueError('t-SNE on the device takes 2 <= N <= %d points (got %d)' % (MAX_POINTS, n))


def _scratch(n, dev):
    return torch.empty(_hip.lib().tt_tsne_scratch_bytes(n) // 8, dtype=torch.float64, device=dev)


def tsne_joint_probabilities(x, perplexity):
    """
    ``(P, beta)`` for the points ``x`` (N, D), a CUDA tensor (fp32 or fp64; 16-bit is upcast to fp32): the joint probabilities
    scikit-learn's exact t-SNE descends on, N x N float64, symmetric bit for bit, zero on the diagonal, summing to 1, and the precision
    of every point's Gaussian, N float64.  ``ValueError`` unless 2 <= N <= 16384, D >= 1 and 0 < perplexity < N; CPU tensors raise
    ``RuntimeError``.
    """
    x = _points(x)
    n, d = x.shape
    _check_n(n)
    perplexity = float(perplexity)
    if d < 1 or not 0.0 < perplexity < n:
        raise ValueError('need D >= 1 and 0 < perplexity < N (got D = %d, perplexity = %r, N = %d)' % (d, perplexity, n))
    P = torch.empty(n, n, dtype=torch.float64, device=x.device)
    beta = torch.empty(n, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        scratch = _scratch(n, x.device)
        _hip.check(_hip.lib().tt_tsne_affinities(_hip.ptr(x), int(x.dtype == torch.float64), n, d, perplexity, _hip.ptr(P), _hip.ptr(beta),
                                                 _hip.ptr(scratch), _hip.stream_ptr()), 'tt_tsne_affinities')
    return P, beta


def _pca_start(x):
    """Host, once, N x D: the two leading principal components by ``numpy.linalg.svd`` of the centred data in float64; in each of the two
    right singular vectors the entry of largest magnitude is made positive; scaled so that the first column has standard deviation 1e-4."""
    x = x.double().cpu().numpy()
    xc = x - x.mean(axis=0)
    vt = np.linalg.svd(xc, full_matrices=False)[2]
    k = min(2, vt.shape[0])
    v = vt[:k].copy()
    for r in range(k):
        if v[r, np.argmax(np.abs(v[r]))] < 0:
            v[r] = -v[r]
    y = np.zeros((x.shape[0], 2))
    y[:, :k] = xc @ v.T
    sd = np.std(y[:, 0])
    return y / sd * 1e-4 if sd > 0 else y


def _run(state, it1):
    n, dev = state.Y.shape[0], state.Y.device
    Y, U, gains = state.Y.clone(), state.U.clone(), state.gains.clone()
    out = torch.empty(2, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        scratch = _scratch(n, dev)
        _hip.check(_hip.lib().tt_tsne_run(_hip.ptr(state.P), n, _hip.ptr(Y), _hip.ptr(U), _hip.ptr(gains), state.n_iter, it1,
                                          state.exploration_iters, state.early_exaggeration, state.learning_rate, MOMENTA[0], MOMENTA[1],
                                          MIN_GAIN, _hip.ptr(out[0:]), _hip.ptr(out[1:]), _hip.ptr(scratch), _hip.stream_ptr()), 'tt_tsne_run')
    return TSNEResult(Y, out[0], out[1], it1, state._replace(Y=Y, U=U, gains=gains, n_iter=it1))


def tsne(x, perplexity=5, n_iter=1000, seed=0, init='pca', learning_rate='auto', early_exaggeration=12.0, exploration_iters=250, state=None):
    """
    Exact t-SNE of the points ``x`` (N, D), a CUDA tensor, in two dimensions, on the device: scikit-learn's ``TSNE(method='exact')``
    with its momenta (0.5 while exaggerating, then 0.8), gains and ``min_gain`` 0.01.  Returns a ``TSNEResult``.

    ``n_iter``: the iteration at which the run ends.  There is no early stop: exactly ``n_iter`` iterations run (scikit-learn may stop
    sooner on its progress checks), all enqueued by one call without a host round trip.  ``learning_rate='auto'``:
    ``max(N / early_exaggeration / 4, 50)``.  ``init``: ``'pca'`` (the two leading principal components, formed on the host in float64
    by ``numpy.linalg.svd`` of the centred data, the entry of largest magnitude of each right singular vector made positive, scaled so
    that the first column has standard deviation 1e-4), ``'random'`` (``1e-4 * RandomState(seed).standard_normal((N, 2))`` drawn as
    float32 like scikit-learn's) or an (N, 2) tensor taken as the start.

    ``state`` (the ``state`` of an earlier result): continue that run from its iteration to ``n_iter``; ``x`` and every other argument are
    then ignored, and the result equals bit for bit the run made in one piece.  The state passed in is left unchanged.

    ``ValueError`` for N outside [2, 16384] or a perplexity outside (0, N); CPU tensors raise ``RuntimeError``: there is no CPU fallback.
    """
    n_iter = int(n_iter)
    if state is not None:
        for t in state[:4]:
            _hip.require_cuda(t)
        if n_iter < state.n_iter:
            raise ValueError('the state stands at iteration %d, beyond n_iter = %d' % (state.n_iter, n_iter))
        return _run(state, n_iter)
    x = _points(x)
    n, dev = x.shape[0], x.device
    if n_iter < 0 or int(exploration_iters) < 0:
        raise ValueError('n_iter and exploration_iters must not be negative')
    P, _ = tsne_joint_probabilities(x, perplexity)
    if isinstance(learning_rate, str):
        if learning_rate != 'auto':
            raise ValueError("learning_rate: a positive number or 'auto' (got %r)" % (learning_rate,))
        learning_rate = max(n / float(early_exaggeration) / 4.0, 50.0)
    learning_rate, early_exaggeration = float(learning_rate), float(early_exaggeration)
    if not learning_rate > 0 or not early_exaggeration > 0:
        raise ValueError('learning_rate and early_exaggeration must be positive')
    if isinstance(init, str):
        if init == 'pca':
            Y = torch.from_numpy(_pca_start(x)).to(dev)
        elif init == 'random':
            Y = torch.from_numpy((1e-4 * np.random.RandomState(seed).standard_normal((n, 2)).astype(np.float32)).astype(np.float64)).to(dev)
        else:
            raise ValueError("init: 'pca', 'random' or an (N, 2) tensor (got %r)" % (init,))
    else:
        _hip.require_cuda(init)
        if tuple(init.shape) != (n, 2):
            raise ValueError('init must have shape (%d, 2), got %s' % (n, tuple(init.shape)))
        Y = init.detach().to(device=dev, dtype=torch.float64).contiguous()
    start = TSNEState(P, Y, torch.zeros_like(Y), torch.ones_like(Y), 0, learning_rate, early_exaggeration, int(exploration_iters))
    return _run(start, n_iter)


def latent_codes(model, audio, pool=True):
    """
    The latent codes of ``audio`` (B, 1, N) under ``model``, as ``experiments/latents.py:111-119`` forms them: ``pad_to_block_length``,
    ``model.encode``, no gradients.  ``pool=True``: the time averages ``latents.mean(-1)``, (B, D).  ``pool=False``: every frame's code,
    ``(codes (B T, D), clip (B T) int64)`` with ``clip[r]`` the clip row r came from (frames of a clip in order).
    """
    with torch.no_grad():
        latents = model.encode(model.sliCQ.pad_to_block_length(audio))[0]
    if pool:
        return latents.mean(-1)
    B, D, T = latents.shape
    codes = latents.permute(0, 2, 1).reshape(B * T, D)
    return codes, torch.arange(B, device=latents.device).repeat_interleave(T)


def plot_latents_device(latents, labels, seed=0, perplexity=5, fig=None, save_path=None):
    """
    ``plot_latents`` of the reference (utils/visualization.py:109-185: same layout, same title) with the embedding formed on the device by
    ``tsne(latents, perplexity, 1000, seed)`` instead of scikit-learn on the host; only the N x 2 map is downloaded.  ``latents``: a CUDA
    tensor (L, D); ``labels``: L labels.  Returns the figure.
    """
    import matplotlib.pyplot as plt

    points = tsne(latents, perplexity=perplexity, n_iter=1000, seed=seed).embedding.cpu().numpy()
    if fig is None:
        fig = plt.figure(figsize=(9, 6), tight_layout=True)
    ax = fig.gca()
    labels = np.array(labels)
    for label in np.unique(labels):
        idcs = labels == label
        ax.scatter(points[idcs, 0], points[idcs, 1], label=label, s=40)
    ax.legend()
    ax.spines['left'].set_position('center')
    ax.spines['bottom'].set_position('center')
    ax.spines['right'].set_color('none')
    ax.spines['top'].set_color('none')
    ax.xaxis.set_ticks_position('bottom')
    ax.yaxis.set_ticks_position('left')
    for tick in ax.xaxis.get_ticklabels()[::2] + ax.yaxis.get_ticklabels()[::2]:
        tick.set_visible(False)
    fig.suptitle('t-SNE Visualization of Latents Averaged Over Stems')
    if save_path is not None:
        fig.savefig(save_path, bbox_inches='tight', pad_inches=0)
    return fig
