"""
Exact t-SNE on the device (csrc/tsne.hip) against scikit-learn on the host of the same machine: four Gaussian clusters in D = 128
dimensions (centres 2 N(0, 1), unit noise), perplexity 5, 1000 iterations, PCA start.

    python tools/kb_tsne.py [--sizes 40 1024 4096 8192] [--iters 3] [--host-exact-max 1024] [--host-bh-max 4096]

One JSON line per N:
  affinities_ms   tsne_joint_probabilities (distances, 128-step search, symmetrisation) on points that are on the device, warm, host clock
                  between two device synchronisations, median / min / max over --iters
  run_ms          1000 iterations from a prepared state (P, start) through tsne(state=...), the same way; us_per_iter = run_ms / 1000
  tsne_ms         tsne() as a whole: affinities, the PCA start on the host (download, SVD, upload) and the 1000 iterations
  kl              KL(P || Q) of the device's final map
  sklearn_exact_s / sklearn_exact_kl / sklearn_exact_iters   TSNE(method='exact', perplexity=5, max_iter=1000, init='pca',
                  random_state=0).fit on the same points (float32, as experiments/latents.py hands them over), one run, up to
                  --host-exact-max points (it is O(N^2) per iteration on the host); n_iter_ tells where scikit-learn's early stop ended it
  sklearn_bh_s / sklearn_bh_kl   the same with method='barnes_hut' (an approximation; for context), up to --host-bh-max points
If scikit-learn does not import the host columns are null and ``sklearn`` says why.
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'timbre-trap_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def clusters(n, d=128):
    rs = np.random.RandomState(0)
    centres = 2.0 * rs.standard_normal((4, d))
    return (centres[np.arange(n) % 4] + rs.standard_normal((n, d))).astype(np.float32)


def timed(fn, iters):
    ms = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return tuple(round(v, 3) for v in (statistics.median(ms), min(ms), max(ms)))


def host(x, method):
    from sklearn.manifold import TSNE
    est = TSNE(n_components=2, perplexity=5, max_iter=1000, init='pca', method=method, random_state=0)
    t0 = time.perf_counter()
    est.fit(x)
    return round(time.perf_counter() - t0, 2), round(float(est.kl_divergence_), 4), int(est.n_iter_)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[40, 1024, 4096, 8192])
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--host-exact-max', type=int, default=1024)
    ap.add_argument('--host-bh-max', type=int, default=4096)
    args = ap.parse_args()
    from timbre_trap.utils import tsne, tsne_joint_probabilities
    try:
        import sklearn
        have = 'scikit-learn %s' % sklearn.__version__
    except Exception as e:                                    # noqa: BLE001
        sklearn, have = None, 'not importable here: %r' % (e,)
    dev = torch.device('cuda:0')
    for n in args.sizes:
        x = clusters(n)
        xd = torch.from_numpy(x).to(dev)
        start = tsne(xd, n_iter=0)                            # P and the PCA start; also the untimed first call
        tsne(None, n_iter=10, state=start.state)
        aff = timed(lambda: tsne_joint_probabilities(xd, 5), args.iters)
        done = []
        run = timed(lambda: done.append(tsne(None, n_iter=1000, state=start.state)), args.iters)
        whole = timed(lambda: tsne(xd), max(1, args.iters - 1))
        row = dict(n=n, d=x.shape[1], p_mb=round(n * n * 8 / 1e6, 1), affinities_ms=aff, run_ms=run, us_per_iter=round(run[0], 1),
                   tsne_ms=whole, kl=round(float(done[-1].kl_divergence), 4), grad_norm=float('%.3e' % float(done[-1].grad_norm)),
                   sklearn=have, sklearn_exact_s=None, sklearn_exact_kl=None, sklearn_exact_iters=None, sklearn_bh_s=None, sklearn_bh_kl=None)
        if sklearn is not None and n <= args.host_exact_max:
            row['sklearn_exact_s'], row['sklearn_exact_kl'], row['sklearn_exact_iters'] = host(x, 'exact')
        if sklearn is not None and n <= args.host_bh_max:
            row['sklearn_bh_s'], row['sklearn_bh_kl'], _ = host(x, 'barnes_hut')
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
