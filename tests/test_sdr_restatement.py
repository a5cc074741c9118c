"""
CPU-only: a NumPy float64 restatement of the device SDR (csrc/sdr.hip) -- direct correlation sums taken chunk by chunk in the
kernel's chunk order, then the Levinson recursion for a general right-hand side -- held against the host yardstick
``signal_distortion_ratio`` (FFT correlations, dense solve) over the input set of tests/test_gpu_sdr.py.  This re-measures the
constant the GPU test's 1e-6 dB bar rests on: the two algorithms agree to <= 1e-8 dB on these inputs (4.1e-9 dB measured; 3.8e-9 dB on
the set the bar was derived from).
Also the API surface that needs no GPU.

``sdr_case`` / ``LENGTHS`` / ``restated_*`` are shared with tests/test_gpu_sdr.py.
"""

import numpy as np
import pytest
import torch
from scipy.signal import lfilter

from timbre_trap.utils import metrics
from timbre_trap.utils.metrics import signal_distortion_ratio, SDR_CHUNK as S

LENGTHS = (300, 511, 512, 513, S - 1, S, S + 1, S + 511, S + 512, 2 * S + 37, 66150)
POLES = (0.0, 0.9)
NOISE_DB = (0, -20, -60)


def sdr_case(n, pole, noise_db, seed=0):
    """Seeded fp32 pair (preds, target): target = white noise through 1 / (1 - pole z^-1); preds = 0.7 t + 0.2 t delayed by 3
    samples + white noise at ``noise_db`` relative to the target."""
    rng = np.random.default_rng([seed, n, int(pole * 10), -noise_db])
    t = lfilter([1.0], [1.0, -pole], rng.standard_normal(n)).astype(np.float32)
    noise = rng.standard_normal(n)
    noise *= np.linalg.norm(t.astype(np.float64)) / np.linalg.norm(noise) * 10.0 ** (noise_db / 20.0)
    delayed = np.concatenate([np.zeros(3), t[:-3].astype(np.float64)])
    p = (0.7 * t + 0.2 * delayed + noise).astype(np.float32)
    return p, t


def all_cases():
    return [(n, a, db) for n in LENGTHS for a in POLES for db in NOISE_DB]


def restated_correlations(p, t, L, zero_mean=False, chunk=S):
    """r[0..L), b[0..L), sum p^2 of one clip: float64 dot products per chunk of ``chunk`` samples of n, chunks added in
    ascending order (linear correlation: t[n + l], p[n + l] are zero beyond the end)."""
    p, t = p.astype(np.float64), t.astype(np.float64)
    if zero_mean:
        p, t = p - p.mean(), t - t.mean()
    n = len(t)
    tz, pz = np.concatenate([t, np.zeros(L)]), np.concatenate([p, np.zeros(L)])
    r, b, pp = np.zeros(L), np.zeros(L), 0.0
    for c0 in range(0, n, chunk):
        c1 = min(c0 + chunk, n)
        seg = t[c0:c1]
        r += np.array([np.dot(seg, tz[c0 + l:c1 + l]) for l in range(L)])
        b += np.array([np.dot(seg, pz[c0 + l:c1 + l]) for l in range(L)])
        pp += np.dot(p[c0:c1], p[c0:c1])
    return r, b, pp


def restated_levinson(r, b):
    """coh = b . h with Toeplitz(r) h = b, by the recursion of k_sdr_finish: prediction polynomial a (a[0] = 1), error E carried with
    its reciprocal (one division per step)."""
    L = len(r)
    a, h = np.zeros(L), np.zeros(L)
    a[0], E = 1.0, r[0]
    inv = 1.0 / E
    h[0] = b[0] * inv
    for k in range(1, L):
        rev = r[k:0:-1]                                   # r[k - i], i = 0 .. k-1
        acc, q = np.dot(a[:k], rev), np.dot(h[:k], rev)
        ref = -acc * inv
        E *= 1.0 - ref * ref
        inv = 1.0 / E
        a[:k + 1] = a[:k + 1] + ref * a[k::-1]            # a[i] + ref a[k - i], i = 0 .. k (a[k] = 0 before, a[0] stays 1)
        h[:k + 1] += (b[k] - q) * inv * a[k::-1]
    return float(np.dot(b, h))


def restated_sdr(p, t, L=512, zero_mean=False, load_diag=None):
    r, b, pp = restated_correlations(p, t, L, zero_mean)
    nt, npd = max(np.sqrt(r[0]), 1e-6), max(np.sqrt(pp), 1e-6)
    r, b = r / (nt * nt), b / (nt * npd)
    if load_diag is not None:
        r[0] += load_diag
    coh = restated_levinson(r, b)
    ratio = coh / (1.0 - coh)
    return 10.0 * np.log10(ratio) if ratio > 0 else -np.inf


def test_restatement_agrees_with_host_function():
    worst, where = 0.0, None
    lo, hi = np.inf, -np.inf
    for n, a, db in all_cases():
        p, t = sdr_case(n, a, db)
        ref = signal_distortion_ratio(p, t)
        got = restated_sdr(p, t)
        lo, hi = min(lo, ref), max(hi, ref)
        if abs(got - ref) > worst:
            worst, where = abs(got - ref), (n, a, db)
    print('restatement vs signal_distortion_ratio: worst %.3e dB at %s; SDR range %.1f .. %.1f dB' % (worst, where, lo, hi))
    assert hi < 60.0                                      # the inputs stay away from coh -> 1
    assert worst <= 1e-8


@pytest.mark.parametrize('kw', [dict(L=7), dict(L=100), dict(zero_mean=True), dict(load_diag=1e-3)])
def test_restatement_options(kw):
    p, t = sdr_case(S + 511, 0.9, -20)
    p = p + np.float32(0.25)                              # a mean for zero_mean to remove
    host = dict(kw)
    if 'L' in host:
        host['filter_length'] = host.pop('L')
    assert abs(restated_sdr(p, t, **kw) - signal_distortion_ratio(p, t, **host)) <= 1e-8


def test_chunk_order_only_moves_round_off():
    p, t = sdr_case(2 * S + 37, 0.9, -20)
    r1, b1, pp1 = restated_correlations(p, t, 512)
    r2, b2, pp2 = restated_correlations(p, t, 512, chunk=10 ** 9)
    assert np.abs(r1 - r2).max() <= 1e-13 * r1[0] and np.abs(b1 - b2).max() <= 1e-13 * r1[0] and abs(pp1 - pp2) <= 1e-13 * r1[0]


def test_api_surface():
    import timbre_trap.utils as u
    for name in ('signal_distortion_ratio', 'signal_distortion_ratio_device', 'SignalDistortionRatio'):
        assert hasattr(u, name), name
    assert u.signal_distortion_ratio_device is metrics.signal_distortion_ratio_device
    m = u.SignalDistortionRatio()
    assert isinstance(m, torch.nn.Module)
    assert (m.filter_length, m.zero_mean, m.load_diag) == (512, False, None)
    assert metrics.SDR_CHUNK >= 512 and metrics.SDR_MAX_FILTER == 512


def test_cpu_tensors_raise():
    import timbre_trap.utils as u
    x = torch.zeros(2, 1000)
    with pytest.raises(RuntimeError):
        u.signal_distortion_ratio_device(x, x)
    with pytest.raises(RuntimeError):
        u.SignalDistortionRatio()(x, x)
