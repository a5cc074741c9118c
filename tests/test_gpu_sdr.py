"""
The device SDR (csrc/sdr.hip; timbre_trap.utils.signal_distortion_ratio_device / SignalDistortionRatio) on the MI355X against the
float64 host yardstick ``signal_distortion_ratio``, and its correlation sums against float64 dot products of the same fp32 values.

Bars (fixed by reasoning, not by what the kernels give):
  * correlations: 1e-13 r[0].  Every product of two fp32 values is exact in float64, so only the order of the additions differs
    between the kernel and np.dot: about 1e-14 relative at N <= 66150, while one dropped or doubled sample is >= 1e-6 r[0].
  * SDR: 1e-6 dB, more than 100 times what tests/test_sdr_restatement.py re-measures (<= 1e-8 dB) for direct sums + Levinson against
    FFTs + dense solve in float64 on these very inputs.
Lengths: below the filter length (300 < 512: lags beyond the signal are zero), around 512, around the kernel's chunk length S
(read from metrics.SDR_CHUNK), S + 511 / S + 512 (the halo just inside / just past the next chunk), more than two chunks, 3 s.
"""

import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from timbre_trap import _hip
from timbre_trap.utils import SignalDistortionRatio, signal_distortion_ratio, signal_distortion_ratio_device
from timbre_trap.utils.metrics import SDR_CHUNK as S, sdr_correlations

from test_sdr_restatement import LENGTHS, NOISE_DB, POLES, restated_correlations, sdr_case

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CORR_BAR = 1e-13          # times r[0]
SDR_BAR = 1e-6            # dB


@functools.lru_cache(maxsize=None)
def batch(n):
    """The six (pole, noise) clips of length n as one (6, n) fp32 pair; read-only."""
    ps, ts = zip(*[sdr_case(n, a, db) for a in POLES for db in NOISE_DB])
    p, t = np.stack(ps), np.stack(ts)
    p.setflags(write=False)
    t.setflags(write=False)
    return p, t


@functools.lru_cache(maxsize=None)
def host_sdr(n, filter_length=512, zero_mean=False, load_diag=None):
    p, t = batch(n)
    return signal_distortion_ratio(p, t, filter_length, zero_mean, load_diag)


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)             # a writable, contiguous copy (the cached batches are read-only)


@pytest.mark.parametrize('n', LENGTHS)
def test_correlations(n):
    p, t = batch(n)
    rb = sdr_correlations(dev(p), dev(t), 512).cpu().numpy()
    assert rb.shape == (6, 1025)
    worst = 0.0
    for i in range(6):
        r, b, pp = restated_correlations(p[i], t[i], 512, chunk=10 ** 9)        # whole-signal float64 dot products
        err = max(np.abs(rb[i, :512] - r).max(), np.abs(rb[i, 512:1024] - b).max(), abs(rb[i, 1024] - pp)) / r[0]
        worst = max(worst, err)
    print('N = %d: worst |device - float64 dot| / r[0] = %.2e' % (n, worst))
    assert worst <= CORR_BAR
    if n < 512:
        assert not rb[:, n:512].any() and not rb[:, 512 + n:1024].any()          # lags beyond the signal: exactly zero


def test_correlations_zero_mean():
    n = 2 * S + 37
    p, t = batch(n)
    p = p + np.float32(0.25)
    rb = sdr_correlations(dev(p), dev(t), 100, zero_mean=True).cpu().numpy()
    for i in range(6):
        r, b, pp = restated_correlations(p[i], t[i], 100, zero_mean=True, chunk=10 ** 9)
        assert max(np.abs(rb[i, :100] - r).max(), np.abs(rb[i, 100:200] - b).max(), abs(rb[i, 200] - pp)) <= CORR_BAR * r[0]


@pytest.mark.parametrize('n', LENGTHS)
def test_sdr_against_host(n):
    p, t = batch(n)
    got = signal_distortion_ratio_device(dev(p), dev(t))
    assert got.dtype == torch.float64 and got.is_cuda and got.shape == (6,)
    diff = np.abs(got.cpu().numpy() - host_sdr(n))
    print('N = %d: host SDR %s dB, worst |device - host| = %.2e dB' % (n, np.round(host_sdr(n), 2), diff.max()))
    assert diff.max() <= SDR_BAR


@pytest.mark.parametrize('n', (300, S + 511))
def test_batching_and_shapes(n):
    p, t = batch(n)
    p3, t3 = dev(p[1:4]), dev(t[1:4])
    flat = signal_distortion_ratio_device(p3, t3)
    nested = signal_distortion_ratio_device(p3.unsqueeze(1), t3.unsqueeze(1))
    assert flat.shape == (3,) and nested.shape == (3, 1)
    assert torch.equal(flat, nested[:, 0])
    rb3 = sdr_correlations(p3, t3)
    for i in range(3):
        single = signal_distortion_ratio_device(p3[i], t3[i])
        assert single.shape == ()
        assert torch.equal(single, flat[i])                                      # bit for bit
        assert torch.equal(sdr_correlations(p3[i], t3[i])[0], rb3[i])
    assert len(set(flat.tolist())) == 3                                          # different clips


@pytest.mark.parametrize('kw', [dict(filter_length=7), dict(filter_length=100), dict(filter_length=512), dict(zero_mean=True),
                                dict(load_diag=1e-3), dict(filter_length=100, zero_mean=True, load_diag=1e-3)],
                         ids=lambda kw: '-'.join('%s=%s' % kv for kv in kw.items()))
def test_options(kw):
    n = S + 511
    p, t = batch(n)
    p = p + np.float32(0.25)                                                     # a mean for zero_mean to remove
    ref = signal_distortion_ratio(p, t, **kw)
    got = signal_distortion_ratio_device(dev(p), dev(t), **kw).cpu().numpy()
    print('%s: worst |device - host| = %.2e dB' % (kw, np.abs(got - ref).max()))
    assert np.abs(got - ref).max() <= SDR_BAR


def test_argument_checks():
    x = torch.zeros(2, 1000, device=DEV)
    with pytest.raises(ValueError):
        signal_distortion_ratio_device(x, x, filter_length=513)
    with pytest.raises(ValueError):
        signal_distortion_ratio_device(x, x, filter_length=0)
    with pytest.raises(ValueError, match='signal_distortion_ratio'):
        signal_distortion_ratio_device(x.double(), x.double())
    with pytest.raises(ValueError):
        signal_distortion_ratio_device(x, x[:, :999])
    with pytest.raises(ValueError):
        signal_distortion_ratio_device(x, x[:1])


def test_c_abi_argument_checks():
    lib = _hip.lib()
    x = torch.zeros(2, 1000, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.float64, device=DEV)
    P, st = _hip.ptr, _hip.stream_ptr()
    assert lib.tt_sdr_chunk() == S
    assert lib.tt_sdr_scratch_bytes(2, 1000, 512) == 2 * 1025 * 8
    assert lib.tt_sdr_scratch_bytes(1, 2 * S + 1, 7) == 3 * 15 * 8
    for B, N, L in ((2, 1000, 0), (2, 1000, 513), (2, 0, 512), (0, 1000, 512)):
        assert lib.tt_sdr_scratch_bytes(B, N, L) == -1
        assert lib.tt_sdr_correlate(P(x), P(x), B, N, L, None, P(ws), P(ws), st) == -1
    assert lib.tt_sdr_finish(P(ws), 2, 513, ctypes.c_double(0.0), 0, P(ws), P(ws), st) == -1
    assert lib.tt_sdr_finish(P(ws), 2, 0, ctypes.c_double(0.0), 0, P(ws), P(ws), st) == -1
    assert lib.tt_sdr_means(P(x), P(x), 2, 0, P(ws), P(ws), st) == -1


def test_reproducible():
    p, t = batch(2 * S + 37)
    pd, td = dev(p), dev(t)
    assert torch.equal(sdr_correlations(pd, td), sdr_correlations(pd, td))
    for kw in ({}, dict(zero_mean=True)):
        assert torch.equal(signal_distortion_ratio_device(pd, td, **kw), signal_distortion_ratio_device(pd, td, **kw))


def test_module():
    n = S + 1
    p, t = batch(n)
    pd, td = dev(p), dev(t)
    values = signal_distortion_ratio_device(pd, td).cpu().numpy()
    module = SignalDistortionRatio().to(DEV)
    out = module(pd[:, None], td[:, None])                                       # (6, 1, N), the shape evaluate.py passes
    assert out.dim() == 0 and out.dtype == torch.float32 and out.is_cuda
    assert abs(out.item() - values.mean()) <= 2.0 ** -23 * abs(values.mean())
    # update / compute / reset over two batches
    module.reset()
    module.update(pd[:2], td[:2])
    module.update(pd[2:], td[2:])
    total = module.compute()
    assert total.dtype == torch.float64 and abs(total.item() - values.mean()) <= 1e-12 * abs(values.mean())
    module.reset()
    module.update(pd[4:], td[4:])
    assert abs(module.compute().item() - values[4:].mean()) <= 1e-12 * abs(values[4:].mean())
    # options reach the kernels
    short = SignalDistortionRatio(filter_length=7, zero_mean=True, load_diag=1e-3).to(DEV)(pd, td)
    assert abs(short.item() - signal_distortion_ratio(p, t, 7, True, 1e-3).mean()) <= 1e-5


def test_half_inputs_are_upcast():
    p, t = batch(513)
    for dtype in (torch.float16, torch.bfloat16):
        ph, th = dev(p).to(dtype), dev(t).to(dtype)
        assert torch.equal(signal_distortion_ratio_device(ph, th), signal_distortion_ratio_device(ph.float(), th.float()))
        assert SignalDistortionRatio().to(DEV)(ph, th).dtype == dtype


def test_all_zero_target_is_not_an_error():
    p, _ = batch(513)
    got = signal_distortion_ratio_device(dev(p[:1]), torch.zeros(1, 513, device=DEV))
    torch.cuda.synchronize()
    assert not math.isfinite(got.item())
