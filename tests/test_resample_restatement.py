"""
CPU-only: the tap design and the float64 yardstick of the device resampler (timbre_trap.utils.audio; csrc/resample.hip).

  * ``sinc_resample_kernel``: reduced rates, half-width and taps per phase of the rate pairs the datasets meet, computed by hand
    from the formula; unit DC gain of every phase.
  * ``resample_host`` (padded strided conv1d, float64) against ``defining_sum``: an independent per-output loop over
        y[q new + p] = sum_k h[p][k] x[q orig + k - w]
    with explicit bounds checks on the input index -- no padding, no conv1d, no transpose.  Both are float64 sums of the same K
    products in a different order, so they agree to K 2^-53 sum_k |h_k| |x_k| per output (the running-error bound of a K-term sum).
  * impulses come back as the fp32 taps exactly (one product per output), output lengths are ceil(new L / orig).
  * a known answer that guards the gross shape (ratio, scale, phase order), not the taps: a 1 kHz sine from 48 kHz to 22.05 kHz
    stays within 5e-4 of the sine sampled at 22.05 kHz (1.05e-4 measured; a wrong ratio or a missing scale gives > 1e-2).
  * the fp32 torch conv1d route on the CPU (torchaudio's own arithmetic) lies inside the bar the GPU test uses against
    ``resample_host``: K 2^-24 sum_k |h_k| |x_k|, the bound of a K-term fp32 dot product in any order, with or without fused
    multiply-add (0.012 of the bar measured at 320:147, L = 5003).

``RATIOS`` / ``noise`` / ``conv_route`` / ``magnitude`` / ``fp32_taps`` / ``impulse_expected`` are shared with tests/test_gpu_resample.py.
"""

import functools
import math

import numpy as np
import pytest
import torch

from timbre_trap.utils import audio
from timbre_trap.utils import sinc_resample_kernel, resample_host, resample, prepare_audio

# (from Hz, to Hz) -> (orig, new, width, K)
TABLE = {(44100, 22050): (2, 1, 13, 28), (48000, 22050): (320, 147, 14, 348), (16000, 22050): (320, 441, 7, 334),
         (32000, 22050): (640, 441, 9, 658), (96000, 22050): (640, 147, 27, 694), (11025, 22050): (1, 2, 7, 15), (3, 2): (3, 2, 10, 23)}
RATIOS = ((2, 1), (320, 147), (320, 441), (3, 2))          # the four classes: one phase, down, up, small


def fp32_taps(orig, new):
    """(float64 value of the fp32 taps [new][K], width)."""
    taps, width, o, n = sinc_resample_kernel(orig, new)
    assert (o, n) == (orig, new)
    return taps.astype(np.float32).astype(np.float64), width


@functools.lru_cache(maxsize=None)
def noise(L, B=1, seed=0):
    """Seeded Gaussian noise (B, L) as fp32; read-only."""
    x = np.random.default_rng([seed, L, B]).standard_normal((B, L)).astype(np.float32)
    x.setflags(write=False)
    return x


def out_len(L, orig, new):
    return -(-new * L // orig)


def conv_route(x, h, orig, width):
    """torchaudio's route in the dtype of the tensors given: x (B, L), h (new, K) -> (B, ceil(new L / orig))."""
    L, new = x.shape[-1], h.shape[0]
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(x[:, None], (width, width + orig)), h[:, None], stride=orig)
    return y.transpose(1, 2).reshape(x.shape[0], -1)[:, :out_len(L, orig, new)]


def magnitude(x, orig, new):
    """sum_k |h_k| |x_k| per output in float64, (B, Lout) ndarray: what every error bar here is a multiple of."""
    h, width = fp32_taps(orig, new)
    return conv_route(torch.from_numpy(np.abs(np.asarray(x, dtype=np.float64))), torch.from_numpy(np.abs(h)), orig, width).numpy()


def defining_sum(x, h, orig, new, width):
    """The defining sum, output by output; returns (y, sum |h| |x|)."""
    L, K = len(x), h.shape[1]
    n_out = out_len(L, orig, new)
    y, mag = np.zeros(n_out), np.zeros(n_out)
    for n in range(n_out):
        q, p = divmod(n, new)
        acc = m = 0.0
        for k in range(K):
            i = q * orig + k - width
            if i < 0 or i >= L:                                                  # zero extension: nothing to add
                continue
            acc += h[p, k] * x[i]
            m += abs(h[p, k] * x[i])
        y[n], mag[n] = acc, m
    return y, mag


def impulse_expected(L, m, orig, new):
    """Response to a unit impulse at m: y[q new + p] = h[p][m + w - q orig] where that index lies in [0, K), else 0 (fp32 taps)."""
    h, width = fp32_taps(orig, new)
    K = h.shape[1]
    y = np.zeros(out_len(L, orig, new))
    for n in range(len(y)):
        q, p = divmod(n, new)
        k = m + width - q * orig
        if 0 <= k < K:
            y[n] = h[p, k]
    return y


def lengths(orig):
    return sorted({L for L in (1, 5, orig - 1, orig, orig + 1, 5003) if L >= 1})


@pytest.mark.parametrize('rates', list(TABLE), ids=lambda r: '%d-%d' % r)
def test_table(rates):
    taps, width, orig, new = sinc_resample_kernel(*rates)
    assert (orig, new, width, taps.shape[1]) == TABLE[rates]
    assert taps.shape == (new, 2 * width + orig) and taps.dtype == np.float64
    assert sinc_resample_kernel(*rates)[0] is taps                              # cached
    sums = taps.astype(np.float32).astype(np.float64).sum(axis=1)
    print('%s: phase sums %.5f .. %.5f' % (rates, sums.min(), sums.max()))
    assert sums.min() >= 1.0 and sums.max() <= 1.0010


def test_phase_offsets_keep_their_float32_rounding():
    """p / new is a float32 quotient in torch before it meets the float64 sample grid: at 147 phases the taps differ from the
    all-float64 design by more than float64 rounding, and by no more than the rounding can move them: the quotient is off by at
    most 2^-24 (half an ulp below 1), the argument t of the windowed sinc by base times that, and |d/dt (sinc(pi t) window(t))|
    <= 1.37 + pi / 12 < 2 (the steepest slope of sinc, plus the window's slope under |sinc| <= 1), scaled by base / orig."""
    taps, width, orig, new = sinc_resample_kernel(48000, 22050)
    idx = np.arange(-width, width + orig, dtype=np.float64) / orig
    t = np.clip(((np.arange(0, -new, -1) / new)[:, None] + idx[None, :]) * new * 0.99, -6, 6)
    with np.errstate(invalid='ignore'):
        exact = np.where(t == 0, 1.0, np.sin(t * math.pi) / (t * math.pi)) * np.cos(t * math.pi / 12) ** 2 * (new * 0.99 / orig)
    diff = np.abs(taps - exact).max()
    base = new * 0.99
    print('float32 phase offsets move the taps by up to %.2e' % diff)
    assert 1e-12 < diff <= 2.0 ** -24 * base * 2.0 * (base / orig)


@pytest.mark.parametrize('orig,new', [(3, 2), (2, 1), (320, 147)])
def test_host_against_defining_sum(orig, new):
    h, width = fp32_taps(orig, new)
    K = h.shape[1]
    for L in lengths(orig):
        x = noise(L)[0].astype(np.float64)
        got = resample_host(x, orig, new)
        assert got.dtype == torch.float64 and got.shape == (out_len(L, orig, new),)
        ref, mag = defining_sum(x, h, orig, new, width)
        err, bar = np.abs(got.numpy() - ref), K * 2.0 ** -53 * mag
        print('%d:%d L = %d: worst |conv - loop| / bar = %.3f' % (orig, new, L, (err / np.maximum(bar, 1e-300)).max()))
        assert (err <= bar).all()
        assert np.abs(ref).max() > 0.01                                          # something was computed


@pytest.mark.parametrize('rates', list(TABLE), ids=lambda r: '%d-%d' % r)
def test_output_length(rates):
    orig, new = TABLE[rates][:2]
    for L in lengths(orig):
        y = resample_host(np.zeros((2, 3, L)), *rates)
        assert y.shape == (2, 3, math.ceil(new * L / orig))
    assert resample_host(np.ones((2, 7)), 22050, 22050).shape == (2, 7)


@pytest.mark.parametrize('orig,new', RATIOS)
def test_impulse(orig, new):
    L = 4 * orig + 37
    for m in (0, L // 2, L - 1):
        x = np.zeros(L)
        x[m] = 1.0
        got = resample_host(x, orig, new).numpy()
        want = impulse_expected(L, m, orig, new)
        assert np.count_nonzero(want) > 0
        assert np.array_equal(got, want)


def test_sine_known_answer():
    n = np.arange(48000)
    y = resample_host(np.sin(2 * math.pi * 1000.0 * n / 48000.0), 48000, 22050).numpy()
    assert y.shape == (22050,)
    want = np.sin(2 * math.pi * 1000.0 * np.arange(22050) / 22050.0)
    err = np.abs(y - want)[100:-100].max()
    print('1 kHz sine, 48000 -> 22050: worst error %.3e' % err)
    assert err <= 5e-4


@pytest.mark.parametrize('orig,new', RATIOS)
def test_fp32_conv_route_is_inside_the_gpu_bar(orig, new):
    h, width = fp32_taps(orig, new)
    K = h.shape[1]
    for L in (5, orig + 1, 5003):
        x = noise(L, 3)
        ref = resample_host(x, orig, new).numpy()
        got = conv_route(torch.from_numpy(np.array(x)), torch.from_numpy(h.astype(np.float32)), orig, width).numpy().astype(np.float64)
        bar = K * 2.0 ** -24 * magnitude(x, orig, new)
        ratio = (np.abs(got - ref) / np.maximum(bar, 1e-300)).max()
        print('%d:%d L = %d: worst |fp32 conv1d - float64| / bar = %.4f' % (orig, new, L, ratio))
        assert (np.abs(got - ref) <= bar).all()


def test_host_takes_tensors_and_arrays():
    x = noise(700, 2)
    a = resample_host(x, 48000, 22050)
    b = resample_host(torch.from_numpy(np.array(x)), 48000, 22050)
    c = resample_host(torch.from_numpy(np.array(x)).reshape(2, 1, 700), 48000, 22050)
    assert torch.equal(a, b) and torch.equal(a, c[:, 0]) and a.dtype == torch.float64
    assert torch.equal(resample_host(x * 2.0, 320, 147), a * 2.0)               # reduced rates name the same filter; exact scaling by 2


def test_argument_checks_without_a_gpu():
    x = torch.zeros(1, 1000)
    with pytest.raises(RuntimeError):                                           # no CPU fallback
        resample(x, 48000, 22050)
    with pytest.raises(RuntimeError):
        prepare_audio(torch.zeros(2, 1000), 48000, 22050)
    with pytest.raises(ValueError):
        resample(x, 44100.5, 22050)
    with pytest.raises(ValueError):
        resample(x, 48000, 22050, resampling_method='sinc_interp_kaiser')
    with pytest.raises(ValueError):
        resample(x, 1000, 999)                                                  # 1014 taps per phase: beyond the kernels' capacity
    with pytest.raises(ValueError):
        resample_host(np.zeros(10), 48000, 22050, resampling_method='kaiser_best')
    with pytest.raises(ValueError):
        sinc_resample_kernel(0, 22050)
    assert 2 * 27 + 640 <= audio.RESAMPLE_MAX_TAPS and 441 <= audio.RESAMPLE_MAX_PHASES


def test_stand_in_dataset_has_prepare_audio():
    from timbre_trap import datasets
    if datasets.REFERENCE_DATASETS is None:
        assert datasets.AudioDataset.prepare_audio is prepare_audio
    import timbre_trap.utils as u
    assert u.resample is resample and u.prepare_audio is prepare_audio and not hasattr(u, 'torchaudio')
