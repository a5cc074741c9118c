"""
The device resampler (csrc/resample.hip; timbre_trap.utils.resample / mix_resample / prepare_audio) on the MI355X against the
float64 host yardstick ``resample_host``, which applies the same fp32 taps.

Bars (fixed by reasoning, not by what the kernels give):
  * noise: K 2^-24 sum_k |h_k| |x_k| per output, formed in float64 -- the running-error bound of a K-term fp32 dot product in any
    order, with or without fused multiply-add.  tests/test_resample_restatement.py holds torch's own fp32 conv1d to the same bar.
  * impulses: bit-exact, an output is one product of 1.0 and an fp32 tap plus zeros.
  * fused mono mix: C = 1 and C = 2 bit-equal to resample(x.mean(-2)) (x / 1 and (a + b) / 2 are exact in either form); C = 3 against
    float64 with (K + 3) 2^-24 sum_k |h_k| mean_c |x_{c,k}|: two additions and a division, three more roundings of relative size
    2^-24 on every input of the dot product.
  * prepare_audio: bit-equal to r / r.abs().max() formed by torch on the device from the kernel's own r (IEEE division both ways).
Lengths: 1; 5 (below the half-width); around orig (one frame); around tile orig (one workgroup) for the tile of the kernel that
serves the ratio and, for the small ratios, also for the general kernel's; more than three workgroups.
"""

import math

import numpy as np
import pytest
import torch

from timbre_trap import _hip
from timbre_trap.utils import resample, resample_host, prepare_audio, sinc_resample_kernel
from timbre_trap.utils import audio
from timbre_trap.utils.audio import mix_resample, resample_tiles

from test_resample_restatement import RATIOS, impulse_expected, magnitude, noise, out_len

pytestmark = pytest.mark.gpu

DEV = 'cuda'
EPS = 2.0 ** -24


def is_direct(orig, new):
    return new <= 4 and orig <= 8


def seam(orig, new):
    """Input samples per workgroup of the kernel that serves the ratio (the tiles are compile-time constants of the library, mirrored
    in utils.audio and checked against the library on first use; test ids cannot wait for the library)."""
    return (audio.RESAMPLE_DIRECT_TILE if is_direct(orig, new) else audio.RESAMPLE_TILE) * orig


def cases():
    out = []
    for orig, new in RATIOS:
        ls = {1, 5, orig - 1, orig, orig + 1}
        for s in {seam(orig, new), audio.RESAMPLE_TILE * orig}:
            ls |= {s - 1, s, s + 1, 3 * s + 17}
        out += [(orig, new, L) for L in sorted(ls) if L >= 1]
    return out


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def same_bits(a, b):
    """Equal including the sign of zero, NaN equal to NaN."""
    both_nan = a.isnan() & b.isnan()
    return a.shape == b.shape and a.dtype == b.dtype and bool((both_nan | ((a == b) & (a.signbit() == b.signbit()))).all())


def test_tiles_match_the_library():
    lib = _hip.lib()
    assert resample_tiles() == (lib.tt_resample_tile(), lib.tt_resample_direct_tile()) == (audio.RESAMPLE_TILE, audio.RESAMPLE_DIRECT_TILE)


@pytest.mark.parametrize('orig,new,L', cases())
def test_noise_against_host(orig, new, L):
    x = noise(L, 3)
    K = 2 * sinc_resample_kernel(orig, new)[1] + orig
    got = resample(dev(x), orig, new)
    assert got.shape == (3, out_len(L, orig, new)) and got.dtype == torch.float32 and got.is_cuda
    ref = resample_host(x, orig, new).numpy()
    err, bar = np.abs(got.cpu().numpy().astype(np.float64) - ref), K * EPS * magnitude(x, orig, new)
    print('%d:%d L = %d: worst |device - float64| / bar = %.4f' % (orig, new, L, (err / np.maximum(bar, 1e-300)).max()))
    assert (err <= bar).all()
    assert np.abs(ref).max() > 1e-3


@pytest.mark.parametrize('orig,new', RATIOS)
def test_impulse(orig, new):
    s, t = seam(orig, new), audio.RESAMPLE_TILE * orig
    L = 2 * s + 37
    for m in (0, L // 2, L - 1, s - 1, s, t - 1, t):
        x = np.zeros((1, L), dtype=np.float32)
        x[0, m] = 1.0
        got = resample(dev(x), orig, new).cpu().numpy()[0]
        want = impulse_expected(L, m, orig, new).astype(np.float32)
        assert np.count_nonzero(want) > 0
        assert np.array_equal(got, want), 'impulse at %d' % m


@pytest.mark.parametrize('orig,new', RATIOS)
def test_fused_mono_mix(orig, new):
    L = seam(orig, new) + 3
    K = 2 * sinc_resample_kernel(orig, new)[1] + orig
    for C in (1, 2):
        x = dev(noise(L, 2 * C, seed=C)).reshape(2, C, L)
        assert torch.equal(mix_resample(x, orig, new), resample(x.mean(-2), orig, new))
    x = noise(L, 6, seed=3).reshape(2, 3, L)
    got = mix_resample(dev(x), orig, new).cpu().numpy().astype(np.float64)
    x64 = x.astype(np.float64)
    ref = resample_host(x64.mean(-2), orig, new).numpy()
    bar = (K + 3) * EPS * magnitude(np.abs(x64).mean(-2), orig, new)
    print('%d:%d C = 3: worst |device - float64| / bar = %.4f' % (orig, new, (np.abs(got - ref) / bar).max()))
    assert (np.abs(got - ref) <= bar).all()


def torch_inf_norm(r):
    """r / r.abs().max() per row where that maximum is non-zero (a NaN maximum is), by torch."""
    peak = r.abs().amax(dim=-1, keepdim=True)
    return torch.where(peak != 0, r / peak, r)


def track(L, B=1, C=2, seed=7):
    return dev(noise(L, B * C, seed=seed)).reshape(B, C, L) * 0.3


@pytest.mark.parametrize('orig,new', RATIOS)
def test_prepare_audio(orig, new):
    L = 3 * seam(orig, new) + 17
    # a plain track, (C, N) -> (1, N')
    x = track(L)
    got = prepare_audio(x[0], orig, new)
    want = torch_inf_norm(mix_resample(x, orig, new))
    assert got.shape == (1, out_len(L, orig, new)) and same_bits(got, want)
    assert got.abs().max().item() == 1.0
    # an all-zero row stays zero and finite
    z = prepare_audio(torch.zeros(2, L, device=DEV), orig, new)
    assert z.shape == (1, out_len(L, orig, new)) and not z.any() and bool(torch.isfinite(z).all())
    # one NaN sample, one inf sample
    for poison in (float('nan'), float('inf')):
        xp = track(L).clone()
        xp[0, 1, L // 2] = poison
        got = prepare_audio(xp, orig, new)
        r = mix_resample(xp, orig, new)
        assert got.shape == (1, 1, out_len(L, orig, new)) and same_bits(got[:, 0], torch_inf_norm(r))
        assert bool(r.isnan().any()) and bool(got.isnan().all()) if math.isnan(poison) else bool(got.isnan().any())
    # a batch of three with one poisoned row: the others are what they are alone
    xb = track(L, B=3)
    alone = [prepare_audio(xb[i], orig, new) for i in range(3)]
    xb[1, 0, 5] = float('nan')
    got = prepare_audio(xb, orig, new)
    assert got.shape == (3, 1, out_len(L, orig, new))
    assert same_bits(got[0], alone[0]) and same_bits(got[2], alone[2]) and bool(got[1].isnan().all())
    assert same_bits(got[:, 0], torch_inf_norm(mix_resample(xb, orig, new)))


def test_prepare_audio_at_the_same_rate():
    x = track(5003, B=2, C=3)
    x[1] = 0
    got = prepare_audio(x, 22050, 22050)
    assert got.shape == (2, 1, 5003)
    assert same_bits(got[:, 0], torch_inf_norm(torch.mean(x, dim=1))) and not got[1].any()
    assert same_bits(prepare_audio(x[0], 44100, 44100), got[0])


def test_reproducible_and_batching():
    x = track(3 * audio.RESAMPLE_TILE * 320 + 17, B=3, C=1)[:, 0]
    a, b = resample(x, 48000, 22050), resample(x, 48000, 22050)
    assert torch.equal(a, b)
    assert torch.equal(resample(x[1], 48000, 22050), a[1]) and torch.equal(resample(x.reshape(3, 1, 1, -1), 48000, 22050)[:, 0, 0], a)
    assert torch.equal(prepare_audio(x[:, None], 48000, 22050), prepare_audio(x[:, None], 48000, 22050))
    assert torch.equal(resample(x, 44100, 22050), resample(x, 44100, 22050))


def test_more_rows_than_one_launch_holds():
    """The clips ride on grid.y (65535 at most): further rows go to further launches, unseen by the caller."""
    B = 65535 + 3
    x = (torch.arange(B * 9, device=DEV, dtype=torch.float32).reshape(B, 9) % 17.0) - 8.0
    y = resample(x, 44100, 22050)
    assert y.shape == (B, 5)
    for i in (0, 65534, 65535, B - 1):
        assert torch.equal(y[i], resample(x[i], 44100, 22050))
    z = prepare_audio(x[:, None], 44100, 22050)
    assert z.shape == (B, 1, 5) and same_bits(z[:, 0], torch_inf_norm(y))
    same = prepare_audio(x[:, None], 22050, 22050)
    assert same_bits(same[:, 0], torch_inf_norm(x))


def test_dtypes_and_empty():
    x = track(700, B=2, C=1)[:, 0]
    for dtype in (torch.float16, torch.bfloat16):
        xh = x.to(dtype)
        y = resample(xh, 16000, 22050)
        assert y.dtype == dtype and torch.equal(y, resample(xh.float(), 16000, 22050).to(dtype))
        assert prepare_audio(xh[:, None], 16000, 22050).dtype == dtype
    e = resample(torch.zeros(1, 0, device=DEV), 48000, 22050)
    assert e.shape == (1, 0) and e.is_cuda
    assert prepare_audio(torch.zeros(2, 0, device=DEV), 48000, 22050).shape == (1, 0)
    assert resample(x, 22050, 22050) is x


def test_argument_checks():
    x = torch.zeros(2, 1000, device=DEV)
    with pytest.raises(ValueError, match='resample_host'):
        resample(x.double(), 48000, 22050)
    with pytest.raises(ValueError):
        resample(x, 44100.5, 22050)
    with pytest.raises(ValueError):
        resample(x, 48000, 22050, resampling_method='sinc_interp_kaiser')
    with pytest.raises(ValueError):
        resample(x, 1000, 999)
    with pytest.raises(RuntimeError):
        resample(x.cpu(), 48000, 22050)
    with pytest.raises(ValueError):
        prepare_audio(x[0], 48000, 22050)


def test_c_abi_argument_checks():
    lib = _hip.lib()
    P, st = _hip.ptr, _hip.stream_ptr()
    x = torch.zeros(2, 1000, device=DEV)
    y = torch.zeros(2, 1000, device=DEV)
    taps = torch.zeros(704 * 8, device=DEV)
    assert lib.tt_resample_max_taps() >= 694 and lib.tt_resample_max_phases() >= 441
    assert lib.tt_resample_partials(1000, 2, 1) == 1 and lib.tt_resample_partials(320 * 16 + 1, 320, 147) == 2
    assert lib.tt_resample_partials(1000, 1000, 999) == -1 and lib.tt_resample_partials(0, 2, 1) == -1
    assert lib.tt_resample(P(x), 2, 1, 1000, P(taps), 2, 1, 13, P(y), 500, None, st) == 0
    for args in ((2, 1, 1000, 2, 1, 13, 499), (2, 1, 1000, 2, 1, 352, 500), (2, 1, 1000, 2, 2000, 13, 1000000), (0, 1, 1000, 2, 1, 13, 500),
                 (2, 0, 1000, 2, 1, 13, 500), (2, 1, 0, 2, 1, 13, 0)):
        B, C, L, orig, new, width, Lout = args
        assert lib.tt_resample(P(x), B, C, L, P(taps), orig, new, width, P(y), Lout, None, st) == -1
    assert lib.tt_resample_normalize(P(y), 2, 500, P(x), 0, st) == -1
    assert lib.tt_resample_normalize(P(y), 0, 500, P(x), 1, st) == -1
    torch.cuda.synchronize()
