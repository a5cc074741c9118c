"""
Elementwise float64 parity of the constant-Q kernels (csrc/cqt.hip, csrc/cqt_generic.hip) at bars that know each bin's scale.

tests/test_gpu_cqt.py holds the transform to 1e-4 of the global maximum on uniform noise.  Here every coefficient bin and every audio
block has its own bar (oracle/nsgt_error.py: the absolute sum behind the bin, plus the round-off floor of the transforms), and the
inputs reach spectral indices on their own: impulses, DC / Nyquist (whose float64 result is zero everywhere), tones on the indices
where k_fft49_cols changes path (the k1 = 0 column, the 337 / 338 low / mirror boundary, the last tile, the first and last index any
window reaches, bins 0 / 1 with their one- and two-sample windows), a loud and a quiet tone 80 dB apart, a chirp.  Forward through
all three epilogues (planes, interleaved complex, magnitude), inverse through both prologues and WITHOUT the inf-norm division
(_decode_raw against oracle.nsgt.decode: the synthesis' absolute scale), the division itself against torch on the kernel's own raw
output, non-finite values, and the any-length path at N = 66150 and N = 11025 with the Bluestein stage count in the same bars.

Constants.  K[family] is 4 times the worst ratio to the bar that the float32 restatement of the oracle (nsgt_error.encode_f32 /
decode_f32: torch.fft on complex64) reaches against float64 on that family, measured on the CPU and written below as a literal with the
measurement beside it; test_constants_follow_the_restatement (no GPU needed) recomputes the measurement and holds it to K / 4 within
25 %.  The factor 4 covers a different factorisation of the same transforms (675 x 49 with direct radix-5 / 7 / 9 butterflies and
16 x 4 x 16 instead of pocketfft's), nothing more: on noise the kernels were measured equal to pocketfft.  A family used at both block
lengths takes the worse of its two measurements.

Every check prints its ratio to the bar (pytest -rP).  The kernels' worst ratios, measured on an MI355X, in units of the bar (K = 1;
planes and interleaved complex agree to the digits shown, the magnitude epilogue is the second figure):
    forward   noise 0.34 / 0.24, impulses 0.31 / 0.19, dc_nyquist 0.78 / 0.78, tones 1.98 / 1.98, dynamic_range 1.44 / 1.43,
              chirp 0.31 / 0.22
    inverse   analysis 0.38, random 0.35, impulses 0.45 (real planes and complex input alike)
    any-length path, N = 66150:  forward noise 0.16, impulses 0.23, tones (first / last index) 0.79; inverse analysis 0.34, random 0.20
    any-length path, N = 11025:  forward noise 0.20, impulses 0.27, tones (first / last index) 0.31; inverse analysis 0.36, random 0.19
decode() equalled raw / peak bit for bit.  With the fmaxf peak reduction the kernels had before these tests, the four non-finite decode
tests fail: fmaxf drops the NaN and clip 1 comes out finite, all 66150 samples of it.
"""

import functools

import numpy as np
import pytest
import torch

from oracle import nsgt, nsgt_error

gpu = pytest.mark.gpu
SR, N, M, F = 22050, 66150, 1024, 540
N_SMALL = 11025                   # CQT(9, 60, 22050, 0.5): M = 128, odd length, any-length path only

# family: (K, the worst ratio of the float32 restatement to the bar with constant 1 that K is 4 times of).  torch's CPU transforms are
# MKL's, whose code path -- and so whose round-off -- depends on the processor: each family was measured on two x86 hosts with different
# processors (both figures beside the literal; a family that also runs at N = 11025 counted at the worse of its two block lengths) and K
# takes the worse host.
K_FWD = {
    'noise': (1.60, 0.3988),              # 0.3988, 0.3787
    'impulses': (1.16, 0.2890),           # 0.2730, 0.2890
    'dc_nyquist': (1.48, 0.3704),         # 0.3704, 0.2631
    'tones': (10.87, 2.7174),             # 2.6922, 2.7174
    'dynamic_range': (11.18, 2.7952),     # 2.7952, 1.2901
    'chirp': (1.42, 0.3538),              # 0.3538, 0.2791
}
K_INV = {
    'analysis': (1.82, 0.4536),           # 0.3260, 0.4536
    'random': (1.25, 0.3125),             # 0.3125, 0.3107
    'impulses': (1.31, 0.3272),           # 0.3040, 0.3272
}

_worst = {}


def _note(key, ratio, k):
    _worst[key] = max(_worst.get(key, 0.0), ratio)
    print('ratio to bar: %-40s %.3f (worst so far %.3f, K %.2f)' % (key, ratio, _worst[key], k))


# ---- inputs -------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _tab(n):
    return nsgt.nsgt_tables(9, 60, SR, n)


def _tone(j, n):
    t = np.arange(n, dtype=np.int64)
    return np.cos(2.0 * np.pi * ((j * t) % n) / n + 0.3)                 # the phase reduced exactly


def _tone_indices(n, edges_only=False):
    tab = _tab(n)
    first, last = int(tab['spec_index'].min()), int(tab['spec_index'].max())
    if edges_only or n != N:
        return [first, last]
    assert (first, last) == (64, 33071) and tab['lengths'][0] == 1 and tab['positions'][0] == tab['positions'][1] == 65
    p = tab['positions']
    # bins 0 and 1 share centre 65 (bin 0 has a one-sample window), a mid and the top bin; the first and last index any window reaches;
    # then k = k1 + 675 k2 of k_fft49_cols: its k1 = 0 column, the low / mirror boundary k1 = 337 | 338 (and through NC - k their
    # partners), the last low column of the last tile
    return [int(p[0]), int(p[333]), int(p[539]), first, last, 675 * 3, 337 + 675 * 5, 338 + 675 * 5, 336 + 675 * 48]


def _audio(family, n):
    """float32 (B, 1, blocks * n)"""
    rng = np.random.default_rng(11 + n)
    t = np.arange(n, dtype=np.float64)
    if family == 'noise':
        x = rng.uniform(-1, 1, (2, 2 * n))                               # 2 clips x 2 blocks, every block different
    elif family == 'impulses':
        x = np.zeros((4, n))
        for b, i in enumerate((0, 1, n - 1, n // 2)):
            x[b, i] = 1.0
    elif family == 'dc_nyquist':
        x = np.stack([np.ones(n), 1.0 - 2.0 * (np.arange(n) % 2)])
    elif family == 'tones':
        x = np.stack([_tone(j, n) for j in _tone_indices(n)])
    elif family == 'tones_edge':
        x = np.stack([_tone(j, n) for j in _tone_indices(n, True)])
    elif family == 'dynamic_range':
        x = (np.cos(2 * np.pi * 5000.3 * t / SR) + 1e-4 * np.cos(2 * np.pi * 50.1 * t / SR))[None]
    elif family == 'chirp':
        secs = n / SR
        x = np.sin(2 * np.pi * (20.0 * t / SR + (11000.0 - 20.0) / (2 * secs) * (t / SR) ** 2))[None]     # 20 Hz -> 11 kHz over the block
    else:
        raise KeyError(family)
    return np.ascontiguousarray(x[:, None, :].astype(np.float32))


def _fwd_case(family, n=N):
    return _fwd_case_cached(family, n)


@functools.lru_cache(maxsize=None)
def _fwd_case_cached(family, n):
    """(audio float32, float64 coefficients of the rounded audio); computed once, shared by every test, read-only"""
    a = _audio(family, n)
    ref = nsgt.encode(a.astype(np.float64), _tab(n))
    for v in (a, ref):
        v.setflags(write=False)
    return a, ref


@functools.lru_cache(maxsize=None)
def _fwd_bar(family, n, generic):
    bar = nsgt_error.encode_bar(_fwd_case(family, n)[0], _tab(n), nsgt_error.fft_stages(n, generic))
    bar.setflags(write=False)
    return bar


def _coeffs(family, n):
    """complex64 (B, 1, F, blocks * m)"""
    tab = _tab(n)
    m = tab['max_window_length']
    rng = np.random.default_rng({'analysis': 21, 'random': 22}.get(family, 23) + n)
    if family == 'analysis':
        c = nsgt.encode(rng.uniform(-1, 1, (2, 1, 2 * n)), tab)
    elif family == 'random':
        c = rng.standard_normal((2, 1, F, m)) + 1j * rng.standard_normal((2, 1, F, m))
    elif family == 'impulses':
        # (a constant row has a float64 result of exactly zero, and so a bar of zero: none here)
        c = np.zeros((5, 1, F, m), dtype=np.complex128)
        c[0, 0, 0, 0] = 1.0
        c[1, 0, 0, m - 1] = 1.0j
        c[2, 0, 539, m // 2 - 1] = 1.0
        c[3, 0, 1, 3] = 1.0
        c[4, 0, 300, :] = np.exp(1j * np.pi * (np.arange(m) % 2))       # exp(i pi t) = +-1, the argument reduced exactly
    else:
        raise KeyError(family)
    return np.ascontiguousarray(c.astype(np.complex64))


def _inv_case(family, n=N):
    return _inv_case_cached(family, n)


@functools.lru_cache(maxsize=None)
def _inv_case_cached(family, n):
    """(coefficients complex64, float64 synthesis of the rounded coefficients, no inf-norm)"""
    c = _coeffs(family, n)
    ref = nsgt.decode(c.astype(np.complex128), _tab(n))
    for v in (c, ref):
        v.setflags(write=False)
    return c, ref


@functools.lru_cache(maxsize=None)
def _inv_bar(family, n, generic):
    c, ref = _inv_case(family, n)
    bar = nsgt_error.decode_bar(c, _tab(n), nsgt_error.fft_stages(n, generic), reference=ref)
    bar.setflags(write=False)
    return bar


def _fwd_ratio(got, family, n=N, generic=False, magnitude=False):
    """worst |got - float64| / bar over every frame of every (clip, block, bin).  got: complex or (magnitude) real ndarray (B, 1, F, T)."""
    a, ref = _fwd_case(family, n)
    m = _tab(n)['max_window_length']
    B, nblk = a.shape[0], a.shape[-1] // n
    if magnitude:
        # | got - |ref| | <= bar + 2^-22 |ref|: the square root and the two squares of the epilogue on top of the coefficient's own error
        err = np.maximum(np.abs(got - np.abs(ref)) - 2.0 ** -22 * np.abs(ref), 0.0)
    else:
        err = np.abs(got - ref)
    assert err.shape == (B, 1, F, nblk * m), err.shape
    err = err.reshape(B, F, nblk, m).max(-1).transpose(0, 2, 1)
    return float((err / _fwd_bar(family, n, generic)).max())


def _inv_ratio(got, family, n=N, generic=False):
    c, ref = _inv_case(family, n)
    assert got.shape == ref.shape, got.shape
    B, nblk = ref.shape[0], ref.shape[-1] // n
    err = np.abs(got.astype(np.float64) - ref).reshape(B, nblk, n).max(-1)
    return float((err / _inv_bar(family, n, generic)).max())


# ---- the constants follow their definition (CPU) -------------------------------------------------------------------------------------------

def _restatement_fwd(family):
    r = _fwd_ratio(nsgt_error.encode_f32(_fwd_case(family)[0], _tab(N)), family)
    if family in GENERIC_FWD:                                                    # also used at the short block length: the worse of the two
        fam = GENERIC_FWD[family]
        r = max(r, _fwd_ratio(nsgt_error.encode_f32(_fwd_case(fam, N_SMALL)[0], _tab(N_SMALL)), fam, N_SMALL))
    return r


def _restatement_inv(family):
    r = _inv_ratio(nsgt_error.decode_f32(_inv_case(family)[0], _tab(N)), family)
    if family in GENERIC_INV:
        r = max(r, _inv_ratio(nsgt_error.decode_f32(_inv_case(family, N_SMALL)[0], _tab(N_SMALL)), family, N_SMALL))
    return r


# family of the constant -> the inputs the any-length path runs of it ('tones': the first and last index any window reaches)
GENERIC_FWD = {'noise': 'noise', 'impulses': 'impulses', 'tones': 'tones_edge'}
GENERIC_INV = ('analysis', 'random')


@pytest.mark.parametrize('direction,family', [('fwd', f) for f in K_FWD] + [('inv', f) for f in K_INV])
def test_constants_follow_the_restatement(direction, family):
    """K[family] / 4 is what pocketfft in complex64 reaches on the family, re-measured here: a literal that drifted from its definition
    (inputs, tables or bars changed without re-measuring) fails."""
    k, measured = (K_FWD if direction == 'fwd' else K_INV)[family]
    r = _restatement_fwd(family) if direction == 'fwd' else _restatement_inv(family)
    print('float32 restatement, %s %-14s worst ratio to the bar %.4f (literal %.4f, K %.2f)' % (direction, family, r, measured, k))
    assert r <= k / 4 * 1.25, (r, k)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def cqt():
    from timbre_trap.framework import CQT
    return CQT(9, 60, SR, 3).to('cuda')


@pytest.fixture(scope='module')
def generic_cqt():
    """N = 66150 forced onto the any-length kernels, and the short odd block length that only they serve"""
    from timbre_trap.framework import CQT, cqtwrapper
    mp = pytest.MonkeyPatch()
    mp.setattr(cqtwrapper, 'FORCE_GENERIC', True)
    try:
        forced = CQT(9, 60, SR, 3).to('cuda')
    finally:
        mp.undo()
    small = CQT(9, 60, SR, 0.5).to('cuda')
    assert not forced._fast and forced.block_length == N and forced.max_window_length == M
    assert not small._fast and small.block_length == N_SMALL and small.max_window_length == _tab(N_SMALL)['max_window_length'] == 128
    return {N: forced, N_SMALL: small}


def _run_forward(cq, audio, way):
    """complex (or, for the magnitude, real) float ndarray (B, 1, F, T) of the epilogue ``way``"""
    a = torch.tensor(audio).cuda()
    if way == 'planes':
        out = cq(a)
        assert out.dtype == torch.float32 and out.is_contiguous() and out.size(1) == 2
        o = out.cpu().numpy().astype(np.float64)
        return (o[:, 0] + 1j * o[:, 1])[:, None]
    if way == 'complex':
        out = cq.encode(a)
        assert out.dtype == torch.complex64 and out.size(1) == 1
        return out.cpu().numpy().astype(np.complex128)
    out = cq.magnitude(a)
    assert out.dtype == torch.float32 and out.dim() == 3
    return out.cpu().numpy().astype(np.float64)[:, None]


def _run_inverse(cq, coeffs, way):
    c = torch.tensor(coeffs).cuda()
    if way == 'planes':
        c = torch.stack([c[:, 0].real, c[:, 0].imag], 1).contiguous()
    return cq._decode_raw(c)


@gpu
@pytest.mark.parametrize('way', ['planes', 'complex', 'magnitude'])
@pytest.mark.parametrize('family', list(K_FWD))
def test_forward_family(cqt, family, way):
    got = _run_forward(cqt, _fwd_case(family)[0], way)
    assert np.isfinite(got).all()
    r = _fwd_ratio(got, family, magnitude=(way == 'magnitude'))
    _note('forward %s %s' % (family, way), r, K_FWD[family][0])
    assert r <= K_FWD[family][0]


@gpu
@pytest.mark.parametrize('way', ['planes', 'complex'])
@pytest.mark.parametrize('family', list(K_INV))
def test_inverse_family_without_normalisation(cqt, family, way):
    """_decode_raw against oracle.nsgt.decode: the absolute scale of the synthesis (1 / NC, 1 / M, the factor 2 of the Hermitian half),
    which the inf-norm division of decode() hides."""
    got = _run_inverse(cqt, _inv_case(family)[0], way).cpu().numpy()
    assert np.isfinite(got).all()
    r = _inv_ratio(got, family)
    _note('inverse %s %s' % (family, way), r, K_INV[family][0])
    assert r <= K_INV[family][0]


def _ulp(x):
    return (torch.nextafter(x.abs(), torch.full_like(x, float('inf'))) - x.abs())


@gpu
@pytest.mark.parametrize('family', ['analysis', 'random'])
def test_decode_is_raw_over_its_peak(cqt, family):
    c = torch.tensor(_inv_case(family)[0]).cuda()
    raw = cqt._decode_raw(c)
    want = raw / raw.abs().max()
    got = cqt.decode(c)
    excess = float(((got - want).abs() - _ulp(want)).max())
    print('decode vs raw / peak, %s: worst difference %.3e, beyond one ulp by %.3e' % (family, float((got - want).abs().max()), max(excess, 0.0)))
    assert excess <= 0.0
    assert float(got.abs().max()) == 1.0


@gpu
@pytest.mark.parametrize('value', [float('nan'), float('inf')], ids=['nan', 'inf'])
@pytest.mark.parametrize('path', ['specialised', 'generic'])
def test_decode_peak_propagates_non_finite(cqt, generic_cqt, path, value):
    """Reference cqtwrapper.py:209-211 divides the batch by audio.abs().max() whenever that is truthy: a NaN anywhere makes the maximum
    NaN and the whole batch NaN.  One non-finite coefficient in clip 0 of two: decode() equals that expression applied to the kernel's
    own raw output, NaN positions included."""
    cq = cqt if path == 'specialised' else generic_cqt[N]
    c = torch.tensor(_inv_case('random')[0])
    c[0, 0, 200, 100] = complex(value, 0.0)
    c = c.cuda()
    raw = cq._decode_raw(c)
    assert bool(torch.isfinite(raw[1]).all()) and not bool(torch.isfinite(raw[0]).all())
    want = raw / raw.abs().max()
    got = cq.decode(c)
    if value != value:
        assert bool(torch.isnan(want).all())                         # a NaN in clip 0: the peak is NaN, and so is the whole batch
    assert torch.allclose(got, want, rtol=0.0, atol=0.0, equal_nan=True), \
        'clip 1 holds %d finite samples' % int(torch.isfinite(got[1]).sum())


@gpu
@pytest.mark.parametrize('path', ['specialised', 'generic'])
def test_forward_nan_stays_in_its_block(cqt, generic_cqt, path):
    cq = cqt if path == 'specialised' else generic_cqt[N]
    a = torch.tensor(_fwd_case('noise')[0]).cuda()
    clean = cq(a)
    b = a.clone()
    b[0, 0, N + 12345] = float('nan')                                    # clip 0, block 1
    out = cq(b)
    assert bool(torch.isnan(out[0, :, :, M:]).all())
    assert torch.equal(out[0, :, :, :M], clean[0, :, :, :M]) and torch.equal(out[1], clean[1])
    if path == 'specialised':
        mag = cq.magnitude(b)
        assert bool(torch.isnan(mag[0, :, M:]).all()) and torch.equal(mag[0, :, :M], cq.magnitude(a)[0, :, :M])


@gpu
@pytest.mark.parametrize('family', list(GENERIC_FWD))
@pytest.mark.parametrize('n', [N, N_SMALL])
def test_generic_forward_family(generic_cqt, n, family):
    """The any-length path at the same bars: that block length's tables, 3 log2(P) stages for the length-N transform."""
    fam = GENERIC_FWD[family]
    for way in ('planes', 'complex'):
        got = _run_forward(generic_cqt[n], _fwd_case(fam, n)[0], way)
        assert np.isfinite(got).all()
        r = _fwd_ratio(got, fam, n, generic=True)
        _note('generic %d forward %s %s' % (n, fam, way), r, K_FWD[family][0])
        assert r <= K_FWD[family][0]


@gpu
@pytest.mark.parametrize('family', list(GENERIC_INV))
@pytest.mark.parametrize('n', [N, N_SMALL])
def test_generic_inverse_family(generic_cqt, n, family):
    for way in ('planes', 'complex'):
        got = _run_inverse(generic_cqt[n], _inv_case(family, n)[0], way).cpu().numpy()
        assert np.isfinite(got).all()
        r = _inv_ratio(got, family, n, generic=True)
        _note('generic %d inverse %s %s' % (n, family, way), r, K_INV[family][0])
        assert r <= K_INV[family][0]
