"""
Float64 references for the gradients of the constant-Q transform (helper of test_cqt_grad_restatement.py / test_gpu_cqt_grad.py).

Both directions of oracle/nsgt.py are real-linear and every window lies inside the open positive half-spectrum, so with a gradient
w.r.t. complex values held as dL/dre + i dL/dim (torch's convention), N = block length, M = frames per block and ``adj`` the tables
with ``window`` and ``dual`` exchanged:

    analysis (encode)    E^T g = (N / 2M) decode(g, adj)      <E x, g> = Re sum conj(E x) g = <x, E^T g>
    synthesis (decode)   D^T y = (2M / N) encode(y, adj)

(encode is X = fft_N x, crop and window, ifft_M: its transpose is N ifft_N of the scattered, windowed (1 / M) fft_M, real part taken;
decode's Hermitian extension doubles the real part of the same expression, hence the 1 / 2.)

    adjoint_tables                         the exchanged tables
    analysis_vjp / synthesis_vjp /         the three vector-Jacobian products in numpy float64, through oracle.nsgt.encode / decode on
    magnitude_vjp                          the exchanged tables
    encode_t / decode_t                    oracle.nsgt.encode / decode restated in torch float64 so that autograd can differentiate
                                           them: an independent check of the derivation above (decode_t goes through irfft, not through
                                           the explicit Hermitian extension)
"""

import numpy as np
import torch

from oracle import nsgt


def adjoint_tables(tab):
    adj = dict(tab)
    adj['window'], adj['dual'] = tab['dual'], tab['window']
    return adj


def _nm(tab):
    return tab['block_length'], tab['max_window_length']


def analysis_vjp(g, tab):
    """g complex (B, 1, F, n M) = dL/dre + i dL/dim of encode's output -> dL/daudio float64 (B, 1, n N)."""
    N, M = _nm(tab)
    return (N / (2.0 * M)) * nsgt.decode(np.asarray(g, dtype=np.complex128), adjoint_tables(tab))


def synthesis_vjp(y, tab):
    """y real (B, 1, n N) = dL/daudio of decode's output -> dL/dre + i dL/dim of the coefficients, complex128 (B, 1, F, n M)."""
    N, M = _nm(tab)
    return (2.0 * M / N) * nsgt.encode(np.asarray(y, dtype=np.float64), adjoint_tables(tab))


def magnitude_direction(c, dmag):
    """dc = dmag c / |c|, exactly 0 where c == 0 (torch's norm backward).  c complex (B, 1, F, T), dmag real (B, 1, F, T) or (B, F, T)."""
    c = np.asarray(c, dtype=np.complex128)
    a = np.abs(c)
    dmag = np.asarray(dmag, dtype=np.float64).reshape(c.shape)
    return np.where(a > 0, dmag * c / np.where(a > 0, a, 1.0), 0.0)


def magnitude_vjp(audio, dmag, tab):
    """gradient of |encode(audio)| w.r.t. the audio for the upstream gradient dmag."""
    return analysis_vjp(magnitude_direction(nsgt.encode(audio, tab), dmag), tab)


# ---- torch float64 restatements (differentiable) --------------------------------------------------------------------------------------

def encode_t(audio, tab):
    """oracle.nsgt.encode on a torch float64 tensor (B, 1, n N) -> complex128 (B, 1, F, n M), differentiable."""
    N, M = _nm(tab)
    F, off, pad = tab['n_bins'], tab['win_off'], tab['pad']
    B = audio.shape[0]
    nblk = audio.shape[-1] // N
    X = torch.fft.fft(audio.reshape(B, nblk, N).to(torch.complex128), dim=-1)
    w = torch.from_numpy(np.asarray(tab['window'], dtype=np.float64))
    rows = []
    for k in range(F):
        L = int(off[k + 1] - off[k])
        idx = torch.from_numpy(tab['spec_index'][off[k]:off[k + 1]] % N)
        v = torch.nn.functional.pad(X[..., idx] * w[off[k]:off[k + 1]], (int(pad[k]), M - int(pad[k]) - L))
        rows.append(torch.fft.ifft(v, dim=-1))
    out = torch.stack(rows, dim=2)                                       # (B, n, F, M)
    return out.permute(0, 2, 1, 3).reshape(B, 1, F, nblk * M)


def decode_t(coefficients, tab):
    """oracle.nsgt.decode on a torch complex128 tensor (B, 1, F, n M) -> float64 (B, 1, n N), differentiable.  The windows span the open
    positive half-spectrum only, so the Hermitian extension of the oracle is irfft of the half spectrum here."""
    N, M = _nm(tab)
    F, off, pad = tab['n_bins'], tab['win_off'], tab['pad']
    B = coefficients.shape[0]
    nblk = coefficients.shape[-1] // M
    V = torch.fft.fft(coefficients.reshape(B, F, nblk, M), dim=-1)
    d = torch.from_numpy(np.asarray(tab['dual'], dtype=np.float64))
    segs = [V[:, k, :, int(pad[k]):int(pad[k]) + int(off[k + 1] - off[k])] * d[off[k]:off[k + 1]] for k in range(F)]
    seg = torch.cat(segs, dim=-1)                                        # (B, n, sum L)
    idx = torch.from_numpy(np.asarray(tab['spec_index'], dtype=np.int64))
    zero = torch.zeros((B, nblk, N // 2 + 1), dtype=torch.float64)
    Xh = torch.complex(zero.index_add(-1, idx, seg.real), zero.index_add(-1, idx, seg.imag))
    return torch.fft.irfft(Xh, n=N, dim=-1).reshape(B, 1, nblk * N)


# ---- the cases of the gradient tests: inputs, float64 references and bars, computed once and shared (read-only) -------------------------
# The analysis gradient is held per block at K (N / 2M) decode_bar(g, adj), the synthesis gradient per bin at K (2M / N) encode_bar(y, adj)
# (oracle/nsgt_error.py: the bars take any table dict, the exchanged one included).  K[family] is 4 times the worst ratio to its bar that
# the float32 restatement (nsgt_error.decode_f32 / encode_f32 on the exchanged tables: torch.fft on complex64) reaches against float64,
# measured on the CPU and written below as a literal with the measurement beside it; test_cqt_grad_restatement.py re-measures it and holds
# it to K / 4 within 25 %.  The factor 4 covers a different factorisation of the same transforms (tests/test_gpu_cqt_parity.py), nothing
# more.  A family used at both block lengths takes the worse of its two measurements.

import functools                                                          # noqa: E402

from oracle import nsgt_error                                             # noqa: E402

SR, F = 22050, 540
N_FAST, N_SMALL = 66150, 11025                                            # CQT(9, 60, 22050, 3) / CQT(9, 60, 22050, 0.5): M = 1024 / 128
SINGLE_BINS, N_SINGLE = (0, 1, 539), 6                                    # x frames (0, M - 1)

K_ANALYSIS = {
    'random': (1.48, 0.3691),             # 0.3334 at N = 66150, 0.3691 at N = 11025
    'l2': (1.71, 0.4278),                 # 0.3319, 0.4278
    'single': (5.76, 1.4406),             # 1.4406, 0.8223
    'magnitude': (1.94, 0.4860),          # 0.4070, 0.4860 (the float32 composition: encode, dmag c / |c|, decode on the exchanged tables)
}
K_SYNTHESIS = {
    'noise': (1.34, 0.3352),              # 0.2958, 0.3352
    'impulses': (1.45, 0.3630),           # 0.2604, 0.3630
    'dc_nyquist': (5.40, 1.3512),         # 1.2891, 1.3512
    'tones': (9.48, 2.3700),              # 2.3700, 1.9797
}


@functools.lru_cache(maxsize=None)
def tables(n):
    return nsgt.nsgt_tables(9, 60, SR, n)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _tone(j, n):
    t = np.arange(n, dtype=np.int64)
    return np.cos(2.0 * np.pi * ((j * t) % n) / n + 0.3)                 # the phase reduced exactly


def single_positions(n, clips=2):
    """(clip, bin, frame) of the one non-zero coefficient of each of the N_SINGLE cases stacked along the batch: ``clips`` clips x 2 blocks
    per case, the coefficient in the second block of the case's last clip."""
    m = tables(n)['max_window_length']
    return [(clips * i + clips - 1, b, m + t) for i, (b, t) in enumerate((b, t) for b in SINGLE_BINS for t in (0, m - 1))]


@functools.lru_cache(maxsize=None)
def noise_audio(n, seed=0):
    """float32 (2, 1, 2 n): 2 clips x 2 blocks, every block different"""
    a = np.random.default_rng(31 + n + seed).uniform(-1, 1, (2, 1, 2 * n)).astype(np.float32)
    return _frozen(a)[0]


@functools.lru_cache(maxsize=None)
def analysis_case(family, n, clips=2):
    """(g complex64 (B, 1, F, 2 M), float64 gradient w.r.t. the audio (B, 1, 2 n))"""
    tab = tables(n)
    m = tab['max_window_length']
    rng = np.random.default_rng({'random': 41, 'l2': 42}.get(family, 43) + n)
    if family == 'random':
        g = rng.standard_normal((2, 1, F, 2 * m)) + 1j * rng.standard_normal((2, 1, F, 2 * m))
    elif family == 'l2':                                                  # the gradient of an L2 loss between two analyses
        g = nsgt.encode(noise_audio(n).astype(np.float64), tab) - nsgt.encode(noise_audio(n, 1).astype(np.float64), tab)
    elif family == 'single':
        g = np.zeros((N_SINGLE * clips, 1, F, 2 * m), dtype=np.complex128)
        for i, (b, k, t) in enumerate(single_positions(n, clips)):
            g[b, 0, k, t] = (1.0, 1.0j, 0.6 - 0.8j)[i % 3]
    else:
        raise KeyError(family)
    g = np.ascontiguousarray(g.astype(np.complex64))
    return _frozen(g, analysis_vjp(g, tab))


@functools.lru_cache(maxsize=None)
def analysis_bar(family, n, generic, clips=2):
    """float64 (B, 2): the bar of every sample of a block, constant 1"""
    tab = tables(n)
    N, M = _nm(tab)
    if family == 'magnitude':
        g, ref = magnitude_case(n)[2:]
    else:
        g, ref = analysis_case(family, n, clips)
    scale = N / (2.0 * M)
    return _frozen(scale * nsgt_error.decode_bar(g, adjoint_tables(tab), nsgt_error.fft_stages(n, generic), reference=ref / scale))[0]


def analysis_ratio(got, ref, bar):
    """worst |got - float64| / bar over the blocks; a block whose bar is zero (float64 result zero, nothing reaches it) must be exact"""
    B, nblk = bar.shape
    err = np.abs(np.asarray(got, dtype=np.float64) - ref).reshape(B, nblk, -1).max(-1)
    assert not (err[bar == 0] != 0).any(), 'a block nothing reaches is not exactly zero'
    return float((err[bar > 0] / bar[bar > 0]).max())


@functools.lru_cache(maxsize=None)
def synthesis_case(family, n):
    """(y float32 (B, 1, blocks n), float64 gradient w.r.t. the coefficients, complex (B, 1, F, blocks M))"""
    tab = tables(n)
    if family == 'noise':
        y = noise_audio(n, 2).astype(np.float64)[:, 0]
    elif family == 'impulses':
        y = np.zeros((4, n))
        for b, i in enumerate((0, 1, n - 1, n // 2)):
            y[b, i] = 1.0
    elif family == 'dc_nyquist':                                          # float64 result zero everywhere: no window reaches either
        y = np.stack([np.ones(n), 1.0 - 2.0 * (np.arange(n) % 2)])
    elif family == 'tones':                                               # the first and last spectral index any window reaches
        y = np.stack([_tone(int(tab['spec_index'].min()), n), _tone(int(tab['spec_index'].max()), n)])
    else:
        raise KeyError(family)
    y = np.ascontiguousarray(y[:, None, :].astype(np.float32))
    return _frozen(y, synthesis_vjp(y.astype(np.float64), tab))


@functools.lru_cache(maxsize=None)
def synthesis_bar(family, n, generic):
    """float64 (B, blocks, F): the bar of every frame of a bin, constant 1"""
    tab = tables(n)
    N, M = _nm(tab)
    bar = (2.0 * M / N) * nsgt_error.encode_bar(synthesis_case(family, n)[0], adjoint_tables(tab), nsgt_error.fft_stages(n, generic))
    return _frozen(bar)[0]


def synthesis_ratio(got, ref, bar):
    B, nblk, nb = bar.shape
    err = np.abs(np.asarray(got, dtype=np.complex128) - ref).reshape(B, nb, nblk, -1).max(-1).transpose(0, 2, 1)
    return float((err / bar).max())


@functools.lru_cache(maxsize=None)
def magnitude_case(n):
    """(audio float32 (2, 1, 2 n), dmag float32 (2, F, 2 M) = h |c_ref| with h uniform in [0.5, 1.5], dc = dmag c / |c| of the rounded
    values (= h c: well conditioned), float64 gradient w.r.t. the audio)"""
    tab = tables(n)
    a = noise_audio(n, 3)
    c = nsgt.encode(a.astype(np.float64), tab)
    h = np.random.default_rng(51 + n).uniform(0.5, 1.5, c.shape)
    dmag = np.ascontiguousarray((h * np.abs(c))[:, 0].astype(np.float32))
    dc = magnitude_direction(c, dmag)
    return _frozen(a, dmag, dc, analysis_vjp(dc, tab))


# ---- what float32 reaches on the same cases (CPU; compared with float64 only, never with the kernels) ------------------------------------

def restatement_analysis(family, n):
    tab = tables(n)
    N, M = _nm(tab)
    if family == 'magnitude':
        a, dmag, _, ref = magnitude_case(n)
        c = nsgt_error.encode_f32(a, tab)
        mag = np.abs(c)
        dc = np.where(mag > 0, dmag[:, None] * c / np.where(mag > 0, mag, 1), 0).astype(np.complex64)
        got = nsgt_error.decode_f32(dc, adjoint_tables(tab))
    else:
        g, ref = analysis_case(family, n)
        got = nsgt_error.decode_f32(g, adjoint_tables(tab))
    return analysis_ratio(got.astype(np.float64) * (N / (2.0 * M)), ref, analysis_bar(family, n, False))


def restatement_synthesis(family, n):
    tab = tables(n)
    N, M = _nm(tab)
    y, ref = synthesis_case(family, n)
    got = nsgt_error.encode_f32(y, adjoint_tables(tab))
    return synthesis_ratio(got.astype(np.complex128) * (2.0 * M / N), ref, synthesis_bar(family, n, False))
