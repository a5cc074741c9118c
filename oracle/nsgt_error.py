"""
ORACLE (test infrastructure only -- never imported by the product path).

Round-off yardsticks for the constant-Q transform: what a float32 implementation of oracle/nsgt.py's algorithm can be held to
against the float64 one, per coefficient bin and per audio block, for ANY input -- a bar that knows each bin's scale instead of
one fraction of the global maximum.

    encode_f32 / decode_f32     oracle.nsgt.encode / decode restated in float32 (torch.fft on complex64 CPU tensors, the window /
                                dual tables rounded to float32).  The independent "what fp32 can do" measurement: compared with
                                float64 only, never with the kernels.
    encode_bar / decode_bar     the bars, from float64 quantities of the input alone (nothing of any implementation's output).

Model.  A radix-2-like FFT of length n in float32 leaves, on every output, an error of about 2^-24 log2(n) times the rms of the
outputs (Gentleman & Sande 1966; Higham, Accuracy and Stability, ch. 24): white, independent of the output's own size.

Forward, bin k, frames t:  c_k = ifft_M(g_k X[start_k + .]).
  * the length-M inverse transform of the windowed samples: log2(M) stages over terms whose absolute sum is
    A_k = (1/M) sum_m g_k[m] |X[j_m]|   (the  sum |a||b|  of a dot product: no frame of the bin can lose more than 2^-24 per stage
    of it);
  * the length-N transform's floor on the samples the window picks up, R = rms |X| over the half spectrum per stage, which the
    window and the 1/M carry into every frame with the gain  G_k = ||g_k||_2 / M  (Parseval: white noise of deviation s on the L_k
    samples gives frames of deviation s ||g_k||_2 / M).  It reaches bins whose own samples are zero (DC / Nyquist input).
      bar[clip, block, k] = 2^-24 (log2(M) A_k + n_fft_stages G_k R)

Inverse, one block:  x = irfft_N( sum_k dual_k V_k ),  V_k = fft_M(c_k).
  * V_k carries 2^-24 log2(M) (|V_k[m]| + rms_m |V_k|): its own rounding and the length-M transform's floor -- the floor matters
    because it lands on window tails where the dual gain is large (up to 4.7e3 with the default tables) while V_k there is tiny;
    times |dual_k[m]|, summed over the bins that reach spectral index j:  E[j];
  * the length-N real inverse spreads the spectral error over the samples: deviation (2/N) ||E||_2 per sample (half spectrum,
    Hermitian: factor 2), and adds its own floor n_fft_stages rms(x).
      bar[clip, block] = 2^-24 (log2(M) (2/N) ||E||_2 + n_fft_stages rms(x_ref))

``n_fft_stages``: log2(N) where one length-N transform runs (csrc/cqt.hip, and pocketfft here), 3 log2(P) for the any-length path
(csrc/cqt_generic.hip: Bluestein runs three length-P power-of-two transforms in its place) -- a count of stages.  The constant in
front of a bar is measured per input family with encode_f32 / decode_f32 (tests/test_gpu_cqt_parity.py).
"""

import math

import numpy as np
import torch

U = 2.0 ** -24


def _geometry(tab):
    return tab['block_length'], tab['max_window_length'], tab['n_bins'], tab['win_off'], tab['pad']


def bluestein_length(N):
    """Length of the cyclic convolution of the any-length path (nsgt_plan.build_plan): the power of two >= 2 N - 1."""
    return 1 << int(2 * N - 2).bit_length()


def fft_stages(N, generic=False):
    return 3 * math.log2(bluestein_length(N)) if generic else math.log2(N)


def encode_f32(audio, tab):
    """oracle.nsgt.encode in float32: audio (B, 1, n N) -> complex64 ndarray (B, 1, F, n M)."""
    N, M, F, off, pad = _geometry(tab)
    x = torch.from_numpy(np.array(audio, dtype=np.float32))                 # (a copy: the caller's array may be read-only)
    B = x.shape[0]
    assert x.shape[-1] % N == 0
    nblk = x.shape[-1] // N
    X = torch.fft.fft(x.reshape(B, nblk, N).to(torch.complex64), dim=-1)
    w32 = torch.from_numpy(tab['window'].astype(np.float32))
    out = torch.zeros((B, nblk, F, M), dtype=torch.complex64)
    for k in range(F):
        L = int(off[k + 1] - off[k])
        v = torch.zeros((B, nblk, M), dtype=torch.complex64)
        idx = torch.from_numpy(tab['spec_index'][off[k]:off[k + 1]] % N)
        v[..., pad[k]:pad[k] + L] = X[..., idx] * w32[off[k]:off[k + 1]]
        out[:, :, k] = torch.fft.ifft(v, dim=-1)
    return out.permute(0, 2, 1, 3).reshape(B, 1, F, nblk * M).numpy()


def decode_f32(coefficients, tab):
    """oracle.nsgt.decode in float32: complex (B, 1, F, n M) -> float32 ndarray (B, 1, n N)."""
    N, M, F, off, pad = _geometry(tab)
    c = torch.from_numpy(np.array(coefficients, dtype=np.complex64))
    B = c.shape[0]
    nblk = c.shape[-1] // M
    V = torch.fft.fft(c.reshape(B, F, nblk, M), dim=-1)
    d32 = torch.from_numpy(tab['dual'].astype(np.float32))
    Xh = torch.zeros((B, nblk, N), dtype=torch.complex64)
    for k in range(F):
        L = int(off[k + 1] - off[k])
        idx = torch.from_numpy(tab['spec_index'][off[k]:off[k + 1]])
        Xh[..., idx] += V[:, k, :, pad[k]:pad[k] + L] * d32[off[k]:off[k + 1]]
    j = torch.arange(1, (N + 1) // 2)
    Xh[..., N - j] = torch.conj(Xh[..., j])
    return torch.fft.ifft(Xh, dim=-1).real.reshape(B, 1, nblk * N).numpy()


def encode_bar(audio, tab, n_fft_stages):
    """float64 (B, n, F): the bar of every frame of bin k of block n of clip b (module docstring).  ``audio`` (B, 1, n N) is rounded
    to float32 first: the bar belongs to the values an fp32 transform is handed."""
    N, M, F, off, pad = _geometry(tab)
    x = np.asarray(audio, dtype=np.float32).astype(np.float64)
    B = x.shape[0]
    nblk = x.shape[-1] // N
    Xa = np.abs(np.fft.rfft(x.reshape(B, nblk, N), axis=-1))
    R = np.sqrt((Xa ** 2).mean(-1))                                     # (B, n)
    A = np.zeros((B, nblk, F))
    G = np.zeros(F)
    for k in range(F):
        g = tab['window'][off[k]:off[k + 1]]
        A[..., k] = (Xa[..., tab['spec_index'][off[k]:off[k + 1]]] * g).sum(-1) / M
        G[k] = math.sqrt(float((g ** 2).sum())) / M
    return U * (math.log2(M) * A + n_fft_stages * G * R[..., None])


def decode_bar(coefficients, tab, n_fft_stages, reference=None):
    """float64 (B, n): the bar of every sample of block n of clip b (module docstring).  ``coefficients`` complex (B, 1, F, n M), rounded
    to complex64 first; ``reference``: oracle.nsgt.decode of the same values if the caller has it already."""
    from oracle import nsgt
    N, M, F, off, pad = _geometry(tab)
    c = np.asarray(coefficients).astype(np.complex64).astype(np.complex128)
    B = c.shape[0]
    nblk = c.shape[-1] // M
    if reference is None:
        reference = nsgt.decode(c, tab)
    rms = np.sqrt((np.asarray(reference, dtype=np.float64).reshape(B, nblk, N) ** 2).mean(-1))
    Va = np.abs(np.fft.fft(c.reshape(B, F, nblk, M), axis=-1))
    E = np.zeros((B, nblk, N // 2 + 1))
    for k in range(F):
        L = int(off[k + 1] - off[k])
        idx = tab['spec_index'][off[k]:off[k + 1]]
        floor = np.sqrt((Va[:, k] ** 2).mean(-1))[..., None]            # (B, n, 1)
        E[..., idx] += (Va[:, k, :, pad[k]:pad[k] + L] + floor) * np.abs(tab['dual'][off[k]:off[k + 1]])
    return U * (math.log2(M) * (2.0 / N) * np.sqrt((E ** 2).sum(-1)) + n_fft_stages * rms)

