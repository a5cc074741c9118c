"""
Float64 reference of the Griffin-Lim phase retrieval (helper of test_gl_restatement.py / test_gpu_griffin_lim.py), on oracle.nsgt.encode /
decode.

One iteration on the audio x with the target magnitudes ``mag``:

    c = encode(x);   p = mag c / |c|, and mag + 0i where |c| == 0;   y = decode(p)
    convergence of x = sqrt(sum (|c| - mag)^2 / sum mag^2) per clip: exactly 0 when the numerator is 0, +inf when only the denominator is

and the k-step sequence with the momentum of "fast Griffin-Lim" applied to the AUDIO:  x_{k+1} = y_k + alpha (y_k - y_{k-1}),  x_1 = y_0.
decode is linear, so this equals the usual coefficient-domain form  y_{k+1} = decode(project(encode(decode(t_k)))),  t_k = p_k + alpha
(p_k - p_{k-1})  (test_gl_restatement.py checks the identity).

The case: cqt_grad_ref.magnitude_case(n) -- noise audio, 2 clips x 2 blocks, and mag = h |c| with h uniform in [0.5, 1.5], so that the
projection of the audio's own coefficients is h c: well conditioned, no coefficient near 0 decides a phase.  The step starts from that
audio; the 8-step sequence (alpha = 0.99) starts from it too.

Bars.  One step is held per block at K_STEP nsgt_error.decode_bar(p, tab, stages, reference = y); the last audio of the sequence per block
at K_SEQ rms(reference block); every convergence value at a relative K_CONV.  Each K is 4 times what the float32 restatement of the same
computation (nsgt_error.encode_f32 / decode_f32, the projection and the extrapolation in float32) reaches against float64, the worse of
N = 66150 and N = 11025, written below as a literal with the measurement beside it; test_gl_restatement.py re-measures it and holds it to
K / 4 within 25 %.  The factor 4 covers a different factorisation of the same transforms (tests/test_gpu_cqt_parity.py), nothing more.
The sequence's bar is a plain fraction of the block's rms because its error is no longer round-off of one transform: a phase perturbed
in step k moves the projection of step k + 1, and the float32 restatement's distance from float64 grows by about 1.5 x per step.
"""

import functools

import numpy as np

import cqt_grad_ref as G
from oracle import nsgt, nsgt_error

N_FAST, N_SMALL, F, SR = G.N_FAST, G.N_SMALL, G.F, G.SR
N_SEQ, ALPHA = 8, 0.99

# (K, measured): K = 4 x measured, rounded
K_STEP = (2.34, 0.5848)                   # ratio to decode_bar: 0.5375 at N = 66150, 0.5848 at N = 11025
K_SEQ = (4.08e-4, 1.0203e-4)              # max error / block rms after step 8: 1.0203e-4, 4.4156e-5 (after step 1: 3.00e-6, 2.35e-6)
K_CONV = (1.67e-7, 4.1722e-8)             # relative, worst of the 8 x 2 values: 3.4168e-8, 4.1722e-8 (float32 results: half an ulp is 6e-8)


def tables(n):
    return G.tables(n)


def convergence(absc, mag):
    """float64 (B,): sqrt(sum (|c| - mag)^2 / sum mag^2) per clip; 0 when the numerator is 0, inf when only the denominator is"""
    absc = np.asarray(absc, dtype=np.float64)
    mag = np.asarray(mag, dtype=np.float64).reshape(absc.shape)
    B = absc.shape[0]
    num, den = ((absc - mag) ** 2).reshape(B, -1).sum(-1), (mag ** 2).reshape(B, -1).sum(-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(num == 0, 0.0, np.sqrt(num / den))


def project(c, mag):
    """mag c / |c|, mag + 0i where c == 0.  c complex (B, 1, F, T); mag real (B, F, T) or (B, 1, F, T)"""
    a = np.abs(c)
    m = np.asarray(mag).reshape(c.shape)
    return np.where(a > 0, m * c / np.where(a > 0, a, 1), m + 0j)


def step(x, mag, tab):
    """(y, projected coefficients, convergence of x): float64"""
    c = nsgt.encode(np.asarray(x, dtype=np.float64), tab)
    p = project(c, np.asarray(mag, dtype=np.float64))
    return nsgt.decode(p, tab), p, convergence(np.abs(c), mag)


def sequence(x0, mag, tab, n_iter, alpha):
    """([y_0 .. y_{n_iter-1}], convergence (n_iter, B)) with the audio-domain extrapolation; x0 None = silence"""
    m = tab['max_window_length']
    x = np.zeros((mag.shape[0], 1, mag.shape[-1] // m * tab['block_length'])) if x0 is None else np.asarray(x0, dtype=np.float64)
    ys, conv = [], []
    for k in range(n_iter):
        y, _, cv = step(x, mag, tab)
        conv.append(cv)
        x = y if not ys else y + alpha * (y - ys[-1])
        ys.append(y)
    return ys, np.stack(conv)


def sequence_coefficient_domain(x0, mag, tab, n_iter, alpha):
    """The same sequence with the extrapolation applied to the projected coefficients, t_k = p_k + alpha (p_k - p_{k-1}), as fast
    Griffin-Lim is usually written: [decode(p_0) .. decode(p_{n_iter-1})]"""
    mag = np.asarray(mag, dtype=np.float64)
    c = nsgt.encode(np.asarray(x0, dtype=np.float64), tab)
    ys, p_prev = [], None
    for k in range(n_iter):
        p = project(c, mag)
        ys.append(nsgt.decode(p, tab))
        t = p if p_prev is None else p + alpha * (p - p_prev)
        p_prev = p
        c = nsgt.encode(nsgt.decode(t, tab), tab)
    return ys


def from_decibels(d):
    return 10.0 ** (4.0 * (np.asarray(d, dtype=np.float64) - 1.0))


# ---- the float32 restatement (CPU; compared with float64 only, never with the kernels) -----------------------------------------------

def convergence_f32(absc, mag, m_frames):
    """the convergence as the entry point is specified: float32 sums over the frames of one bin of one block, float64 across bins and
    blocks, the result a float32"""
    B = absc.shape[0]
    a, m = (np.asarray(v, dtype=np.float32).reshape(B, -1, m_frames) for v in (absc, mag))
    num = ((a - m) ** 2).sum(-1, dtype=np.float32).astype(np.float64).sum(-1)
    den = (m ** 2).sum(-1, dtype=np.float32).astype(np.float64).sum(-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(num == 0, 0.0, np.sqrt(num / den)).astype(np.float32)


def step_f32(x, mag, tab):
    c = nsgt_error.encode_f32(np.asarray(x, dtype=np.float32), tab)
    a = np.abs(c)
    m = np.asarray(mag, dtype=np.float32).reshape(c.shape)
    p = np.where(a > 0, m * c / np.where(a > 0, a, 1), m + 0j).astype(np.complex64)
    return nsgt_error.decode_f32(p, tab), convergence_f32(a, m, tab['max_window_length'])


def sequence_f32(x0, mag, tab, n_iter, alpha):
    x = np.asarray(x0, dtype=np.float32)
    ys, conv = [], []
    for k in range(n_iter):
        y, cv = step_f32(x, mag, tab)
        conv.append(cv)
        x = y if not ys else (y + np.float32(alpha) * (y - ys[-1])).astype(np.float32)
        ys.append(y)
    return ys, np.stack(conv)


# ---- cases, computed once and shared (read-only) ---------------------------------------------------------------------------------------

def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def case_inputs(n):
    """(audio float32 (2, 1, 2 n), mag float32 (2, F, 2 M))"""
    return G.magnitude_case(n)[:2]


@functools.lru_cache(maxsize=None)
def step_case(n):
    """(y float64 (2, 1, 2 n), projected coefficients, convergence (2,)) of one step from the case's audio"""
    a, mag = case_inputs(n)
    return _frozen(*step(a, mag, tables(n)))


@functools.lru_cache(maxsize=None)
def step_bar(n, generic):
    """float64 (2, 2): the bar of every sample of a block, constant 1"""
    y, p, _ = step_case(n)
    tab = tables(n)
    return _frozen(nsgt_error.decode_bar(p, tab, nsgt_error.fft_stages(n, generic), reference=y))[0]


@functools.lru_cache(maxsize=None)
def silent_case(n):
    """the zero-phase synthesis decode(mag + 0i) and its bar with the specialised / any-length stage count: (y, bar, bar_generic)"""
    _, mag = case_inputs(n)
    tab = tables(n)
    p = mag[:, None].astype(np.complex128)
    y = nsgt.decode(p, tab)
    return _frozen(y, *(nsgt_error.decode_bar(p, tab, nsgt_error.fft_stages(n, g), reference=y) for g in (False, True)))


@functools.lru_cache(maxsize=None)
def sequence_case(n):
    """(tuple of y_0 .. y_7 float64, convergence (8, 2)) from the case's audio with alpha = 0.99"""
    a, mag = case_inputs(n)
    ys, conv = sequence(a, mag, tables(n), N_SEQ, ALPHA)
    return tuple(_frozen(*ys)), _frozen(conv)[0]


def block_ratio(got, ref, bar):
    """worst |got - float64| / bar over the blocks (bar (B, blocks))"""
    B, nblk = bar.shape
    err = np.abs(np.asarray(got, dtype=np.float64) - ref).reshape(B, nblk, -1).max(-1)
    return float((err / bar).max())


def block_rms(ref, nblk=2):
    ref = np.asarray(ref, dtype=np.float64)
    return np.sqrt((ref.reshape(ref.shape[0], nblk, -1) ** 2).mean(-1))


def conv_ratio(got, ref):
    """worst relative distance of the convergence values"""
    return float((np.abs(np.asarray(got, dtype=np.float64) - ref) / ref).max())


def as_single_blocks(audio, mag, n):
    """the 2 clips x 2 blocks of a case as 4 clips x 1 block, in (clip, block) order"""
    m = tables(n)['max_window_length']
    a = None if audio is None else np.ascontiguousarray(audio.reshape(4, 1, n))
    g = np.ascontiguousarray(mag.reshape(2, F, 2, m).transpose(0, 2, 1, 3).reshape(4, F, m))
    return a, g


def restatement(n):
    """what float32 reaches on the case: (step ratio to its bar, sequence error / block rms after each step (8,), worst relative
    convergence error)"""
    a, mag = case_inputs(n)
    tab = tables(n)
    y32, _ = step_f32(a, mag, tab)
    r_step = block_ratio(y32, step_case(n)[0], step_bar(n, False))
    ys, conv = sequence_case(n)
    ys32, conv32 = sequence_f32(a, mag, tab, N_SEQ, ALPHA)
    r_seq = np.array([block_ratio(g, r, block_rms(r)) for g, r in zip(ys32, ys)])
    return r_step, r_seq, conv_ratio(conv32, conv)
