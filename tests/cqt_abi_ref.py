"""
The constant-Q entry points of include/ttrap.h on bin layouts other than CQT(9, 60, 22050, 3), handed over through the C ABI: plans
whose tables are windows of the guarded arena of tests/cl16_ref.py, inputs, float64 references and bars.  Helper of
tests/test_cqt_layouts_restatement.py (CPU: tables, header sizes, the constants) and tests/test_gpu_cqt_abi_parity.py (the kernels).

Layouts (n_octaves, bins_per_octave, N) at 22050 Hz.  FAST run on csrc/cqt.hip (N = 66150, M = 1024): F = 549 and 531 are no multiple
of the four bins a workgroup of the band kernels serves, 420 has its lowest window far above spectral index 64, 540 is the control.
ANY run on csrc/cqt_generic.hip: M from 16 to 2048, even and odd N, N = 4096 with P = 2 N exactly, F from 4 to 1080.

Plan in the arena.  Every table is a window of its own, sized as include/ttrap.h states (gat_off [N / 2 + 2], bin_tab [F][4], ...), 16-byte
aligned, with cl16_ref.GUARD bytes of the fill behind it: a read one element past a table lands in the guard.

References, all float64 and all on the layout's own tables: oracle.nsgt.encode / decode, cqt_grad_ref.analysis_vjp / synthesis_vjp /
magnitude_vjp, gl_ref.step / sequence.  Bars: nsgt_error.encode_bar / decode_bar with the stage count of the path, for the adjoints on
the exchanged tables times the adjoint's constant (the rules of cqt_grad_ref), for Griffin-Lim the rules of gl_ref (one step: decode_bar
of the projected coefficients; later steps: a fraction of the block's rms; convergence: relative).

Families.  Entry points that take audio (forward, forward_mag, inverse_bwd): noise; impulses at samples 0, 1, N - 1, N / 2; tones on the
first and last spectral index any window reaches and on the centres of bin 0 and bin F - 1.  Entry points that take coefficients
(inverse, forward_bwd): the analysis of noise; random coefficients; single coefficients in bins 0 and F - 1 at frames 0 and M - 1.

Constants.  K[(entry, family, path)] is 4 times the worst ratio to the bar that the float32 restatement of the oracle
(nsgt_error.encode_f32 / decode_f32: torch.fft on complex64, on the same tables) reaches against float64 over ALL layouts of the path,
measured on the CPU and written below as a literal with the measurement beside it; tests/test_cqt_layouts_restatement.py re-measures
each and holds it to K / 4 within 25 %.  The factor 4 covers a different factorisation of the same transforms, nothing more
(tests/test_gpu_cqt_parity.py).  No constant comes from what a kernel returned.
"""

import ctypes
import functools
import math

import numpy as np
import torch

import cl16_ref as C
import cqt_grad_ref as G
import gl_ref
from oracle import nsgt, nsgt_error

SR = 22050
N_FAST = 66150
# layout -> (F, M)
FAST = {(9, 61, 66150): (549, 1024), (9, 59, 66150): (531, 1024), (7, 60, 66150): (420, 1024), (9, 60, 66150): (540, 1024)}
ANY = {(9, 120, 2205): (1080, 16), (9, 61, 2205): (549, 32), (5, 12, 2205): (60, 128), (3, 7, 2205): (21, 256), (1, 4, 2205): (4, 512),
       (5, 12, 735): (60, 64), (4, 9, 1001): (36, 128), (9, 59, 4096): (531, 64), (9, 24, 66150): (216, 2048)}
LAYOUTS = {'fast': tuple(FAST), 'any': tuple(ANY)}
REFUSED_LAYOUTS = ((9, 59, 2205), (9, 96, 2205))          # build_plan: a window leaves the open positive half-spectrum
GL_LAYOUTS = ((9, 61, 66150), (9, 59, 66150))
AUDIO_FAMILIES = ('noise', 'impulses', 'tones')
COEFF_FAMILIES = ('analysis', 'random', 'impulses')

FAST_TABLES = ('tw675', 'tw49', 'twNc', 'twN', 'tw1024', 'bin_tab', 'window', 'dual', 'gat_off', 'gat_idx')
ANY_TABLES = ('chirp', 'bfilt', 'twP', 'twM', 'bin_tab', 'window', 'dual', 'gat_off', 'gat_idx', 'pos_bin')

# (K, measured): K = 4 x measured, rounded up in the last digit.  Keys: (entry, family, path).  'forward' also bars forward_mag (the
# epilogue's own 2^-22 |c| is taken off first, as in tests/test_gpu_cqt_parity.py).
K = {
    # per-layout measurements beside each literal, in the order of LAYOUTS[path] (Griffin-Lim: GL_LAYOUTS)
    ('forward', 'noise', 'fast'):            (1.427, 0.3554),   # 0.3273, 0.2908, 0.2574, 0.3554
    ('forward', 'impulses', 'fast'):         (1.146, 0.2853),   # 0.2853, 0.25, 0.2655, 0.2669
    ('forward', 'tones', 'fast'):            (10.81, 2.692),   # 2.692, 2.692, 2.494, 2.692
    ('inverse_bwd', 'noise', 'fast'):        (1.369, 0.341),   # 0.341, 0.3395, 0.2622, 0.3074
    ('inverse_bwd', 'impulses', 'fast'):     (1.131, 0.2815),   # 0.2815, 0.27, 0.2604, 0.2604
    ('inverse_bwd', 'tones', 'fast'):        (10.81, 2.692),   # 2.692, 2.692, 1.908, 2.692
    ('inverse', 'analysis', 'fast'):         (1.679, 0.418),   # 0.3079, 0.2972, 0.418, 0.3542
    ('inverse', 'random', 'fast'):           (1.3, 0.3236),   # 0.2528, 0.3236, 0.2928, 0.3143
    ('inverse', 'impulses', 'fast'):         (1.509, 0.3758),   # 0.2821, 0.3758, 0.3115, 0.3115
    ('forward_bwd', 'analysis', 'fast'):     (1.416, 0.3525),   # 0.3288, 0.3311, 0.3525, 0.3171
    ('forward_bwd', 'random', 'fast'):       (1.392, 0.3466),   # 0.3091, 0.3466, 0.2792, 0.3044
    ('forward_bwd', 'impulses', 'fast'):     (6.261, 1.559),   # 1.559, 1.492, 1.38, 1.38
    ('forward', 'noise', 'any'):             (0.8233, 0.205),   # 0.205, 0.1768, 0.1339, 0.1079, 0.0773, 0.1835, 0.1458, 0.1667, 0.1421
    ('forward', 'impulses', 'any'):          (1.016, 0.253),   # 0.1362, 0.1673, 0.1649, 0.1721, 0.1277, 0.253, 0.1491, 0.1873, 0.2018
    ('forward', 'tones', 'any'):             (2.117, 0.5272),   # 0.5272, 0.4235, 0.3326, 0.2346, 0.156, 0.2577, 0.2998, 0.2874, 0.4657
    ('inverse_bwd', 'noise', 'any'):         (0.8269, 0.2059),   # 0.1749, 0.1869, 0.1469, 0.1504, 0.1654, 0.189, 0.1457, 0.2059, 0.1427
    ('inverse_bwd', 'impulses', 'any'):      (0.7795, 0.1941),   # 0.1627, 0.1624, 0.1805, 0.1463, 0.1627, 0.1596, 0.131, 0.1691, 0.1941
    ('inverse_bwd', 'tones', 'any'):         (2.62, 0.6525),   # 0.4878, 0.4625, 0.3831, 0.3076, 0.3355, 0.3664, 0.2555, 0.3397, 0.6525
    ('inverse', 'analysis', 'any'):          (2.015, 0.5017),   # 0.2342, 0.1731, 0.3085, 0.5017, 0.3762, 0.3014, 0.2867, 0.2407, 0.3333
    ('inverse', 'random', 'any'):            (0.8598, 0.2141),   # 0.2047, 0.1696, 0.1983, 0.1831, 0.2141, 0.175, 0.1606, 0.1688, 0.1718
    ('inverse', 'impulses', 'any'):          (1.094, 0.2725),   # 0.1815, 0.1733, 0.204, 0.1237, 0.126, 0.1442, 0.137, 0.1056, 0.2725
    ('forward_bwd', 'analysis', 'any'):      (1.68, 0.4183),   # 0.4183, 0.2542, 0.166, 0.1847, 0.1674, 0.1943, 0.1998, 0.2139, 0.1561
    ('forward_bwd', 'random', 'any'):        (0.8197, 0.2041),   # 0.1324, 0.161, 0.1665, 0.1977, 0.1879, 0.1858, 0.2041, 0.1813, 0.1686
    ('forward_bwd', 'impulses', 'any'):      (4.289, 1.068),   # 0.2146, 0.217, 0.4316, 0.3786, 0.5172, 0.3677, 0.3145, 0.3477, 1.068
    ('magnitude_bwd', 'case', 'fast'):       (1.706, 0.4249),   # 0.3791, 0.4249, 0.407, 0.3903
    ('gl_step', 'case', 'fast'):             (1.767, 0.4399),   # 0.4399, 0.3787
    ('gl_seq2', 'case', 'fast'):             (0.0004606, 0.0001147),   # 0.0001085, 0.0001147
    ('gl_seq3', 'case', 'fast'):             (0.0006301, 0.0001569),   # 0.0001569, 0.0001491
    ('gl_conv', 'case', 'fast'):             (8.791e-07, 2.189e-07),   # 2.106e-07, 2.189e-07
}


def path_of(layout):
    return 'fast' if layout in FAST else 'any'


def shapes(layout):
    """(B, n_blocks) of the noise-like families"""
    return ((1, 1), (2, 2)) if layout[2] == N_FAST else ((1, 1), (1, 2), (3, 2))


def big_shape(layout):
    return shapes(layout)[-1]


@functools.lru_cache(maxsize=None)
def tables(layout):
    return nsgt.nsgt_tables(layout[0], layout[1], SR, layout[2])


@functools.lru_cache(maxsize=None)
def plan(layout):
    from timbre_trap.framework import nsgt_plan
    return nsgt_plan.build_plan(layout[0], layout[1], SR, layout[2], generic=(path_of(layout) == 'any'))


def stages(layout):
    return nsgt_error.fft_stages(layout[2], path_of(layout) == 'any')


def header_sizes(layout):
    """table -> elements of its type that include/ttrap.h states (float2 tables count two floats per entry)"""
    p = plan(layout)
    F, S, N = p['n_bins'], p['sum_len'], p['N']
    ragged = dict(bin_tab=4 * F, window=S, dual=S, gat_off=N // 2 + 2, gat_idx=S)
    if p['fast']:
        return dict(tw675=2 * 675, tw49=2 * 49, twNc=2 * 49 * 675, twN=2 * 33076, tw1024=2 * 1024, **ragged)
    return dict(chirp=2 * N, bfilt=2 * p['P'], twP=2 * (p['P'] // 2), twM=2 * (p['M'] // 2), pos_bin=S, **ragged)


@functools.lru_cache(maxsize=None)
def plan_tensors(layout):
    """table -> flat float32 / int32 tensor, exactly as long as the header states"""
    p = plan(layout)
    out = {}
    for name, n in header_sizes(layout).items():
        a = np.ascontiguousarray(p[name])
        t = torch.from_numpy(a).to(torch.int32 if a.dtype.kind == 'i' else torch.float32).reshape(-1).contiguous()
        assert t.numel() == n, (layout, name, t.numel(), n)
        out[name] = t
    return out


def add_plan(A, layout):
    for name, t in plan_tensors(layout).items():
        A.inp('t_' + name, t)


def plan_struct(A, layout, **override):
    """the tt_cqt_plan / tt_cqt_gplan whose tables are the arena's windows (after A.build()); ``override``: fields set to other values"""
    from timbre_trap import _hip
    p = plan(layout)
    ps = _hip.CqtPlan() if p['fast'] else _hip.CqtGenericPlan()
    for name in (FAST_TABLES if p['fast'] else ANY_TABLES):
        ptr = A.ptr('t_' + name).value
        assert ptr % 16 == 0
        setattr(ps, name, ptr)
    ps.n_bins, ps.sum_len = p['n_bins'], p['sum_len']
    if not p['fast']:
        ps.N, ps.M, ps.P = p['N'], p['M'], p['P']
    for k, v in override.items():
        setattr(ps, k, v)
    return ps


def _a256(v):
    return (v + 255) // 256 * 256


def scratch_carve(layout, Q, griffin_lim=False):
    """the bytes of scratch, from the carve of the two sources written out: csrc/cqt.hip  mx word (256) | A [Q][33075] float2 |
    X [Q][33088] float2 | S [Q][sum_len] float2, Griffin-Lim adds two audio buffers [Q][66150] float and the partial sums [Q][F][2] float;
    csrc/cqt_generic.hip  peak word (256) | two work buffers of max(Q F M, Q P) float2 | the half spectra [Q][N / 2 + 1] float2; every
    region rounded up to 256 bytes"""
    p = plan(layout)
    F, S = p['n_bins'], p['sum_len']
    if p['fast']:
        n = 256 + _a256(Q * 33075 * 8) + _a256(Q * 33088 * 8) + _a256(Q * S * 8)
        return n + (2 * _a256(Q * 33075 * 8) + _a256(Q * F * 8) if griffin_lim else 0)
    assert not griffin_lim
    return 256 + 2 * _a256(max(Q * F * p['M'], Q * p['P']) * 8) + _a256(Q * (p['N'] // 2 + 1) * 8)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------

def _seed(layout, *more):
    return [17, *layout, *more]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _tone(j, n):
    t = np.arange(n, dtype=np.int64)
    return np.cos(2.0 * np.pi * ((j * t) % n) / n + 0.3)                 # the phase reduced exactly


def family_shape(layout, family, shape=None):
    return (4, 1) if family in ('impulses', 'tones') else (shape or big_shape(layout))


@functools.lru_cache(maxsize=None)
def audio(layout, family, shape=None):
    """float32 (B, 1, n_blocks N)"""
    tab, n = tables(layout), layout[2]
    B, nb = family_shape(layout, family, shape)
    if family == 'noise':
        x = np.random.default_rng(_seed(layout, 1, B, nb)).uniform(-1, 1, (B, nb * n))
    elif family == 'impulses':
        x = np.zeros((4, n))
        for b, i in enumerate((0, 1, n - 1, n // 2)):
            x[b, i] = 1.0
    elif family == 'tones':
        si, pos = tab['spec_index'], tab['positions']
        x = np.stack([_tone(int(j), n) for j in (si.min(), si.max(), pos[0], pos[-1])])
    else:
        raise KeyError(family)
    return _frozen(np.ascontiguousarray(x[:, None, :].astype(np.float32)))[0]


@functools.lru_cache(maxsize=None)
def coeffs(layout, family, shape=None):
    """complex64 (B, 1, F, n_blocks M)"""
    tab = tables(layout)
    F, m, n = tab['n_bins'], tab['max_window_length'], layout[2]
    B, nb = family_shape(layout, family, shape)
    rng = np.random.default_rng(_seed(layout, 2, B, nb))
    if family == 'analysis':
        c = nsgt.encode(rng.uniform(-1, 1, (B, 1, nb * n)), tab)
    elif family == 'random':
        c = rng.standard_normal((B, 1, F, nb * m)) + 1j * rng.standard_normal((B, 1, F, nb * m))
    elif family == 'impulses':
        c = np.zeros((4, 1, F, m), dtype=np.complex128)
        c[0, 0, 0, 0] = 1.0
        c[1, 0, 0, m - 1] = 1.0j
        c[2, 0, F - 1, 0] = 0.6 - 0.8j
        c[3, 0, F - 1, m - 1] = 1.0
    else:
        raise KeyError(family)
    return _frozen(np.ascontiguousarray(c.astype(np.complex64)))[0]


def planes(c):
    """complex (B, 1, F, T) -> float32 (B, 2, F, T)"""
    return np.ascontiguousarray(np.stack([c[:, 0].real, c[:, 0].imag], 1).astype(np.float32))


def interleaved(c):
    """complex (B, 1, F, T) -> float32 (B, 1, F, T, 2)"""
    return np.ascontiguousarray(np.stack([c.real, c.imag], -1).astype(np.float32))


def to_complex(got, is_complex):
    """the float32 output of an entry point, planes (B, 2, F, T) or interleaved (B, 1, F, T, 2) -> complex128 (B, 1, F, T)"""
    g = np.asarray(got, dtype=np.float64)
    return (g[..., 0] + 1j * g[..., 1]) if is_complex else (g[:, 0] + 1j * g[:, 1])[:, None]


# ---- references and bars (float64; computed once, shared, read-only) ------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case(entry, layout, family, shape=None):
    """(input, float64 reference, bar with constant 1) of one entry point.  entry: 'forward' | 'inverse' | 'forward_bwd' | 'inverse_bwd'.
    Bars: (B, n_blocks, F) for coefficient outputs, (B, n_blocks) for audio outputs."""
    tab, st = tables(layout), stages(layout)
    N, M = tab['block_length'], tab['max_window_length']
    adj = G.adjoint_tables(tab)
    if entry == 'forward':
        x = audio(layout, family, shape)
        ref, bar = nsgt.encode(x.astype(np.float64), tab), nsgt_error.encode_bar(x, tab, st)
    elif entry == 'inverse_bwd':
        x = audio(layout, family, shape)
        ref, bar = G.synthesis_vjp(x.astype(np.float64), tab), (2.0 * M / N) * nsgt_error.encode_bar(x, adj, st)
    elif entry == 'inverse':
        x = coeffs(layout, family, shape)
        ref = nsgt.decode(x.astype(np.complex128), tab)
        bar = nsgt_error.decode_bar(x, tab, st, reference=ref)
    elif entry == 'forward_bwd':
        x = coeffs(layout, family, shape)
        ref = G.analysis_vjp(x, tab)
        scale = N / (2.0 * M)
        bar = scale * nsgt_error.decode_bar(x, adj, st, reference=ref / scale)
    else:
        raise KeyError(entry)
    return (x,) + _frozen(ref, bar)


def coeff_ratio(got, ref, bar, magnitude=False):
    """worst |got - float64| / bar over every frame of every (clip, block, bin); got, ref (B, 1, F, T), bar (B, n_blocks, F)"""
    B, nb, F = bar.shape
    if magnitude:
        # | got - |ref| | <= bar + 2^-22 |ref|: the square root and the two squares of the epilogue on top of the coefficient's own error
        err = np.maximum(np.abs(got - np.abs(ref)) - 2.0 ** -22 * np.abs(ref), 0.0)
    else:
        err = np.abs(got - ref)
    assert err.shape[:3] == (B, 1, F) and err.shape[3] % nb == 0, (err.shape, bar.shape)
    err = err.reshape(B, F, nb, -1).max(-1).transpose(0, 2, 1)
    assert (bar > 0).all()
    return float((err / bar).max())


def audio_ratio(got, ref, bar):
    """worst |got - float64| / bar over the blocks; got, ref (B, 1, n_blocks N), bar (B, n_blocks).  A block whose bar is zero (nothing
    reaches it in float64) must be exactly zero."""
    B, nb = bar.shape
    assert tuple(got.shape) == tuple(ref.shape), (got.shape, ref.shape)
    err = np.abs(np.asarray(got, dtype=np.float64) - ref).reshape(B, nb, -1).max(-1)
    assert not (err[bar == 0] != 0).any(), 'a block nothing reaches is not exactly zero'
    return float((err[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0


def ratio(entry, got, ref, bar):
    return coeff_ratio(got, ref, bar) if entry in ('forward', 'inverse_bwd') else audio_ratio(got, ref, bar)


@functools.lru_cache(maxsize=None)
def magnitude_case(layout):
    """(audio float32 (B, 1, n N), dmag float32 (B, 1, F, n M) = h |c| with h uniform in [0.5, 1.5] (dc = h c: well conditioned),
    float64 gradient w.r.t. the audio, its bar with constant 1 (B, n))"""
    tab, st = tables(layout), stages(layout)
    N, M = tab['block_length'], tab['max_window_length']
    a = audio(layout, 'noise', (2, 2))
    c = nsgt.encode(a.astype(np.float64), tab)
    h = np.random.default_rng(_seed(layout, 3)).uniform(0.5, 1.5, c.shape)
    dmag = np.ascontiguousarray((h * np.abs(c)).astype(np.float32))
    dc = G.magnitude_direction(c, dmag)
    ref = G.analysis_vjp(dc, tab)
    scale = N / (2.0 * M)
    bar = scale * nsgt_error.decode_bar(dc, G.adjoint_tables(tab), st, reference=ref / scale)
    return (a,) + _frozen(dmag, ref, bar)


# ---- Griffin-Lim (csrc/cqt.hip only) ---------------------------------------------------------------------------------------------------

GL_ITERS, GL_ALPHAS = (1, 2, 3), (0.0, 0.99)


@functools.lru_cache(maxsize=None)
def gl_inputs(layout):
    """(audio float32 (2, 1, 2 N), mag float32 (2, 1, F, 2 M)): the case of gl_ref on this layout's tables"""
    a, dmag = magnitude_case(layout)[:2]
    return a, dmag


@functools.lru_cache(maxsize=None)
def gl_case(layout, init, alpha):
    """float64: (y_0, y_1, y_2), convergence (3, B), bar of y_0 with constant 1 (B, n).  init: start from the case's audio, else silence."""
    a, mag = gl_inputs(layout)
    tab = tables(layout)
    x0 = a.astype(np.float64) if init else None
    ys, conv = gl_ref.sequence(x0, mag[:, 0], tab, 3, alpha)
    _, p0, _ = gl_ref.step(np.zeros_like(ys[0]) if x0 is None else x0, mag[:, 0], tab)
    bar0 = nsgt_error.decode_bar(p0, tab, stages(layout), reference=ys[0])
    return tuple(_frozen(*ys)), _frozen(conv)[0], _frozen(bar0)[0]


def gl_restatement(layout, init, alpha):
    """what float32 reaches: (ratio of y_0 to its bar, [error / block rms of y_1, y_2], worst relative convergence error over the values
    that are not exactly 1)"""
    a, mag = gl_inputs(layout)
    tab = tables(layout)
    ys, conv, bar0 = gl_case(layout, init, alpha)
    x0 = a if init else np.zeros_like(a)
    ys32, conv32 = gl_ref.sequence_f32(x0, mag[:, 0], tab, 3, alpha)
    seq = [gl_ref.block_ratio(g, r, gl_ref.block_rms(r)) for g, r in zip(ys32[1:], ys[1:])]
    return gl_ref.block_ratio(ys32[0], ys[0], bar0), seq, gl_ref.conv_ratio(conv32, conv)


# ---- what float32 reaches (CPU; compared with float64 only, never with the kernels) -----------------------------------------------------

def restatement(entry, family, path):
    """worst ratio to the bar of the float32 restatement over every layout of the path, on the largest batch shape of each"""
    worst = 0.0
    for layout in LAYOUTS[path]:
        if entry in ('magnitude_bwd', 'gl_step', 'gl_seq2', 'gl_seq3', 'gl_conv'):
            if layout not in (GL_LAYOUTS if entry.startswith('gl_') else FAST):
                continue
        worst = max(worst, restatement_one(entry, family, layout))
    return worst


def restatement_one(entry, family, layout):
    tab = tables(layout)
    N, M = tab['block_length'], tab['max_window_length']
    adj = G.adjoint_tables(tab)
    if entry == 'magnitude_bwd':
        a, dmag, ref, bar = magnitude_case(layout)
        c = nsgt_error.encode_f32(a, tab)
        mag = np.abs(c)
        dc = np.where(mag > 0, dmag * c / np.where(mag > 0, mag, 1), 0).astype(np.complex64)
        got = nsgt_error.decode_f32(dc, adj).astype(np.float64) * (N / (2.0 * M))
        return audio_ratio(got, ref, bar)
    if entry.startswith('gl_'):
        worst = 0.0
        for init in (True, False):
            for alpha in GL_ALPHAS:
                r0, seq, rc = gl_restatement(layout, init, alpha)
                worst = max(worst, {'gl_step': r0, 'gl_seq2': seq[0], 'gl_seq3': seq[1], 'gl_conv': rc}[entry])
        return worst
    x, ref, bar = case(entry, layout, family)
    if entry == 'forward':
        got = nsgt_error.encode_f32(x, tab).astype(np.complex128)
    elif entry == 'inverse_bwd':
        got = nsgt_error.encode_f32(x, adj).astype(np.complex128) * (2.0 * M / N)
    elif entry == 'inverse':
        got = nsgt_error.decode_f32(x, tab).astype(np.float64)
    else:
        got = nsgt_error.decode_f32(x, adj).astype(np.float64) * (N / (2.0 * M))
    return ratio(entry, got, ref, bar)


def constant_keys():
    keys = []
    for path in ('fast', 'any'):
        keys += [(e, f, path) for e in ('forward', 'inverse_bwd') for f in AUDIO_FAMILIES]
        keys += [(e, f, path) for e in ('inverse', 'forward_bwd') for f in COEFF_FAMILIES]
    keys += [(e, 'case', 'fast') for e in ('magnitude_bwd', 'gl_step', 'gl_seq2', 'gl_seq3', 'gl_conv')]
    return keys
