"""
CPU: the references of the constant-Q gradient tests are what they claim to be (tests/cqt_grad_ref.py), and the surface they test exists.

    * encode_t / decode_t (torch float64) equal oracle.nsgt.encode / decode to 1e-12 of the maximum at both block lengths;
    * torch autograd through them equals the exchanged-table vector-Jacobian products to 1e-12 -- analysis, synthesis and the magnitude,
      whose gradient is exactly 0 where the coefficients are 0 (one all-zero block);
    * the constants K of tests/test_gpu_cqt_grad.py follow their definition: the float32 restatement on the exchanged tables, re-measured
      here and held to K / 4 within 25 % (the recipe of test_gpu_cqt_parity.py::test_constants_follow_the_restatement);
    * include/ttrap.h declares the five adjoint entry points, the ctypes prototypes hold them, the library is at version 19 and CQT has
      ``analyze`` / ``synthesize``.
"""

import os
import re

import numpy as np
import pytest
import torch

import cqt_grad_ref as R
from oracle import nsgt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ('tt_cqt_forward_bwd', 'tt_cqt_inverse_bwd', 'tt_cqt_forward_mag_bwd', 'tt_cqt_generic_forward_bwd',
               'tt_cqt_generic_inverse_bwd')
LENGTHS = [R.N_FAST, R.N_SMALL]


def _rel(got, ref):
    return float(np.abs(np.asarray(got) - ref).max() / np.abs(ref).max())


def _coefficients(n, seed):
    m = R.tables(n)['max_window_length']
    rng = np.random.default_rng(seed + n)
    return rng.standard_normal((2, 1, R.F, 2 * m)) + 1j * rng.standard_normal((2, 1, R.F, 2 * m))


@pytest.mark.parametrize('n', LENGTHS)
def test_torch_restatements_equal_the_oracle(n):
    tab = R.tables(n)
    x = R.noise_audio(n).astype(np.float64)
    e = _rel(R.encode_t(torch.from_numpy(x), tab).numpy(), nsgt.encode(x, tab))
    c = _coefficients(n, 61)
    d = _rel(R.decode_t(torch.from_numpy(c), tab).numpy(), nsgt.decode(c, tab))
    print('N = %d: encode_t off the oracle by %.2e of the maximum, decode_t by %.2e' % (n, e, d))
    assert e <= 1e-12 and d <= 1e-12


@pytest.mark.parametrize('n', LENGTHS)
def test_autograd_equals_the_exchanged_table_products(n):
    tab = R.tables(n)
    x = R.noise_audio(n).astype(np.float64)
    # analysis: a complex grad_output is dL/dre + i dL/dim
    g = _coefficients(n, 62)
    xt = torch.from_numpy(x).requires_grad_()
    got, = torch.autograd.grad(R.encode_t(xt, tab), xt, grad_outputs=torch.from_numpy(g))
    ea = _rel(got.numpy(), R.analysis_vjp(g, tab))
    # synthesis
    y = np.random.default_rng(63 + n).uniform(-1, 1, x.shape)
    ct = torch.from_numpy(_coefficients(n, 64)).requires_grad_()
    got, = torch.autograd.grad(R.decode_t(ct, tab), ct, grad_outputs=torch.from_numpy(y))
    es = _rel(got.numpy(), R.synthesis_vjp(y, tab))
    print('N = %d: autograd off the exchanged-table products by %.2e (analysis), %.2e (synthesis) of the maximum' % (n, ea, es))
    assert ea <= 1e-12 and es <= 1e-12


@pytest.mark.parametrize('n', LENGTHS)
def test_magnitude_gradient_and_its_zero_guard(n):
    tab = R.tables(n)
    x = R.noise_audio(n).astype(np.float64).copy()
    x[1, 0, n:] = 0.0                                                    # the second block of the second clip: c == 0 there
    m = tab['max_window_length']
    dmag = np.random.default_rng(65 + n).uniform(0.5, 1.5, (2, 1, R.F, 2 * m))
    xt = torch.from_numpy(x).requires_grad_()
    got, = torch.autograd.grad(R.encode_t(xt, tab).abs(), xt, grad_outputs=torch.from_numpy(dmag))
    ref = R.magnitude_vjp(x, dmag, tab)
    assert not got[1, 0, n:].any() and not ref[1, 0, n:].any()          # exactly zero, in both
    assert not R.magnitude_direction(nsgt.encode(x, tab), dmag)[1, 0, :, m:].any()
    e = _rel(got.numpy(), ref)
    print('N = %d: autograd through |encode_t| off the magnitude product by %.2e of the maximum' % (n, e))
    assert e <= 1e-12


@pytest.mark.parametrize('direction,family', [('analysis', f) for f in R.K_ANALYSIS] + [('synthesis', f) for f in R.K_SYNTHESIS])
def test_constants_follow_the_restatement(direction, family):
    """K[family] / 4 is what torch.fft in complex64 reaches on the family with the exchanged tables, re-measured here at both block
    lengths: a literal that drifted from its definition (inputs, tables or bars changed without re-measuring) fails."""
    k, measured = (R.K_ANALYSIS if direction == 'analysis' else R.K_SYNTHESIS)[family]
    fn = R.restatement_analysis if direction == 'analysis' else R.restatement_synthesis
    r = max(fn(family, n) for n in LENGTHS)
    print('float32 restatement, %s %-10s worst ratio to the bar %.4f (literal %.4f, K %.2f)' % (direction, family, r, measured, k))
    assert abs(k - 4 * measured) <= 0.006, 'K is 4 times the measurement, rounded to two places'
    assert r <= k / 4 * 1.25, (r, k)


def test_header_and_prototypes_hold_the_adjoint_entries():
    from timbre_trap import _hip
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ttrap.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(tt_[a-z0-9_]+)\s*\(', text))
    for name in NEW_ENTRIES:
        assert name in declared, '%s is not declared in include/ttrap.h' % name
        assert name in _hip.EXPORTED_SYMBOLS, '%s has no ctypes prototype' % name


def test_library_version_and_bad_arguments():
    from timbre_trap import _hip
    _hip.build()
    lib = _hip.lib()
    assert lib.tt_version() >= 19
    # null pointers and non-positive sizes are refused before anything touches a device
    ps, gs = _hip.CqtPlan(), _hip.CqtGenericPlan()
    import ctypes
    one = ctypes.c_void_p(256)
    assert lib.tt_cqt_forward_bwd(None, one, one, one, 1, 1, 0, None) == -1
    assert lib.tt_cqt_forward_bwd(ctypes.byref(ps), None, one, one, 1, 1, 0, None) == -1
    assert lib.tt_cqt_forward_bwd(ctypes.byref(ps), one, one, one, 0, 1, 0, None) == -1
    assert lib.tt_cqt_inverse_bwd(ctypes.byref(ps), one, None, one, 1, 1, 0, None) == -1
    assert lib.tt_cqt_inverse_bwd(ctypes.byref(ps), one, one, one, 1, -1, 0, None) == -1
    assert lib.tt_cqt_forward_mag_bwd(ctypes.byref(ps), one, None, one, one, 1, 1, None) == -1
    assert lib.tt_cqt_forward_mag_bwd(ctypes.byref(ps), one, one, one, None, 1, 1, None) == -1
    assert lib.tt_cqt_generic_forward_bwd(ctypes.byref(gs), one, one, one, 1, 1, 0, None) == -1          # an empty plan
    assert lib.tt_cqt_generic_inverse_bwd(None, one, one, one, 1, 1, 0, None) == -1


def test_wrapper_surface():
    from timbre_trap.framework import CQT
    cq = CQT(9, 60, R.SR, 0.5)
    for name in ('analyze', 'synthesize', 'encode', 'magnitude'):
        assert callable(getattr(cq, name, None)), name
    # no CPU fallback, with or without autograd
    for audio in (torch.zeros(1, 1, R.N_SMALL), torch.zeros(1, 1, R.N_SMALL, requires_grad=True)):
        for fn in (cq.encode, cq.analyze, cq.magnitude):
            with pytest.raises(RuntimeError):
                fn(audio)
    with pytest.raises(RuntimeError):
        cq.synthesize(torch.zeros(1, 2, R.F, 128, requires_grad=True))
