"""
CPU: the reference of the phase-retrieval tests is what it claims to be (tests/gl_ref.py), and the surface they test exists.

    * the constants K_STEP, K_SEQ, K_CONV follow their definition: the float32 restatement, re-measured here at both block lengths and
      held to K / 4 within 25 % (the recipe of test_gpu_cqt_parity.py::test_constants_follow_the_restatement);
    * the momentum identity in float64: extrapolating the projected coefficients and extrapolating the audio give the same sequence,
      because the synthesis is linear;
    * the reference's convergence values decrease strictly over the 8 steps of the case (an observed property, no theorem: in this frame
      analysis o synthesis is idempotent only to about 4e-3 at N = 11025 and 4e-2 at N = 66150), a silent start measures exactly 1 and
      gives the zero-phase synthesis, and the 0 / inf rules of the convergence hold;
    * CQT.from_decibels is the float64 expression 10^(4 (d - 1)) and inverts oracle.nsgt.to_decibels up to the item's peak;
    * include/ttrap.h declares the two entry points, the ctypes prototypes hold them, the library is at version 20 and refuses bad
      arguments before anything touches a device; CQT.griffin_lim and the models' sonify exist and refuse what they must.
"""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gl_ref as R
from oracle import nsgt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ('tt_cqt_griffin_lim_scratch_bytes', 'tt_cqt_griffin_lim')
LENGTHS = [R.N_FAST, R.N_SMALL]


def test_constants_follow_the_restatement():
    measured = [R.restatement(n) for n in LENGTHS]
    for name, (k, literal), r in (('K_STEP', R.K_STEP, max(m[0] for m in measured)),
                                  ('K_SEQ', R.K_SEQ, max(m[1][-1] for m in measured)),
                                  ('K_CONV', R.K_CONV, max(m[2] for m in measured))):
        print('float32 restatement, %-6s worst %.4e (literal %.4e, K %.3e)' % (name, r, literal, k))
        assert abs(k - 4 * literal) <= 0.005 * k, '%s is 4 times the measurement, rounded' % name
        assert r <= k / 4 * 1.25, (name, r, k)
    for n, m in zip(LENGTHS, measured):
        print('N = %d: float32 sequence error / block rms after each step: %s' % (n, ' '.join('%.2e' % v for v in m[1])))


@pytest.mark.parametrize('n', LENGTHS)
def test_momentum_in_the_audio_domain_equals_momentum_on_the_coefficients(n):
    a, mag = R.case_inputs(n)
    tab = R.tables(n)
    ys, _ = R.sequence(a, mag, tab, 4, R.ALPHA)
    yc = R.sequence_coefficient_domain(a, mag, tab, 4, R.ALPHA)
    worst = max(float(np.abs(u - v).max() / np.abs(v).max()) for u, v in zip(ys, yc))
    print('N = %d: the two forms differ by %.2e of the maximum over 4 steps' % (n, worst))
    assert worst <= 1e-11
    # and the extrapolation does something: without it the third audio is another
    plain, _ = R.sequence(a, mag, tab, 3, 0.0)
    assert np.abs(plain[2] - ys[2]).max() > 1e-3 * np.abs(ys[2]).max()


@pytest.mark.parametrize('n', LENGTHS)
def test_convergence_of_the_reference(n):
    ys, conv = R.sequence_case(n)
    print('N = %d: convergence per step, clip 0: %s' % (n, ' '.join('%.4f' % v for v in conv[:, 0])))
    assert conv.shape == (R.N_SEQ, 2) and (np.diff(conv, axis=0) < 0).all()
    # the start is the audio whose magnitudes were scaled by h in [0.5, 1.5]: sqrt(E (1 - h)^2 / E h^2) = sqrt(1 / 13)
    assert np.allclose(conv[0], np.sqrt(1.0 / 13.0), rtol=0.02)
    assert np.array_equal(R.step_case(n)[2], conv[0]) and np.array_equal(R.step_case(n)[0], ys[0])
    # silence: |c| == 0 everywhere, the projection is mag + 0i and the convergence exactly 1
    _, mag = R.case_inputs(n)
    y, p, cv = R.step(np.zeros_like(ys[0]), mag, R.tables(n))
    assert cv.tolist() == [1.0, 1.0] and not p.imag.any() and np.array_equal(p.real[:, 0], mag.astype(np.float64))
    assert np.array_equal(y, R.silent_case(n)[0])


def test_convergence_rules():
    z, one = np.zeros((2, 1, 3, 4)), np.ones((2, 1, 3, 4))
    assert R.convergence(z, z).tolist() == [0.0, 0.0]                    # 0 / 0: the numerator decides
    assert R.convergence(one, z).tolist() == [np.inf, np.inf]
    assert R.convergence(z, one).tolist() == [1.0, 1.0]
    assert R.convergence_f32(one, z, 4).tolist() == [np.inf, np.inf] and R.convergence_f32(z, z, 4).tolist() == [0.0, 0.0]
    mixed = np.stack([z[0], one[0]])
    assert R.convergence(mixed, np.stack([one[0], one[0]])).tolist() == [1.0, 0.0]          # per clip


def test_from_decibels():
    from timbre_trap.framework import CQT
    d = torch.linspace(0, 1, 4001, dtype=torch.float64)
    got = CQT.from_decibels(d)
    assert got.dtype == torch.float64
    np.testing.assert_allclose(got.numpy(), R.from_decibels(d.numpy()), rtol=1e-13)
    assert float(CQT.from_decibels(torch.tensor(0.0, dtype=torch.float64))) == pytest.approx(1e-4, rel=1e-12)
    assert float(CQT.from_decibels(torch.tensor(1.0))) == 1.0
    # float32 in, float32 out, a few ulps: the rounding of d - 1 enters multiplied by 4 ln 10
    d32 = d.float()
    np.testing.assert_allclose(CQT.from_decibels(d32).numpy().astype(np.float64), R.from_decibels(d32.numpy()), rtol=1e-6)
    # the inverse of to_decibels(rescale=True) up to each item's peak; what lies on the 80 dB floor comes back as 1e-4
    m = np.random.default_rng(7).uniform(0, 3, (2, 5, 16))
    m[0, 0, 0], m[1, 2, 3] = 0.0, 1e-9
    back = R.from_decibels(nsgt.to_decibels(m))
    peak = m.reshape(2, -1).max(-1)[:, None, None]
    want = np.maximum(m / peak, 1e-4)
    np.testing.assert_allclose(back, want, rtol=1e-12)


def test_header_and_prototypes_hold_the_entries():
    from timbre_trap import _hip
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ttrap.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(tt_[a-z0-9_]+)\s*\(', text))
    for name in NEW_ENTRIES:
        assert name in declared, '%s is not declared in include/ttrap.h' % name
        assert name in _hip.EXPORTED_SYMBOLS, '%s has no ctypes prototype' % name


def test_library_version_scratch_and_bad_arguments():
    from timbre_trap import _hip
    _hip.build()
    lib = _hip.lib()
    assert lib.tt_version() >= 20
    # the transform's own carve, two audio buffers and the partial sums
    q, f, s = 4, 540, 65649
    extra = lib.tt_cqt_griffin_lim_scratch_bytes(q, f, s) - lib.tt_cqt_scratch_bytes(q, f, s)
    assert 2 * q * 66150 * 4 + q * f * 8 <= extra <= 2 * q * 66150 * 4 + q * f * 8 + 3 * 256
    assert lib.tt_cqt_griffin_lim_scratch_bytes(0, f, s) == 0
    ps = _hip.CqtPlan()
    one = ctypes.c_void_p(256)
    ok = (ctypes.byref(ps), one, one, one, one, one, 1, 1, 1, 0.5, 0, None)

    def call(**change):
        args = list(ok)
        for i, v in change.items():
            args[int(i[1:])] = v
        return lib.tt_cqt_griffin_lim(*args)
    assert call(a0=None) == -1 and call(a1=None) == -1 and call(a3=None) == -1 and call(a5=None) == -1
    assert call(a6=0) == -1 and call(a7=0) == -1
    assert call(a8=0) == -1 and call(a8=-3) == -1                        # n_iter < 1
    assert call(a9=1.0) == -1 and call(a9=-0.25) == -1 and call(a9=float('nan')) == -1 and call(a9=2.0) == -1


def test_wrapper_surface():
    from timbre_trap.framework import CQT, TimbreTrap, TimbreTrapMag, TimbreTrapMagDB
    cq = CQT(9, 60, R.SR, 0.5)
    assert callable(getattr(cq, 'griffin_lim', None)) and callable(getattr(CQT, 'from_decibels', None))
    for cls in (TimbreTrap, TimbreTrapMag, TimbreTrapMagDB):
        assert callable(getattr(cls, 'sonify', None)), cls
    # no CPU fallback
    with pytest.raises(RuntimeError):
        cq.griffin_lim(torch.zeros(1, R.F, 128))
    with pytest.raises(RuntimeError):
        cq.griffin_lim(torch.zeros(1, 1, R.F, 128), n_iter=1)
    model = TimbreTrapMag(R.SR, 9, 60, 0.5, model_complexity=1)
    with pytest.raises(RuntimeError):
        model.sonify(torch.zeros(1, 1, R.F, 128))
