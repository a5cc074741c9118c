"""
Phase retrieval on the device (tt_cqt_griffin_lim, CQT.griffin_lim / from_decibels, the models' ``sonify``) against float64.

Reference, case, bars and the constants K live in tests/gl_ref.py; tests/test_gl_restatement.py (CPU) checks them.  Shapes: 2 clips x 2
blocks with every block different (the q -> (clip, block) map, the frame offset blk * M of the magnitude plane, the per-clip sums of the
convergence) on the specialised path ('fast', N = 66150: the fused kernel), on the any-length path ('small', N = 11025, M = 128: the
composed loop) and, for the single step, N = 66150 forced onto the any-length kernels.  Every check prints its ratio to the bar
(pytest -rP).

The kernels' worst figures, measured on an MI355X (N = 66150 / N = 11025 / N = 66150 forced onto the any-length kernels):
    one step, ratio to decode_bar (K 2.34)          0.471 / 0.222 / 0.247; the wrapper and the direct C call agree bit for bit
    silent start (same bar)                          0.315 / 0.186 against float64, 0 against synthesize(mag + 0i); conv[0] exactly 1
    eight steps, max error / block rms (K 4.08e-4)   fused 9.72e-5, composed 8.68e-5, fused against composed 9.07e-5 / 6.06e-5
    convergence, relative (K 1.67e-7)                3.2e-8 fused, 3.4e-8 composed, 6.4e-8 fused against composed / 6.6e-8
"""

import ctypes

import numpy as np
import pytest
import torch

import gl_ref as R

pytestmark = pytest.mark.gpu
N, N_SMALL = R.N_FAST, R.N_SMALL

_worst = {}


def _note(key, ratio, k):
    _worst[key] = max(_worst.get(key, 0.0), ratio)
    print('ratio to bar: %-56s %.4g (worst so far %.4g, K %.4g)' % (key, ratio, _worst[key], k))


@pytest.fixture(scope='module')
def cqs():
    """'fast': the specialised kernels; 'small': the short odd block length only the any-length kernels serve; 'forced': N = 66150 on the
    any-length kernels"""
    from timbre_trap.framework import CQT, cqtwrapper
    mp = pytest.MonkeyPatch()
    mp.setattr(cqtwrapper, 'FORCE_GENERIC', True)
    try:
        forced = CQT(9, 60, R.SR, 3).to('cuda')
    finally:
        mp.undo()
    fast, small = CQT(9, 60, R.SR, 3).to('cuda'), CQT(9, 60, R.SR, 0.5).to('cuda')
    assert fast._fast and not forced._fast and not small._fast
    assert (forced.block_length, small.block_length, small.max_window_length) == (N, N_SMALL, 128)
    return dict(fast=fast, small=small, forced=forced)


def _n(path):
    return N_SMALL if path == 'small' else N


def _inputs(n):
    a, mag = R.case_inputs(n)
    return torch.tensor(a).cuda(), torch.tensor(mag).cuda()


def _c_griffin_lim(cq, mag, init, n_iter, momentum, normalize, want_conv=True):
    """tt_cqt_griffin_lim called directly: mag (B, F, T) contiguous fp32, init (B, 1, L) or None -> (return code, audio, conv)"""
    from timbre_trap import _hip
    lib, ps = _hip.lib(), cq._plan_struct(mag.device)
    B, nblk = mag.size(0), mag.size(-1) // cq.max_window_length
    assert mag.is_contiguous() and mag.dtype == torch.float32 and (init is None or init.is_contiguous())
    out = torch.zeros((B, 1, nblk * cq.block_length), dtype=torch.float32, device=mag.device)
    conv = torch.zeros((max(n_iter, 1), B), dtype=torch.float32, device=mag.device) if want_conv else None
    scratch = torch.empty(lib.tt_cqt_griffin_lim_scratch_bytes(B * nblk, cq.n_bins, cq._sum_len), dtype=torch.uint8, device=mag.device)
    rc = lib.tt_cqt_griffin_lim(ctypes.byref(ps), _hip.ptr(mag), _hip.ptr(init), _hip.ptr(out), _hip.ptr(conv), _hip.ptr(scratch),
                                B, nblk, n_iter, momentum, int(normalize), _hip.stream_ptr())
    return rc, out, conv


# ---- 1. one step ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('path', ['fast', 'small', 'forced'])
def test_one_step(cqs, path):
    cq, n = cqs[path], _n(path)
    a, mag = _inputs(n)
    ref, _, conv_ref = R.step_case(n)
    bar, k = R.step_bar(n, path != 'fast'), R.K_STEP[0]
    got, conv = cq.griffin_lim(mag, n_iter=1, audio_init=a, normalize=False, return_convergence=True)
    assert got.shape == a.shape and conv.shape == (1, 2) and got.dtype == conv.dtype == torch.float32
    assert not got.requires_grad and bool(torch.isfinite(got).all())
    r = R.block_ratio(got.cpu().numpy(), ref, bar)
    _note('one step %s' % path, r, k)
    assert r <= k
    rc = R.conv_ratio(conv.cpu().numpy()[0], conv_ref)
    _note('one step %s convergence' % path, rc, R.K_CONV[0])
    assert rc <= R.K_CONV[0]
    # the (B, 1, F, T) form of the magnitudes, and no convergence asked: the same bits
    assert torch.equal(cq.griffin_lim(mag[:, None], n_iter=1, audio_init=a, normalize=False), got)
    if path == 'fast':
        rc_, direct, dconv = _c_griffin_lim(cq, mag, a, 1, 0.99, 0)
        assert rc_ == 0 and torch.equal(direct, got) and torch.equal(dconv, conv)


# ---- 2. silent start -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('path', ['fast', 'small'])
def test_silent_start_is_the_zero_phase_synthesis(cqs, path):
    cq, n = cqs[path], _n(path)
    _, mag = _inputs(n)
    ref, bar_fast, bar_generic = R.silent_case(n)
    bar, k = (bar_fast if path == 'fast' else bar_generic), R.K_STEP[0]
    got, conv = cq.griffin_lim(mag, n_iter=1, audio_init=None, normalize=False, return_convergence=True)
    zero_phase = cq.synthesize(torch.complex(mag, torch.zeros_like(mag))[:, None])
    for what, other in (('float64', ref), ('synthesize(mag + 0i)', zero_phase.cpu().numpy().astype(np.float64))):
        r = R.block_ratio(got.cpu().numpy(), other, bar)
        _note('silent start %s against %s' % (path, what), r, k)
        assert r <= k
    # (0 - mag)^2 and mag^2 are summed in the same order: exactly 1
    assert conv.cpu().tolist() == [[1.0, 1.0]]


# ---- 3. eight steps with momentum ------------------------------------------------------------------------------------------------------------

def _check_sequence(tag, audio, conv, n):
    ys, conv_ref = R.sequence_case(n)
    r = R.block_ratio(audio.cpu().numpy(), ys[-1], R.block_rms(ys[-1]))
    _note('eight steps %s audio' % tag, r, R.K_SEQ[0])
    assert r <= R.K_SEQ[0]
    c = conv.cpu().numpy().astype(np.float64)
    assert c.shape == conv_ref.shape
    rc = R.conv_ratio(c, conv_ref)
    _note('eight steps %s convergence' % tag, rc, R.K_CONV[0])
    assert rc <= R.K_CONV[0]
    assert (np.diff(c, axis=0) < 0).all(), c


@pytest.mark.parametrize('path', ['fast', 'small'])
def test_eight_steps_with_momentum(cqs, path):
    cq, n = cqs[path], _n(path)
    a, mag = _inputs(n)
    audio, conv = cq.griffin_lim(mag, n_iter=R.N_SEQ, momentum=R.ALPHA, audio_init=a, normalize=False, return_convergence=True)
    _check_sequence(path, audio, conv, n)
    if path == 'fast':
        mp = pytest.MonkeyPatch()
        mp.setattr(cq, '_gl_composed', True)
        try:
            audio_c, conv_c = cq.griffin_lim(mag, n_iter=R.N_SEQ, momentum=R.ALPHA, audio_init=a, normalize=False, return_convergence=True)
        finally:
            mp.undo()
        _check_sequence('fast, composed route', audio_c, conv_c, n)
        ref = audio_c.cpu().numpy().astype(np.float64)
        r = R.block_ratio(audio.cpu().numpy(), ref, R.block_rms(ref))
        _note('eight steps fast fused against composed', r, R.K_SEQ[0])
        assert r <= R.K_SEQ[0]
        rc = R.conv_ratio(conv.cpu().numpy(), conv_c.cpu().numpy().astype(np.float64))
        _note('eight steps fast fused against composed, convergence', rc, R.K_CONV[0])
        assert rc <= R.K_CONV[0]


# ---- 4. indexing ---------------------------------------------------------------------------------------------------------------------------

def test_two_by_two_equals_four_by_one(cqs):
    """nothing couples the blocks of a clip without the inf-norm: the same four block-clips as 4 clips x 1 block give the same bits, and
    a clip's convergence, a ratio of sums over its two blocks, lies between its blocks' own"""
    cq = cqs['fast']
    a_np, mag_np = R.case_inputs(N)
    a4_np, mag4_np = R.as_single_blocks(a_np, mag_np, N)
    a, mag, a4, mag4 = (torch.tensor(v).cuda() for v in (a_np, mag_np, a4_np, mag4_np))
    for init, init4 in ((a, a4), (None, None)):
        y, conv = cq.griffin_lim(mag, n_iter=3, momentum=0.99, audio_init=init, normalize=False, return_convergence=True)
        y4, conv4 = cq.griffin_lim(mag4, n_iter=3, momentum=0.99, audio_init=init4, normalize=False, return_convergence=True)
        assert torch.equal(y.reshape(4, 1, N), y4)
        c, c4 = conv.cpu().numpy(), conv4.cpu().numpy().reshape(3, 2, 2)
        assert (c4.min(-1) <= c).all() and (c <= c4.max(-1)).all(), (c, c4)


# ---- 5. determinism ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('path', ['fast', 'small'])
def test_two_runs_give_identical_bits(cqs, path):
    cq, n = cqs[path], _n(path)
    a, mag = _inputs(n)
    first = cq.griffin_lim(mag, n_iter=3, audio_init=a, return_convergence=True)
    second = cq.griffin_lim(mag, n_iter=3, audio_init=a, return_convergence=True)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


# ---- 6. the inf-norm -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('path', ['fast', 'small'])
def test_normalize(cqs, path):
    cq, n = cqs[path], _n(path)
    a, mag = _inputs(n)
    raw = cq.griffin_lim(mag, n_iter=2, audio_init=a, normalize=False)
    out = cq.griffin_lim(mag, n_iter=2, audio_init=a, normalize=True)
    want = raw / raw.abs().max()
    assert float(out.abs().max()) == 1.0
    assert bool(((out - want).abs() <= 2.0 ** -23 * want.abs()).all())
    # all-zero magnitudes: silence, no 0 / 0 anywhere, convergence 0
    for init in (None, a):
        audio, conv = cq.griffin_lim(torch.zeros_like(mag), n_iter=3, audio_init=init, normalize=True, return_convergence=True)
        assert not bool(audio.any()) and bool(torch.isfinite(audio).all())
        if init is None:
            assert not bool(conv.any())
        else:
            # a start that is not silent: |c| > 0 against magnitudes of 0 is +inf by the rule; silence from the next iteration on
            assert bool(torch.isinf(conv[0]).all()) and not bool(conv[1:].any())


# ---- 7. momentum 0 -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('path', ['fast', 'small'])
def test_momentum_zero_is_the_plain_iteration(cqs, path):
    cq, n = cqs[path], _n(path)
    a, mag = _inputs(n)
    audio, conv = cq.griffin_lim(mag, n_iter=8, momentum=0.0, audio_init=a, normalize=False, return_convergence=True)
    x, steps = a, []
    for _ in range(8):
        x, c = cq.griffin_lim(mag, n_iter=1, audio_init=x, normalize=False, return_convergence=True)
        steps.append(c)
    assert torch.equal(audio, x) and torch.equal(conv, torch.cat(steps))


# ---- 8. models -----------------------------------------------------------------------------------------------------------------------------

KW = dict(latent_size=None, model_complexity=1, skip_connections=False)


def test_models_sonify():
    """The model's own output to audio with one call on every variant.  The magnitude variants' output is what inference() returns,
    (B, 1, F, T) -- reconstruct() of the reference already passes through a complex decode and returns audio."""
    from timbre_trap.framework import CQT, TimbreTrap, TimbreTrapMag, TimbreTrapMagDB
    a = torch.tensor(R.case_inputs(N)[0][:1, :, :N]).cuda()
    torch.manual_seed(0)
    mag_model = TimbreTrapMag(R.SR, 9, 60, 3, **KW).cuda().eval()
    with torch.no_grad():
        m = mag_model.inference(a)
    assert m.shape == (1, 1, R.F, 1024) and bool(m.any())
    audio = mag_model.sonify(m, n_iter=4)
    assert audio.shape == a.shape and bool(torch.isfinite(audio).all()) and float(audio.abs().max()) == 1.0
    assert torch.equal(audio, mag_model.sliCQ.griffin_lim(m, n_iter=4))
    # the mixture-phase start
    mixed = mag_model.sonify(m, audio_init=a, n_iter=4)
    assert mixed.shape == a.shape and float(mixed.abs().max()) == 1.0 and not torch.equal(mixed, audio)

    db_model = TimbreTrapMagDB(R.SR, 9, 60, 3, **KW).cuda().eval()
    with torch.no_grad():
        d = db_model.inference(a)
    assert d.shape == (1, 1, R.F, 1024)
    assert torch.equal(db_model.sonify(d, n_iter=4), db_model.sliCQ.griffin_lim(CQT.from_decibels(d), n_iter=4))

    model = TimbreTrap(R.SR, 9, 60, 3, **KW).cuda().eval()
    with torch.no_grad():
        c = model.inference(a)
    assert torch.equal(model.sonify(c), model.sliCQ.decode(c))

    # from_decibels inverts to_decibels(rescale=True) up to the item's peak: against float64 on the same float32 d.  rtol 1e-6 is a few
    # float32 ulps: the rounding of d - 1 enters multiplied by 4 ln 10
    mags = mag_model.sliCQ.magnitude(a)
    dec = CQT.to_decibels(mags)
    back = CQT.from_decibels(dec)
    assert back.dtype == torch.float32 and back.shape == mags.shape
    np.testing.assert_allclose(back.cpu().numpy().astype(np.float64), R.from_decibels(dec.cpu().numpy()), rtol=1e-6, atol=0)
    assert float(CQT.from_decibels(torch.zeros(1, device='cuda'))) == pytest.approx(1e-4, rel=1e-6)


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals(cqs):
    cq = cqs['fast']
    a, mag = _inputs(N)
    with pytest.raises(ValueError):
        cq.griffin_lim(mag[:, :-1])                                      # a wrong F
    with pytest.raises(ValueError):
        cq.griffin_lim(mag[:, :, :-1])                                   # T no multiple of max_window_length
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError):
            cq.griffin_lim(mag, n_iter=bad)
    for bad in (-0.1, 1.0, 1.5, float('nan'), 1.0 - 1e-9):               # the last one is 1 in float32
        with pytest.raises(ValueError):
            cq.griffin_lim(mag, momentum=bad)
    with pytest.raises(ValueError):
        cq.griffin_lim(mag, audio_init=a[:, :, :-2])
    with pytest.raises(RuntimeError):
        cq.griffin_lim(mag.cpu())
    with pytest.raises(RuntimeError):
        cq.griffin_lim(mag, audio_init=a.cpu())
    # the C entry
    assert _c_griffin_lim(cq, mag, a, 0, 0.99, 0)[0] == -1
    assert _c_griffin_lim(cq, mag, a, 1, 1.0, 0)[0] == -1
    assert _c_griffin_lim(cq, mag, a, 1, -0.5, 0)[0] == -1
    from timbre_trap import _hip
    lib, ps = _hip.lib(), cq._plan_struct(mag.device)
    one = ctypes.c_void_p(256)
    assert lib.tt_cqt_griffin_lim(ctypes.byref(ps), None, one, one, one, one, 1, 1, 1, 0.5, 0, None) == -1
    assert lib.tt_cqt_griffin_lim(ctypes.byref(ps), one, None, None, one, one, 1, 1, 1, 0.5, 0, None) == -1
    assert lib.tt_cqt_griffin_lim(None, one, one, one, one, one, 1, 1, 1, 0.5, 0, None) == -1
