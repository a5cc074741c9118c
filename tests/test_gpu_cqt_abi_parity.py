"""
Float64 parity of the constant-Q entry points (csrc/cqt.hip, csrc/cqt_generic.hip) on bin layouts other than CQT(9, 60, 22050, 3), called
through the C ABI of include/ttrap.h with every operand, every plan table and the scratch a window of one guarded arena
(tests/cqt_abi_ref.py on tests/cl16_ref.Arena).  The four older CQT files build one layout (F = 540, a multiple of the four bins a
workgroup of the band kernels serves) and go through the Python wrapper, whose torch allocations have slack behind them.

Layouts: the four FAST and nine ANY layouts of cqt_abi_ref (F % 4 = 1 and 3, one-sample windows, a lowest window far above index 64;
M = 16 .. 2048, odd N, P = 2 N exactly).  Batch shapes (B, n_blocks): (1, 1), (1, 2), (3, 2) on the small layouts, (1, 1), (2, 2) at
N = 66150.  After every call: the guard bands, the inputs and all plan tables are bit-unchanged, every output element (prefilled with
the arena's fill: NaN bytes, or 0x46 bytes) was written and is finite, and every element is within its bar; both fills and both
settings of out_complex / in_complex run.  Scratch is exactly what the *_scratch_bytes functions return, on a 256-byte boundary.

Every check prints its ratio to the bar (pytest -rP).  Constants, references and bars: cqt_abi_ref (K = 4 x the float32 restatement,
measured on the CPU, each literal with its measurement there).

Misaligned data pointers (one pointer shifted by one float, the others aligned), decided from the code before the first run --
there is no LDS-DMA in either file, but csrc/cqt.hip reinterprets audio as float2 and coefficient planes as float4:
    csrc/cqt.hip          refused (TT_E_BADARG, nothing launched): audio / daudio / audio_init / audio_out of every entry point (float2
                          loads and stores: k_fft675_rows, k_fft49_cols, k_scale_by_max, k_gl_extrapolate); out of tt_cqt_forward and
                          tt_cqt_forward_mag, dcoeffs of tt_cqt_inverse_bwd (float4 stores of k_band_fwd); interleaved complex coeffs /
                          dcoeffs of tt_cqt_inverse / tt_cqt_forward_bwd (float2 loads of k_band_inv)
                          same bars: coeffs / dcoeffs as planes of tt_cqt_inverse / tt_cqt_forward_bwd (one float per lane), dmag of
                          tt_cqt_forward_mag_bwd, mag and conv of tt_cqt_griffin_lim
    csrc/cqt_generic.hip  same bars: every audio pointer and every plane pointer (one float per thread); refused: interleaved complex
                          out / coeffs / dcoeffs (float2)
    every entry point     refused: scratch off its 256-byte boundary
Every pair behaved on an MI355X as decided: the served ones at the ratios below, the refused ones with the whole buffer untouched.

Deliberate breaks, each made in a copy of the sources outside the repository and run once (none forms a wild address):
    band-forward grid F / 4 instead of (F + 3) / 4      17 cases fail, all on (9, 61) and (9, 59): forward, inverse_bwd (3 families
                                                        each), forward_mag, the forward scratch-reuse case and the wrapper test, with
                                                        "output ... was not written everywhere" (first missing element: bin 548 / 528);
                                                        tests/test_gpu_cqt.py, test_gpu_cqt_parity.py, test_gpu_cqt_grad.py and
                                                        test_gpu_griffin_lim.py pass with it, all 106 cases: the gap this file closes
    memset of the peak word dropped (inverse tail)      test_normalize_is_raw_over_its_peak under the NaN-byte scratch, the normalised
                                                        twins of test_griffin_lim_on_layout, the inverse scratch-reuse case, the wrapper test
    k_g_ola drops the last gat_idx entry of an index    inverse and forward_bwd on all nine any-length layouts (ratios of 1e5 and more)
    k_spec_gather drops the last gat_idx entry          inverse and forward_bwd on all four fast layouts, forward_mag_bwd, Griffin-Lim
    k_band_mag_bwd: one lane skips its stores           test_magnitude_on_layout on all four fast layouts
    adjoint tail (k_fft49_cols<2>) scales by 1 / NC     forward_bwd on all four fast layouts, forward_mag_bwd
    k_band_project negates the imaginary part           test_griffin_lim_on_layout, all four cases
    k_g_fft_r4 loses the sign of its third twiddle      every transform on all nine any-length layouts

MEASURED on an MI355X: 184 cases in 16 s (the slowest 0.7 s).  Worst ratio to the bar with constant 1 per entry point and family,
csrc/cqt.hip / csrc/cqt_generic.hip, then K of the two paths in brackets (K = 4 x the CPU measurement listed beside it in cqt_abi_ref.K):
    forward       noise 0.381 / 0.298 [1.427 / 0.8233], impulses 0.305 / 0.276 [1.146 / 1.016], tones 4.30 / 1.00 [10.81 / 2.117]
    forward_mag   noise 0.257, impulses 0.192, tones 4.27 [the constants of forward]
    inverse       analysis 0.372 / 0.455 [1.679 / 2.015], random 0.425 / 0.290 [1.3 / 0.8598], impulses 0.545 / 0.310 [1.509 / 1.094]
    forward_bwd   analysis 0.469 / 0.457 [1.416 / 1.68], random 0.370 / 0.288 [1.392 / 0.8197], impulses 2.80 / 1.36 [6.261 / 4.289]
    inverse_bwd   noise 0.383 / 0.252 [1.369 / 0.8269], impulses 0.346 / 0.313 [1.131 / 0.7795], tones 5.22 / 0.902 [10.81 / 2.62]
    forward_mag_bwd 0.497 [1.706] (the same with dmag off by one float)
    griffin_lim   one step 0.431 of decode_bar [1.767]; y_1 9.99e-5 and y_2 1.65e-4 of the block's rms (K 4.61e-4, 6.30e-4); convergence 5.03e-7
                  relative (K 8.79e-7); two steps with mag or conv off by one float 6.3e-6 of the block's rms
normalize = 1 equalled raw / peak bit for bit under both scratch fills, a (1, 1) call after a (3, 2) call on the same scratch equalled a
fresh call bit for bit, and the wrapper equalled the C ABI bit for bit on all six layouts it was held against.
"""

import ctypes
import itertools

import numpy as np
import pytest
import torch

import cl16_ref as C
import cqt_abi_ref as R

gpu = pytest.mark.gpu
BADARG = -1
FILLS = (C.FILL_NAN, C.FILL_BIG)

# entry -> (symbol on csrc/cqt.hip, symbol on csrc/cqt_generic.hip, pointer operands in C order between `plan` and `scratch`)
SPEC = {
    'forward': ('tt_cqt_forward', 'tt_cqt_generic_forward', ('audio', 'out')),
    'forward_mag': ('tt_cqt_forward_mag', None, ('audio', 'out')),
    'inverse': ('tt_cqt_inverse', 'tt_cqt_generic_inverse', ('coeffs', 'audio')),
    'forward_bwd': ('tt_cqt_forward_bwd', 'tt_cqt_generic_forward_bwd', ('dcoeffs', 'daudio')),
    'inverse_bwd': ('tt_cqt_inverse_bwd', 'tt_cqt_generic_inverse_bwd', ('daudio', 'dcoeffs')),
    'forward_mag_bwd': ('tt_cqt_forward_mag_bwd', None, ('audio', 'dmag', 'daudio')),
    'griffin_lim': ('tt_cqt_griffin_lim', None, ('mag', 'audio_init', 'audio_out', 'conv')),
}

_worst = {}


def _note(key, ratio, k):
    _worst[key] = max(_worst.get(key, 0.0), ratio)
    print('ratio to bar: %-56s %.4g (worst so far %.4g, K %.4g)' % (key, ratio, _worst[key], k))


def _lib():
    from timbre_trap import _hip
    return _hip.lib(), _hip.stream_ptr()


def _dims(layout):
    p = R.plan(layout)
    return p['n_bins'], p['M'], p['N']


def coeff_shape(layout, B, nb, is_complex):
    F, M, _ = _dims(layout)
    return (B, 1, F, nb * M, 2) if is_complex else (B, 2, F, nb * M)


def audio_shape(layout, B, nb):
    return (B, 1, nb * layout[2])


def arena_for(entry, layout, B, nb, ins, outs, fill, shifts=None, scratch_shift=0):
    """the arena of one call: plan tables, inputs (name -> ndarray), outputs (name -> shape), scratch of exactly the stated size"""
    shifts = shifts or {}
    A = C.Arena(fill, 'cuda')
    R.add_plan(A, layout)
    for name in SPEC[entry][2]:
        if name in ins:
            A.inp(name, torch.from_numpy(np.array(ins[name], dtype=np.float32)), shifts.get(name, 0))
        elif name in outs:
            A.out(name, outs[name], torch.float32, shifts.get(name, 0))
    A.scratch('scratch', R.scratch_carve(layout, B * nb, entry == 'griffin_lim'), scratch_shift, align=256)
    A.build()
    assert A.dev.data_ptr() % 256 == 0 and (A.ptr('scratch').value - scratch_shift) % 256 == 0
    return A


def invoke(entry, layout, A, B, nb, tail, ps=None, null=()):
    """the C call on the arena's windows; operands that were not added, or are named in ``null``, go as NULL"""
    lib, st = _lib()
    fast = layout in R.FAST
    fn = getattr(lib, SPEC[entry][0 if fast else 1])
    if ps is None:
        ps = R.plan_struct(A, layout)
    if not fast and entry != 'griffin_lim':
        assert lib.tt_cqt_generic_scratch_bytes(ctypes.byref(ps), B * nb) in (R.scratch_carve(layout, B * nb), -1, 0)
    ptrs = [None if n in null else A.ptr(n) for n in SPEC[entry][2]]
    return fn(None if 'plan' in null else ctypes.byref(ps), *ptrs, None if 'scratch' in null else A.ptr('scratch'), B, nb, *tail, st)


def call(entry, layout, B, nb, ins, outs, tail, fill=C.FILL_NAN, shifts=None, what=''):
    A = arena_for(entry, layout, B, nb, ins, outs, fill, shifts)
    rc = invoke(entry, layout, A, B, nb, tail)
    assert rc == 0, (what, rc)
    A.verify(what)
    return A


def refused(entry, layout, B, nb, ins, outs, tail, shifts=None, scratch_shift=0, what='', **kw):
    A = arena_for(entry, layout, B, nb, ins, outs, C.FILL_NAN, shifts, scratch_shift)
    assert invoke(entry, layout, A, B, nb, tail, **kw) == BADARG, what
    A.untouched(what)


def transform_io(entry, layout, x, is_complex):
    """(ins, outs, tail) of the four transforms for the input x of cqt_abi_ref.case"""
    B = x.shape[0]
    if entry in ('forward', 'inverse_bwd'):
        nb = x.shape[-1] // layout[2]
        name_in, name_out = SPEC[entry][2]
        return B, nb, {name_in: x}, {name_out: coeff_shape(layout, B, nb, is_complex)}, (int(is_complex),)
    nb = x.shape[-1] // _dims(layout)[1]
    name_in, name_out = SPEC[entry][2]
    ins = {name_in: R.interleaved(x) if is_complex else R.planes(x)}
    return B, nb, ins, {name_out: audio_shape(layout, B, nb)}, ((int(is_complex), 0) if entry == 'inverse' else (int(is_complex),))


def transform_result(entry, A, is_complex):
    got = A.get(SPEC[entry][2][1]).numpy()
    return R.to_complex(got, is_complex) if entry in ('forward', 'inverse_bwd') else got.astype(np.float64)


def run_transform(entry, layout, family, shape, is_complex, fill, shifts=None):
    x, ref, bar = R.case(entry, layout, family, shape)
    B, nb, ins, outs, tail = transform_io(entry, layout, x, is_complex)
    what = '%s %s %s %s complex=%d fill=%02x' % (entry, layout, family, (B, nb), is_complex, fill)
    A = call(entry, layout, B, nb, ins, outs, tail, fill, shifts, what)
    r = R.ratio(entry, transform_result(entry, A, is_complex), ref, bar)
    k = R.K[(entry, family, R.path_of(layout))][0]
    _note('%s %s %s' % (entry, family, R.path_of(layout)), r, k)
    assert r <= k, (what, r, k)
    return A


def _families(entry):
    return R.AUDIO_FAMILIES if entry in ('forward', 'inverse_bwd') else R.COEFF_FAMILIES


def _shapes(layout, family):
    return R.shapes(layout) if family in ('noise', 'analysis', 'random') else (None,)


TRANSFORMS = ('forward', 'inverse', 'forward_bwd', 'inverse_bwd')
CASES = [(e, l, f) for l in tuple(R.FAST) + tuple(R.ANY) for e in TRANSFORMS for f in _families(e)]


@gpu
@pytest.mark.parametrize('entry,layout,family', CASES, ids=lambda v: str(v).replace(' ', ''))
def test_transform_on_layout(entry, layout, family):
    """forward, inverse and the two adjoints on every layout of their path: every batch shape, both layouts of the coefficients, both
    fills (the largest shape under all four combinations)"""
    shapes = _shapes(layout, family)
    for shape in shapes:
        combos = itertools.product((0, 1), FILLS) if shape == shapes[-1] else zip((0, 1), FILLS)
        for is_complex, fill in combos:
            run_transform(entry, layout, family, shape, is_complex, fill)


@gpu
@pytest.mark.parametrize('layout', tuple(R.FAST), ids=str)
def test_magnitude_on_layout(layout):
    """tt_cqt_forward_mag against |encode| on the three audio families, tt_cqt_forward_mag_bwd against magnitude_vjp"""
    for family, fill in zip(R.AUDIO_FAMILIES, itertools.cycle(FILLS)):
        x, ref, bar = R.case('forward', layout, family)
        B, nb = x.shape[0], x.shape[-1] // layout[2]
        F, M, _ = _dims(layout)
        A = call('forward_mag', layout, B, nb, {'audio': x}, {'out': (B, 1, F, nb * M)}, (), fill, None, 'forward_mag %s %s' % (layout, family))
        r = R.coeff_ratio(A.get('out').numpy().astype(np.float64), ref, bar, magnitude=True)
        k = R.K[('forward', family, 'fast')][0]
        _note('forward_mag %s fast' % family, r, k)
        assert r <= k, (layout, family, r, k)
    a, dmag, ref, bar = R.magnitude_case(layout)
    k = R.K[('magnitude_bwd', 'case', 'fast')][0]
    for fill in FILLS:
        A = call('forward_mag_bwd', layout, 2, 2, {'audio': a, 'dmag': dmag}, {'daudio': audio_shape(layout, 2, 2)}, (), fill, None,
                 'forward_mag_bwd %s' % (layout,))
        r = R.audio_ratio(A.get('daudio').numpy(), ref, bar)
        _note('forward_mag_bwd fast', r, k)
        assert r <= k, (layout, r, k)


def _peaks_case(layout):
    """three clips of one block with different peaks: the analysis of noise times 1, 1 / 4 and 3"""
    c = np.array(R.coeffs(layout, 'analysis', (3, 1)))
    return c * np.array([1.0, 0.25, 3.0], dtype=np.float32).reshape(3, 1, 1, 1)


@gpu
@pytest.mark.parametrize('layout', [(9, 61, 66150), (9, 59, 66150), (9, 120, 2205), (4, 9, 1001), (9, 59, 4096)], ids=str)
def test_normalize_is_raw_over_its_peak(layout):
    """normalize = 1 equals raw / peak formed by torch from the kernel's own raw output, bit for bit, with the scratch (the peak word in
    its first bytes) prefilled with NaN bytes and with zeros: a missing reset of the word shows under the first fill"""
    c = _peaks_case(layout)
    ins, outs = {'coeffs': R.interleaved(c)}, {'audio': audio_shape(layout, 3, 1)}
    raw = call('inverse', layout, 3, 1, ins, outs, (1, 0), what='raw').view('audio').clone()
    peaks = raw.abs().amax((1, 2))
    assert float(peaks.max() / peaks.min()) > 4
    want = raw / raw.abs().max()
    for zero in (False, True):
        A = arena_for('inverse', layout, 3, 1, ins, outs, C.FILL_NAN)
        if zero:
            A.view('scratch').zero_()
        assert invoke('inverse', layout, A, 3, 1, (1, 1)) == 0
        A.verify('normalize, scratch %s' % ('zeros' if zero else 'NaN bytes'))
        got = A.view('audio')
        assert torch.equal(got, want), 'scratch %s: %d samples differ from raw / peak' % ('zeros' if zero else 'NaN bytes', int((got != want).sum()))
        assert float(got.abs().max()) == 1.0


@gpu
@pytest.mark.parametrize('layout', [(9, 61, 66150), (5, 12, 2205)], ids=str)
@pytest.mark.parametrize('entry', ['forward', 'inverse'])
def test_scratch_reuse_is_bit_identical(entry, layout):
    """a (3, 2) call and then a (1, 1) call on the same scratch, left as the first call left it: the second call's output equals a
    fresh-arena call bit for bit (fixed summation orders; the inverse runs with normalize = 1, whose peak word the first call set)"""
    give = (lambda shape: R.audio(layout, 'noise', shape)) if entry == 'forward' else (lambda shape: R.coeffs(layout, 'random', shape))
    big, small = give((3, 2)), give((1, 1))
    tail = (1,) if entry == 'forward' else (1, 1)
    B, nb, ins, outs, _ = transform_io(entry, layout, big, True)
    A = arena_for(entry, layout, B, nb, ins, outs, C.FILL_NAN)
    assert invoke(entry, layout, A, B, nb, tail) == 0
    A.verify('first call')
    _, _, ins1, outs1, _ = transform_io(entry, layout, small, True)
    name_in, name_out = SPEC[entry][2]
    # the small operands in the first arena's windows (their leading parts), the scratch untouched in between
    A.view(name_in).reshape(-1)[:ins1[name_in].size] = torch.from_numpy(np.array(ins1[name_in])).reshape(-1).cuda()
    assert invoke(entry, layout, A, 1, 1, tail) == 0
    torch.cuda.synchronize()
    n_out = int(np.prod(outs1[name_out]))
    second = A.view(name_out).reshape(-1)[:n_out].clone()
    fresh = arena_for(entry, layout, 1, 1, ins1, outs1, C.FILL_BIG)
    assert invoke(entry, layout, fresh, 1, 1, tail) == 0
    fresh.verify('fresh call')
    assert torch.equal(second, fresh.view(name_out).reshape(-1))


# ---- Griffin-Lim ---------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('init', [True, False], ids=['audio_init', 'silence'])
@pytest.mark.parametrize('layout', R.GL_LAYOUTS, ids=str)
def test_griffin_lim_on_layout(layout, init):
    """n_iter 1, 2, 3 x momentum 0, 0.99 x conv NULL / given x normalize 0 / 1, from the case's audio and from silence (audio_init
    NULL).  One step at K gl_step x decode_bar of the projected coefficients, later steps at K gl_seq x the block's rms, convergence
    at a relative K gl_conv (the rules of gl_ref); normalize = 1 equals raw / peak of the same call's raw twin bit for bit; the audio
    does not depend on conv being asked for; audio_init is never written (Arena.verify: inputs bit-unchanged)."""
    a, mag = R.gl_inputs(layout)
    B, nb = 2, 2
    ins = {'mag': mag, **({'audio_init': a} if init else {})}
    kconv = R.K[('gl_conv', 'case', 'fast')][0]
    for i, (n_iter, alpha) in enumerate(itertools.product(R.GL_ITERS, R.GL_ALPHAS)):
        ys, conv_ref, bar0 = R.gl_case(layout, init, alpha)
        ref = ys[n_iter - 1]
        raws = []
        for j, with_conv in enumerate((False, True)):
            outs = {'audio_out': audio_shape(layout, B, nb), **({'conv': (n_iter, B)} if with_conv else {})}
            what = 'griffin_lim %s init=%s n_iter=%d momentum=%g conv=%s' % (layout, init, n_iter, alpha, with_conv)
            A = call('griffin_lim', layout, B, nb, ins, outs, (n_iter, alpha, 0), FILLS[(i + j) % 2], None, what)
            raws.append(A.view('audio_out').clone())
            got = A.get('audio_out').numpy()
            if n_iter == 1:
                r, k, key = R.audio_ratio(got, ref, bar0), R.K[('gl_step', 'case', 'fast')][0], 'griffin_lim step'
            else:
                k, key = R.K[('gl_seq%d' % n_iter, 'case', 'fast')][0], 'griffin_lim y_%d / block rms' % (n_iter - 1)
                r = R.gl_ref.block_ratio(got, ref, R.gl_ref.block_rms(ref))
            _note(key, r, k)
            assert r <= k, (what, r, k)
            if with_conv:
                rc = R.gl_ref.conv_ratio(A.get('conv').numpy(), conv_ref[:n_iter])
                _note('griffin_lim convergence', rc, kconv)
                assert rc <= kconv, (what, rc, kconv)
            An = call('griffin_lim', layout, B, nb, ins, outs, (n_iter, alpha, 1), FILLS[(i + j + 1) % 2], None, what + ' normalize')
            assert torch.equal(An.view('audio_out'), raws[-1] / raws[-1].abs().max()), what + ': normalize is not raw / peak'
            if with_conv:
                assert torch.equal(An.view('conv'), A.view('conv'))
        assert torch.equal(raws[0], raws[1]), 'the audio depends on conv being asked for'


# ---- misaligned pointers (the outcomes: module docstring) ------------------------------------------------------------------------------------

def _mis_layouts():
    return ((9, 61, 66150), (4, 9, 1001))


@gpu
@pytest.mark.parametrize('layout', _mis_layouts(), ids=str)
def test_misaligned_transform_pointers(layout):
    """one pointer off by one float: refused before any launch, or served at the same bars -- as read from the code"""
    fast = layout in R.FAST
    for entry in TRANSFORMS:
        family = _families(entry)[0]
        name_in, name_out = SPEC[entry][2]
        for is_complex in (0, 1):
            x, _, _ = R.case(entry, layout, family, (1, 1))
            B, nb, ins, outs, tail = transform_io(entry, layout, x, is_complex)
            coeff_in = entry in ('inverse', 'forward_bwd')
            # the audio side: csrc/cqt.hip moves pairs, csrc/cqt_generic.hip single samples
            # the coefficient side: written as float4 (fast) / read as planes one float at a time (both) / interleaved as float2 (both)
            served_in = (not is_complex) if coeff_in else (not fast)
            served_out = (not fast) if coeff_in else (not fast and not is_complex)
            for name, served in ((name_in, served_in), (name_out, served_out)):
                what = 'misaligned %s of %s %s complex=%d' % (name, entry, layout, is_complex)
                if served:
                    run_transform(entry, layout, family, (1, 1), is_complex, C.FILL_NAN, {name: 4})
                else:
                    refused(entry, layout, B, nb, ins, outs, tail, {name: 4}, what=what)
            refused(entry, layout, B, nb, ins, outs, tail, scratch_shift=16, what='scratch off its boundary, %s %s' % (entry, layout))
            print('%-12s %-18s complex=%d: %s %s, %s %s, scratch + 16 refused' % (
                entry, layout, is_complex, name_in, 'same bars' if served_in else 'refused', name_out, 'same bars' if served_out else 'refused'))


@gpu
def test_misaligned_magnitude_and_griffin_lim_pointers():
    layout = (9, 61, 66150)
    F, M, _ = _dims(layout)
    x = R.case('forward', layout, 'noise', (1, 1))[0]
    ins, outs = {'audio': x}, {'out': (1, 1, F, M)}
    for name in ('audio', 'out'):
        refused('forward_mag', layout, 1, 1, ins, outs, (), {name: 4}, what='misaligned %s of forward_mag' % name)
    refused('forward_mag', layout, 1, 1, ins, outs, (), scratch_shift=16, what='scratch of forward_mag')
    a, dmag, ref, bar = R.magnitude_case(layout)
    ins, outs = {'audio': a, 'dmag': dmag}, {'daudio': audio_shape(layout, 2, 2)}
    for name in ('audio', 'daudio'):
        refused('forward_mag_bwd', layout, 2, 2, ins, outs, (), {name: 4}, what='misaligned %s of forward_mag_bwd' % name)
    refused('forward_mag_bwd', layout, 2, 2, ins, outs, (), scratch_shift=16, what='scratch of forward_mag_bwd')
    A = call('forward_mag_bwd', layout, 2, 2, ins, outs, (), C.FILL_NAN, {'dmag': 4}, 'misaligned dmag')
    r, k = R.audio_ratio(A.get('daudio').numpy(), ref, bar), R.K[('magnitude_bwd', 'case', 'fast')][0]
    _note('forward_mag_bwd fast, dmag off by one float', r, k)
    assert r <= k
    # Griffin-Lim, two steps from the case's audio
    a, mag = R.gl_inputs(layout)
    ys, conv_ref, _ = R.gl_case(layout, True, 0.99)
    ins, outs = {'mag': mag, 'audio_init': a}, {'audio_out': audio_shape(layout, 2, 2), 'conv': (2, 2)}
    for name in ('audio_init', 'audio_out'):
        refused('griffin_lim', layout, 2, 2, ins, outs, (2, 0.99, 0), {name: 4}, what='misaligned %s of griffin_lim' % name)
    refused('griffin_lim', layout, 2, 2, ins, outs, (2, 0.99, 0), scratch_shift=16, what='scratch of griffin_lim')
    k, kc = R.K[('gl_seq2', 'case', 'fast')][0], R.K[('gl_conv', 'case', 'fast')][0]
    for name in ('mag', 'conv'):
        A = call('griffin_lim', layout, 2, 2, ins, outs, (2, 0.99, 0), C.FILL_NAN, {name: 4}, 'misaligned %s of griffin_lim' % name)
        r = R.gl_ref.block_ratio(A.get('audio_out').numpy(), ys[1], R.gl_ref.block_rms(ys[1]))
        rc = R.gl_ref.conv_ratio(A.get('conv').numpy(), conv_ref[:2])
        _note('griffin_lim, %s off by one float' % name, r, k)
        assert r <= k and rc <= kc, (name, r, k, rc, kc)


# ---- refusals: every one before any launch (the whole buffer untouched) -------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('layout', [(9, 59, 66150), (5, 12, 735)], ids=str)
def test_refusals(layout):
    fast = layout in R.FAST
    for entry in TRANSFORMS + (('forward_mag', 'forward_mag_bwd', 'griffin_lim') if fast else ()):
        F, M, _ = _dims(layout)
        if entry in TRANSFORMS:
            x = R.case(entry, layout, _families(entry)[0], (1, 1))[0]
            B, nb, ins, outs, tail = transform_io(entry, layout, x, 0)
        elif entry == 'forward_mag':
            ins, outs, tail = {'audio': R.audio(layout, 'noise', (1, 1))}, {'out': (1, 1, F, M)}, ()
        elif entry == 'forward_mag_bwd':
            ins = {'audio': R.audio(layout, 'noise', (1, 1)), 'dmag': np.ones((1, 1, F, M), dtype=np.float32)}
            outs, tail = {'daudio': audio_shape(layout, 1, 1)}, ()
        else:
            ins = {'mag': np.ones((1, 1, F, M), dtype=np.float32), 'audio_init': R.audio(layout, 'noise', (1, 1))}
            outs, tail = {'audio_out': audio_shape(layout, 1, 1), 'conv': (1, 1)}, (1, 0.5, 0)
        A = arena_for(entry, layout, 1, 1, ins, outs, C.FILL_NAN)

        def no(what, B=1, nb=1, tail=tail, **kw):
            assert invoke(entry, layout, A, B, nb, tail, **kw) == BADARG, '%s %s: %s was not refused' % (entry, layout, what)
            A.untouched('%s %s: %s' % (entry, layout, what))

        optional = ('audio_init', 'conv')
        for name in ('plan', 'scratch') + tuple(n for n in SPEC[entry][2] if n not in optional):
            no('NULL ' + name, null=(name,))
        for B, nb in ((0, 1), (-1, 1), (1, 0), (1, -2)):
            no('B = %d, n_blocks = %d' % (B, nb), B=B, nb=nb)
        if entry == 'griffin_lim':
            no('n_iter = 0', tail=(0, 0.5, 0))
            no('n_iter = -1', tail=(-1, 0.5, 0))
            no('momentum = 1', tail=(1, 1.0, 0))
            no('momentum = -0.1', tail=(1, -0.1, 0))
            no('momentum = NaN', tail=(1, float('nan'), 0))
        if not fast:
            p = R.plan(layout)
            for what, field in (('M not a power of two', dict(M=p['M'] + p['M'] // 2)), ('P not a power of two', dict(P=p['P'] + 1)),
                                ('P < 2 N - 1', dict(P=p['P'] // 2)), ('N < 2', dict(N=1)), ('n_bins = 0', dict(n_bins=0)),
                                ('n_bins < 0', dict(n_bins=-4))):
                no(what, ps=R.plan_struct(A, layout, **field))
            assert p['P'] // 2 < 2 * p['N'] - 1
            for name in R.ANY_TABLES:
                no('NULL table ' + name, ps=R.plan_struct(A, layout, **{name: None}))


# ---- through the wrapper: F, sum_len and the scratch size arrive for layouts other than 540 ----------------------------------------------------

@gpu
@pytest.mark.parametrize('layout', tuple(R.FAST) + ((5, 12, 2205), (9, 59, 4096)), ids=str)
def test_wrapper_equals_the_c_abi(layout):
    from timbre_trap.framework import CQT
    F, M, N = _dims(layout)
    cq = CQT(layout[0], layout[1], R.SR, N / R.SR).to('cuda')
    assert (cq.n_bins, cq.block_length, cq.max_window_length, cq._fast) == (F, N, M, layout in R.FAST)
    a = R.audio(layout, 'noise', (2, 2))
    at = torch.from_numpy(np.array(a)).cuda()
    c = cq.encode(at)
    assert c.shape == (2, 1, F, 2 * M) and c.dtype == torch.complex64
    A = call('forward', layout, 2, 2, {'audio': a}, {'out': coeff_shape(layout, 2, 2, True)}, (1,), what='forward')
    assert torch.equal(torch.view_as_real(c), A.view('out'))
    planes = cq(at)
    assert planes.shape == (2, 2, F, 2 * M)
    assert torch.equal(planes, call('forward', layout, 2, 2, {'audio': a}, {'out': coeff_shape(layout, 2, 2, False)}, (0,)).view('out'))
    y = cq.decode(c)
    assert y.shape == (2, 1, 2 * N)
    ci = np.ascontiguousarray(torch.view_as_real(c).cpu().numpy())
    assert torch.equal(y, call('inverse', layout, 2, 2, {'coeffs': ci}, {'audio': audio_shape(layout, 2, 2)}, (1, 1)).view('audio'))
    mag = cq.magnitude(at)
    assert mag.shape == (2, F, 2 * M)
    g = cq.griffin_lim(mag, n_iter=2)
    assert g.shape == (2, 1, 2 * N) and bool(torch.isfinite(g).all())
    # audio that is a contiguous view starting one float into its allocation (csrc/cqt.hip refuses that address): the wrapper hands
    # over a copy, the results are the same bits
    buf = torch.zeros(at.numel() + 1, device='cuda')
    buf[1:] = at.reshape(-1)
    off = buf[1:].view_as(at)
    assert off.is_contiguous() and off.data_ptr() % 8 == 4
    assert torch.equal(cq.encode(off), c) and torch.equal(cq(off), planes) and torch.equal(cq.magnitude(off), mag)
    assert torch.equal(cq.griffin_lim(mag, n_iter=2, audio_init=off), cq.griffin_lim(mag, n_iter=2, audio_init=at))
    if cq._fast:
        assert torch.equal(mag[:, None], call('forward_mag', layout, 2, 2, {'audio': a}, {'out': (2, 1, F, 2 * M)}, ()).view('out'))
        m = np.ascontiguousarray(mag[:, None].cpu().numpy())
        Ag = call('griffin_lim', layout, 2, 2, {'mag': m}, {'audio_out': audio_shape(layout, 2, 2)}, (2, 0.99, 1))
        assert torch.equal(g, Ag.view('audio_out'))
    else:
        # no magnitude or Griffin-Lim entry point on the any-length path: the wrapper composes them; shapes and the values of |encode|
        assert torch.allclose(mag[:, None], c.abs(), rtol=2.0 ** -21, atol=0.0)
