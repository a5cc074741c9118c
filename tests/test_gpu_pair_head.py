"""
The pair forms of the decoder's latent head (include/ttrap.h: tt_latent16_expand_reps / _contract_reps / _wgrad_reps, tt_latent16_image_bytes)
through the C ABI -- what TimbreTrap.decode_pair runs instead of concatenating two copies of the latents.

Two claims per case:

  values    against the float64 restatement of tests/cl16_ref.py (lat_z, lat_expand, lat_contract, lat_wgrad), at the bars
            tests/test_gpu_cl16_parity.py holds the one-batch entry points to: K U S of a sum of K fp32 products (S = the sum of their
            absolute values, U = 2^-24) and, for a stored 16-bit value, C.bar16 on top.  The two halves of the summed latent gradient
            are two such sums and one fp32 add: K U (S0 + S1) + U |v0 + v1|.
  bits      against the route the pair form replaces: the one-batch entry points on the CONCATENATED batch of 2 B clips (each half with
            its indicator as a materialised channel), the two halves of the latent gradient added in fp32 afterwards.  Outputs, latent
            gradient, dW and db are equal bit for bit: the pair form changes where the operands are read, not one product or the order
            of a sum.  (One exception, stated where it is made: db of the gated form, whose reduce ends in atomics.)

Shapes, the smallest at which each part can go wrong: B = 1 and 2; T = 64 (one group of frames; with B = 1 the two halves are exactly
one 64-pixel chunk of the weight gradient each), 80 (a partial group; a chunk of the weight gradient spans the two halves) and 320 (several
workgroups of the expansion and the contraction); both instantiations (CT = 32 with D = 33, the model_complexity 1 head, and CT = 64
with D = 129, the model_complexity 2 head of the benchmark); both element types; the indicator pairs (1, 0) and (0, 1); the gated (gy)
and the pregated backward.  Every case ends with a plain reps = 1 call on OTHER latents into the same image buffer, against the one-batch
entry points: an image left over from the pair call would show.
"""

import functools
import zlib

import pytest
import torch

import cl16_ref as C

pytestmark = pytest.mark.gpu

U = C.U
BF16, FP16, F32 = torch.bfloat16, torch.float16, torch.float32
E = 5


def _tag(dtype):
    return 'bf16' if dtype == BF16 else 'fp16'


def _api(dtype):
    from timbre_trap import _hip
    from timbre_trap.framework import ops
    return ops.lib16(dtype), _hip.stream_ptr()


def _gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


def _hold(key, got, want, bar, what):
    e = (got.double() - want).abs()
    r = (e / bar.clamp_min(1e-300)).reshape(-1)
    print('ratio to bar: %-40s %.3f' % (key, float(r.max())))
    assert bool((e <= bar).all()), '%s %s: %.3f of the bar (%d of %d elements over)' % (key, what, float(r.max()), int((e > bar).sum()), e.numel())


def _same(key, a, b, what):
    """bit for bit (compared as integers: -0 and +0 differ, NaN patterns count)"""
    ia, ib = a.contiguous().view(torch.int16 if a.element_size() == 2 else torch.int32), b.contiguous().view(torch.int16 if b.element_size() == 2 else torch.int32)
    n = int((ia != ib).sum())
    assert n == 0, '%s %s: %d of %d elements differ from the concatenated-batch route' % (key, what, n, ia.numel())


@functools.lru_cache(maxsize=4)
def _setup(dtype, CT, D, T, B):
    gen = _gen('pair', CT, D, T, B)
    return dict(z=C.pm32(gen, B, D - 1, T), z1=C.pm32(gen, B, D - 1, T), g=C.pm16(gen, dtype, 2 * B, E, T, CT), gy=C.pm16(gen, dtype, 2 * B, E, T, CT),
                we=C.exact_weights(gen, D, D, CT, E), bc=C.pm32(gen, CT), dw=C.pm32(gen, D, CT, E), db=C.pm32(gen, CT))


def _cat(z, ind):
    """the batch the old route decodes: each half with its indicator as a channel"""
    return torch.cat([torch.cat((z, torch.full_like(z[:, :1], v)), 1) for v in ind], 0)


def _expand_want(zc, D, s, dtype):
    v, S, K = C.lat_expand(C.lat_z(zc, D, D, 0.0, dtype), s['we'])
    bc = s['bc'].double().view(1, -1, 1, 1)
    a = v + bc
    return C.elu(a), K * U * S + 3 * U * bc.abs() + 4 * U * a.abs().clamp_min(1.0)


def _run(dtype, CT, D, T, B, ind, gated, fill):
    lib, st = _api(dtype)
    s = _setup(dtype, CT, D, T, B)
    Dz = D - 1
    zc = _cat(s['z'], ind)                                       # (2B, D, T)
    what = 'pair head %s CT %d D %d T %d B %d ind %s %s' % (_tag(dtype), CT, D, T, B, ind, 'gy' if gated else 'pregated')
    A = C.Arena(fill, 'cuda')
    A.inp('z', s['z']); A.inp('zc', zc); A.inp('z1', s['z1'])
    A.inp('w', s['we']); A.inp('bias', s['bc']); A.inp('g', s['g'])
    if gated:
        A.inp('gy', s['gy'])
    for k in ('new', 'old'):
        A.out('y_' + k, (2 * B, E, T, CT), dtype)
        A.acc('dw_' + k, s['dw']); A.acc('db_' + k, s['db'])
        A.out('y1_' + k, (B, E, T, CT), dtype)
        A.acc('dw1_' + k, s['dw']); A.acc('db1_' + k, s['db'])
    A.out('dz_new', (B, Dz, T), F32); A.out('dz_old', (2 * B, Dz, T), F32)
    A.scratch('zt', lib.tt_latent16_image_bytes(B, CT, D, T))
    A.scratch('ws', lib.tt_latent16_scratch_bytes(2 * B, CT, D, E, T))
    A.build()
    P = A.ptr
    gy = P('gy')                                                 # NULL: the pregated forms
    # --- the pair forms
    assert lib.tt_latent16_expand_reps(P('z'), Dz, ind[0], ind[1], 2, P('w'), P('bias'), P('y_new'), P('zt'), P('ws'), B, CT, D, E, T, st) == 0
    assert lib.tt_latent16_contract_reps(P('g'), gy, P('w'), P('dz_new'), P('ws'), B, CT, D, Dz, E, T, 2, st) == 0
    assert lib.tt_latent16_wgrad_reps(P('zt'), Dz, ind[0], ind[1], 2, P('g'), gy, P('dw_new'), P('db_new'), P('ws'), B, CT, D, E, T, st) == 0
    # --- the route they replace: one batch of 2 B clips with the indicator as a channel
    assert lib.tt_latent16_expand(P('zc'), D, 0.0, P('w'), P('bias'), P('y_old'), P('ws'), 2 * B, CT, D, E, T, st) == 0
    if gated:
        assert lib.tt_latent16_contract(P('g'), gy, P('w'), None, P('dz_old'), P('ws'), 2 * B, CT, D, Dz, E, T, st) == 0
        assert lib.tt_latent16_wgrad(P('zc'), D, 0.0, P('g'), gy, P('dw_old'), P('db_old'), P('ws'), 2 * B, CT, D, E, T, st) == 0
    else:
        assert lib.tt_latent16_contract_pregated(P('g'), P('w'), P('dz_old'), P('ws'), 2 * B, CT, D, Dz, E, T, st) == 0
        assert lib.tt_latent16_wgrad_pregated(P('zc'), D, 0.0, P('g'), P('dw_old'), P('db_old'), P('ws'), 2 * B, CT, D, E, T, st) == 0
    # --- a plain call afterwards, other latents, the same image buffer
    assert lib.tt_latent16_expand_reps(P('z1'), Dz, 0.75, 0.0, 1, P('w'), P('bias'), P('y1_new'), P('zt'), P('ws'), B, CT, D, E, T, st) == 0
    assert lib.tt_latent16_wgrad_reps(P('zt'), Dz, 0.75, 0.0, 1, P('g'), gy, P('dw1_new'), P('db1_new'), P('ws'), B, CT, D, E, T, st) == 0
    assert lib.tt_latent16_expand(P('z1'), Dz, 0.75, P('w'), P('bias'), P('y1_old'), P('ws'), B, CT, D, E, T, st) == 0
    if gated:
        assert lib.tt_latent16_wgrad(P('z1'), Dz, 0.75, P('g'), gy, P('dw1_old'), P('db1_old'), P('ws'), B, CT, D, E, T, st) == 0
    else:
        assert lib.tt_latent16_wgrad_pregated(P('z1'), Dz, 0.75, P('g'), P('dw1_old'), P('db1_old'), P('ws'), B, CT, D, E, T, st) == 0
    A.verify(what)

    # --- bits.  (db of the GATED form is left to the bar below: k_lat_wred adds its sixteen slice sums of a channel to db with atomicAdd, in
    # arrival order, so two runs of the SAME call differ in the last bit there -- before this form existed as well.  The pregated form,
    # which the default train step takes, sums in a fixed order: k_lat_dbrows.)
    for k in ('y', 'dw', 'y1', 'dw1') + (() if gated else ('db', 'db1')):
        _same(k, A.get(k + '_new'), A.get(k + '_old'), what)
    dz_old = A.get('dz_old')
    _same('dz', A.get('dz_new'), dz_old[:B] + dz_old[B:], what)

    # --- values
    tag = _tag(dtype)
    want, beta = _expand_want(zc, D, s, dtype)
    got = C.from_cl(A.get('y_new'))
    _hold('pair expand ' + tag, got, want, C.bar16(want, beta, dtype), what)
    g = C.from_cl(s['g'])
    gsum = g
    if gated:
        gsum = g * C.elu_gate(C.from_cl(s['gy']))
        g = C.round16(gsum, dtype)
    (v0, S0, K), (v1, S1, _) = C.lat_contract(g[:B], s['we'], Dz), C.lat_contract(g[B:], s['we'], Dz)
    _hold('pair contract ' + tag, A.get('dz_new'), v0 + v1, K * U * (S0 + S1) + U * (v0 + v1).abs(), what)
    zq = C.lat_z(zc, D, D, 0.0, dtype)
    dw, S, K, _, _, _ = C.lat_wgrad(zq, g)
    _, _, _, db, Sb, Kb = C.lat_wgrad(zq, gsum)
    pw, pb = s['dw'].double(), s['db'].double()
    _hold('pair wgrad dw ' + tag, A.get('dw_new'), pw + dw, K * U * S + 3 * U * pw.abs(), what)
    _hold('pair wgrad db ' + tag, A.get('db_new'), pb + db, Kb * U * Sb + 3 * U * pb.abs(), what)
    # the plain call: its forward and its weight gradient (the first B clips of g)
    z1c = torch.cat((s['z1'], torch.full_like(s['z1'][:, :1], 0.75)), 1)
    want, beta = _expand_want(z1c, D, s, dtype)
    _hold('plain expand after pair ' + tag, C.from_cl(A.get('y1_new')), want, C.bar16(want, beta, dtype), what)
    dw, S, K, _, _, _ = C.lat_wgrad(C.lat_z(z1c, D, D, 0.0, dtype), g[:B])
    _hold('plain wgrad after pair ' + tag, A.get('dw1_new'), pw + dw, K * U * S + 3 * U * pw.abs(), what)


@pytest.mark.parametrize('T', [64, 80, 320])
@pytest.mark.parametrize('B', [1, 2])
@pytest.mark.parametrize('CT,D', [(32, 33), (64, 129)], ids=['mc1', 'mc2'])
@pytest.mark.parametrize('dtype', [BF16, FP16], ids=_tag)
def test_pair_head(dtype, CT, D, B, T):
    first = True
    for ind in ((1.0, 0.0), (0.0, 1.0)):
        for gated in (False, True):
            _run(dtype, CT, D, T, B, ind, gated, C.FILL_NAN if first else C.FILL_BIG)
            first = False


@pytest.mark.parametrize('dtype', [BF16, FP16], ids=_tag)
def test_pair_head_refusals(dtype, CT=32, D=33, B=1, T=64):
    """reps other than 1 or 2, a missing image, a misaligned image and a head without a free row for the pregated bias gradient are
    refused with nothing written."""
    lib, st = _api(dtype)
    s = _setup(dtype, CT, D, T, B)
    A = C.Arena(C.FILL_NAN, 'cuda')
    A.inp('z', s['z']); A.inp('w', s['we']); A.inp('bias', s['bc']); A.inp('g', s['g'])
    A.out('y', (2 * B, E, T, CT), dtype); A.out('dz', (B, D - 1, T), F32)
    A.acc('dw', s['dw']); A.acc('db', s['db'])
    A.scratch('zt', lib.tt_latent16_image_bytes(B, CT, D, T) + 16)
    A.scratch('ws', lib.tt_latent16_scratch_bytes(2 * B, CT, D, E, T))
    A.build()
    P = A.ptr
    BADARG, UNSUPPORTED = -1, -2
    assert lib.tt_latent16_expand_reps(P('z'), D - 1, 1.0, 0.0, 3, P('w'), P('bias'), P('y'), P('zt'), P('ws'), B, CT, D, E, T, st) == BADARG
    assert lib.tt_latent16_expand_reps(P('z'), D - 1, 1.0, 0.0, 2, P('w'), P('bias'), P('y'), None, P('ws'), B, CT, D, E, T, st) == BADARG
    assert lib.tt_latent16_expand_reps(P('z'), D - 1, 1.0, 0.0, 2, P('w'), P('bias'), P('y'), P('zt', 2), P('ws'), B, CT, D, E, T, st) == BADARG
    assert lib.tt_latent16_expand_reps(P('z'), D - 1, 1.0, 0.0, 2, P('w'), None, P('y'), P('zt'), P('ws'), B, CT, D, E, T, st) == BADARG
    assert lib.tt_latent16_contract_reps(P('g'), None, P('w'), P('dz'), P('ws'), B, CT, D, D - 1, E, T, 0, st) == BADARG
    assert lib.tt_latent16_wgrad_reps(P('zt', 2), D - 1, 1.0, 0.0, 2, P('g'), None, P('dw'), P('db'), P('ws'), B, CT, D, E, T, st) == BADARG
    assert lib.tt_latent16_wgrad_reps(P('zt'), D - 1, 1.0, 0.0, 2, P('g'), None, P('dw'), None, P('ws'), B, CT, D, E, T, st) == BADARG
    # D = 48 fills the three row tiles: no free row for the bias gradient of the pregated forms (tt_latent16_pregated_ok)
    assert lib.tt_latent16_pregated_ok(CT, 48) == 0
    assert lib.tt_latent16_contract_reps(P('g'), None, P('w'), P('dz'), P('ws'), B, CT, 48, 33, E, T, 2, st) == UNSUPPORTED
    assert lib.tt_latent16_wgrad_reps(P('zt'), 47, 1.0, 0.0, 2, P('g'), None, P('dw'), P('db'), P('ws'), B, CT, 48, E, T, st) == UNSUPPORTED
    assert lib.tt_latent16_image_bytes(B, 48, 8, T) == -1
    A.untouched('refused pair-head calls')


@pytest.mark.parametrize('pregated', [False, True], ids=['gy', 'pregated'])
@pytest.mark.parametrize('dtype', [BF16, FP16], ids=_tag)
def test_latdec16_pair_is_the_concatenated_decode(dtype, pregated, B=2, CT=64, D=129, T=80):
    """ops.LatDec16Fn with ``pair`` against itself on the concatenated batch the pair decode used to build (each half with its indicator as a
    channel of the latents): output, latent gradient -- there the sum autograd forms of the halves' slices -- and dW bit for bit; db as
    well on the pregated route (fixed order), to fp32 rounding on the gated one (its reduce ends in atomics)."""
    from timbre_trap.framework import ops
    s = _setup(dtype, CT, D, T, B)
    w0, b0 = s['we'].view(D, CT, E, 1).cuda(), s['bc'].cuda()
    dy = ops._pack(C.from_cl(s['g']).float().cuda().contiguous(), dtype)
    res = []
    for pair in (True, False):
        z = s['z'].cuda().requires_grad_(True)
        w, b = w0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        link = ops.GateLink() if pregated else None
        with torch.autocast('cuda', dtype=dtype):                # the element type the forward creates its output in (ops.cl16_dtype)
            if pair:
                y = ops.LatDec16Fn.apply(z, w, b, None, link, (1.0, 0.0))
            else:
                ones = torch.ones_like(z[:, :1])
                y = ops.LatDec16Fn.apply(torch.cat((torch.cat((z, ones), 1), torch.cat((z, torch.zeros_like(ones)), 1)), 0), w, b, None, link)
        assert tuple(y.shape) == (2 * B, CT, E, T) and y.dtype == dtype
        if pregated:
            assert link.producer
            link.gated = True
        y.backward(dy)
        res.append((y.detach().float(), z.grad, w.grad, b.grad))
    (y1, dz1, dw1, db1), (y0, dz0, dw0, db0) = res
    assert torch.equal(y1, y0) and torch.equal(dz1, dz0) and torch.equal(dw1, dw0)
    if pregated:
        assert torch.equal(db1, db0)
    else:
        assert float((db1 - db0).abs().max()) <= 64 * U * float(db0.abs().max())
