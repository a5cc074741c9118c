"""
The yardstick of tests/test_gpu_cl16_parity.py, checked where no GPU is needed: the float64 restatements of tests/cl16_ref.py against
torch in float64 (F.conv2d, F.conv_transpose2d, torch.nn.grad.conv2d_weight, autograd) at the geometries the GPU file runs, and the
guarded arena itself -- a torch write stands in for a kernel, so the proof that the arena sees a write into a guard band, a changed
input and an output that was not written needs no deliberately wrong kernel.  Agreement of the restatements: 1e-12 of the sum of absolute
products S.

It also pins the rounding term of a stored 16-bit result.  Round-to-nearest to p significant bits moves v by up to 2^-p |v| (p = 8 for
bf16, 11 for fp16): test_rounding_term shows that torch's own correctly rounded conversion of values in [1, 2) reaches 0.99 of that and
therefore exceeds half of it (2^-9 / 2^-12), which no conversion instruction can meet.
"""

import pytest
import torch
import torch.nn.functional as F

import cl16_ref as C

TOL = 1e-12
DTYPES = [torch.bfloat16, torch.float16]
EDGE_PLANES = [(1, 1), (1, 4), (2, 3), (3, 4), (16, 64), (17, 65), (17, 68)]


def _close(got, want, scale, what):
    e = (got - want).abs()
    assert bool((e <= TOL * scale).all()), '%s: off by %.3e where the scale is %.3e' % (what, float(e.max()), float(scale.max()))


# ---- restatements against torch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,T', EDGE_PLANES)
@pytest.mark.parametrize('Cin,Cout', [(2, 4), (1, 4), (4, 2), (4, 1)])
def test_edge_convolutions_against_torch(Cin, Cout, H, T, B=2):
    gen = torch.Generator().manual_seed(Cin * 1000 + Cout * 100 + H + T)
    x = torch.randn(B, Cin, H, T, generator=gen, dtype=torch.float64, requires_grad=True)
    w = torch.randn(Cout, Cin, 3, 3, generator=gen, dtype=torch.float64, requires_grad=True)
    b = torch.randn(Cout, generator=gen, dtype=torch.float64, requires_grad=True)
    v_t = F.conv2d(x, w, b, padding=1)
    for act, fn in ((C.ACT_NONE, lambda v: v), (C.ACT_ELU, F.elu), (C.ACT_RELU, torch.relu), (C.ACT_SIGMOID, torch.sigmoid)):
        y, v, S, K = C.edge_fwd(x.detach(), w.detach(), b.detach(), act)
        _close(v, v_t.detach(), S + b.detach().abs().view(1, -1, 1, 1), 'pre-activation')
        _close(y, fn(v_t.detach()), S + b.detach().abs().view(1, -1, 1, 1) + 1.0, 'act %d' % act)
    assert K.shape == (H, T) and int(K.max()) <= 9 * Cin and int(K.min()) >= Cin * min(H, 2) * min(T, 2)
    g = torch.randn(B, Cout, H, T, generator=gen, dtype=torch.float64)
    dx_t, dw_t, db_t = torch.autograd.grad(v_t, (x, w, b), g)
    r = C.edge_bwd(x.detach(), g, w.detach())
    _close(r['dw'][0], dw_t, r['dw'][1], 'weight gradient')
    _close(r['dw'][0], torch.nn.grad.conv2d_weight(x.detach(), w.shape, g, padding=1), r['dw'][1], 'weight gradient (conv2d_weight)')
    _close(r['db'][0], db_t, r['db'][1], 'bias gradient')
    _close(r['dx'][0], dx_t, r['dx'][1], 'data gradient')
    _close(r['dx'][0], F.conv_transpose2d(g, w.detach(), padding=1), r['dx'][1], 'data gradient (conv_transpose2d)')
    assert r['dw'][2].shape == (3, 3) and int(r['dw'][2][1, 1]) == B * H * T and r['db'][2] == B * H * T
    # a bar on g carried through the three sums is what the sums give for |x|, |w| and that bar
    bw, bb, bx = C.edge_carry(x.detach().abs(), g.abs(), w.detach().abs())
    _close(bw, r['dw'][1], r['dw'][1], 'carried dw')
    _close(bb, r['db'][1], r['db'][1], 'carried db')
    _close(bx, r['dx'][1], r['dx'][1], 'carried dx')


def test_activation_gradients_through_the_output():
    gen = torch.Generator().manual_seed(3)
    a = torch.randn(1000, generator=gen, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(1000, generator=gen, dtype=torch.float64)
    for act, fn in ((C.ACT_RELU, torch.relu), (C.ACT_SIGMOID, torch.sigmoid)):
        y = fn(a)
        want, = torch.autograd.grad(y, a, dy)
        got, _ = C.act_grad(dy, y.detach(), act)
        _close(got, want, dy.abs() + 1e-300, 'act %d' % act)
    y = F.elu(a)
    want, = torch.autograd.grad(y, a, dy)
    _close(dy * C.elu_gate(y.detach()), want, dy.abs(), 'ELU gate')
    _close(C.elu(a.detach()), y.detach(), a.detach().abs() + 1, 'ELU')


LATENT_CASES = [(32, 1, 1, 16, 1), (32, 15, 2, 16, 2), (32, 17, 31, 16, 1), (32, 48, 2, 80, 2), (64, 1, 2, 16, 1), (64, 143, 1, 80, 1),
                (64, 144, 2, 16, 2)]


@pytest.mark.parametrize('CT,D,E,T,B', LATENT_CASES)
def test_latent_heads_against_torch(CT, D, E, T, B):
    """Encoder.convlat = Conv2d(CT, D, (E, 1)) on (B, CT, E, T); Decoder.convin = ConvTranspose2d(D, CT, (E, 1)) on (B, D, 1, T): both weights
    are (D, CT, E, 1) arrays, the restatement's (D, CT, E)."""
    gen = torch.Generator().manual_seed(CT * 1000 + D * 10 + E)
    w = torch.randn(D, CT, E, generator=gen, dtype=torch.float64)
    x = torch.randn(B, CT, E, T, generator=gen, dtype=torch.float64)
    z = torch.randn(B, D, T, generator=gen, dtype=torch.float64)
    for Dout in {D, max(D - 1, 1)}:
        v, S, K = C.lat_contract(x, w, Dout)
        _close(v, F.conv2d(x, w.unsqueeze(3))[:, :Dout, 0], S, 'contract')
        assert K == CT * E and v.shape == (B, Dout, T)
    v, S, K = C.lat_expand(z, w)
    _close(v, F.conv_transpose2d(z.unsqueeze(2), w.unsqueeze(3)), S, 'expand')
    assert K == D and v.shape == (B, CT, E, T)
    dw, Sw, Kw, db, Sb, Kb = C.lat_wgrad(z, x)
    # convlat: x the input, z the gradient of the latents; convin: z the input, x the gradient of the output -- the same sum
    _close(dw, torch.nn.grad.conv2d_weight(x, (D, CT, E, 1), z.unsqueeze(2))[..., 0], Sw, 'weight gradient')
    _close(db, x.sum((0, 2, 3)), Sb, 'bias gradient')
    assert Kw == B * T and Kb == B * E * T
    # the constant last channel
    zc = C.lat_z(z[:, :D - 1].float(), D - 1, D, 0.75, torch.float16) if D > 1 else None
    if zc is not None:
        assert zc.shape == (B, D, T) and bool((zc[:, D - 1] == 0.75).all())
        assert torch.equal(zc[:, :D - 1], z[:, :D - 1].float().half().double())


STRIDED = [('sconv', 4, 2, 0), ('sconv', 5, 4, 0), ('sconv', 6, 5, 0), ('sconv', 7, 3, 0), ('sconv', 13, 6, 0), ('tconv', 1, 2, 0),
           ('tconv', 1, 2, 1), ('tconv', 2, 4, 1), ('tconv', 3, 5, 0), ('tconv', 9, 6, 1)]


@pytest.mark.parametrize('kind,H,T,out_pad', STRIDED)
def test_strided_pair_against_torch(kind, H, T, out_pad, Cn=4, B=2):
    gen = torch.Generator().manual_seed(H * 100 + T + out_pad)
    Cin = Cn if kind == 'sconv' else 2 * Cn
    x = torch.randn(B, Cin, H, T, generator=gen, dtype=torch.float64, requires_grad=True)
    w = torch.randn(2 * Cn, Cn, 4, 1, generator=gen, dtype=torch.float64, requires_grad=True)
    b = torch.randn(2 * Cn if kind == 'sconv' else Cn, generator=gen, dtype=torch.float64, requires_grad=True)
    if kind == 'sconv':
        v_t = F.conv2d(x, w, b, stride=(2, 1))
    else:
        v_t = F.conv_transpose2d(x, w, b, stride=(2, 1), output_padding=(out_pad, 0))
    y, v, S, K = C.stride_fwd(kind, Cn, x.detach(), w.detach(), b.detach(), out_pad)
    _close(v, v_t.detach(), S + b.detach().abs().view(1, -1, 1, 1), 'pre-activation')
    _close(y, F.elu(v_t.detach()), S + b.detach().abs().view(1, -1, 1, 1) + 1, 'ELU')
    assert K.shape == v.shape[2:] and int(K.max()) <= 4 * Cin
    g = torch.randn(v_t.shape, generator=gen, dtype=torch.float64)
    dx_t, dw_t, db_t = torch.autograd.grad(v_t, (x, w, b), g)
    r = C.stride_bwd(kind, Cn, x.detach(), g, w.detach())
    _close(r['dw'][0], dw_t, r['dw'][1], 'weight gradient')
    _close(r['db'][0], db_t, r['db'][1], 'bias gradient')
    _close(r['dx'][0], dx_t, r['dx'][1], 'data gradient')
    assert r['dw'][2].shape == (1, 1, 4, 1) and r['dx'][2].shape == (H, T)
    if kind == 'sconv' and H % 2 == 1:
        assert bool((r['dx'][0][:, :, -1] == 0).all())
    assert torch.equal(C.stride_bwd(kind, Cn, x.detach(), g, w.detach(), gsum=2 * g)['db'][0], 2 * r['db'][0])


@pytest.mark.parametrize('d', [1, 2, 3])
@pytest.mark.parametrize('H,T', [(1, 2), (3, 6), (9, 7)])
def test_residual_block_forward_against_torch(H, T, d, Cn=4, B=2):
    gen = torch.Generator().manual_seed(H * 10 + T + d)
    x = torch.randn(B, Cn, H, T, generator=gen, dtype=torch.float64)
    w1 = torch.randn(Cn, Cn, 3, 3, generator=gen, dtype=torch.float64)
    w2 = torch.randn(Cn, Cn, generator=gen, dtype=torch.float64)
    b1, b2 = torch.randn(Cn, generator=gen, dtype=torch.float64), torch.randn(Cn, generator=gen, dtype=torch.float64)
    h, a1, S1, K1 = C.rb_stage1(x, w1, b1, d)
    a1_t = F.conv2d(x, w1, b1, padding=d, dilation=d)
    _close(a1, a1_t, S1 + b1.abs().view(1, -1, 1, 1), 'conv1')
    _close(h, F.elu(a1_t), S1 + 1, 'h1')
    assert K1.shape == (H, T) and int(K1.max()) <= 9 * Cn and int(K1.min()) >= Cn
    e, a2, S2 = C.rb_stage2(h, w2, b2)
    a2_t = F.conv2d(F.elu(a1_t), w2.view(Cn, Cn, 1, 1), b2)
    _close(a2, a2_t, S2 + b2.abs().view(1, -1, 1, 1), 'conv2')
    _close(e + x, F.elu(a2_t) + x, S2 + x.abs() + 1, 'y')


@pytest.mark.parametrize('dtype', DTYPES)
def test_spacing_and_boundary_marks(dtype):
    gen = torch.Generator().manual_seed(13)
    v = ((torch.rand(20000, generator=gen) - 0.5) * 8).double()
    r = C.round16(v, dtype)
    # the spacing: the next representable value above |r| is one ulp16 away
    up = torch.nextafter(r.abs().to(dtype), torch.tensor(float('inf'), dtype=dtype)).double()
    assert torch.equal(up - r.abs(), C.ulp16(r, dtype))
    assert float(C.ulp16(torch.tensor(1e-9, dtype=torch.float64), torch.float16)) == 2.0 ** -24
    # the spread: any value within beta of v rounds to round16(v) where it is 0, and to within the spread of round16(v) elsewhere; it is
    # one spacing wherever beta is below the spacing
    beta = 1e-6 * (1 + v.abs())
    spread = C.boundary_spread(v, beta, dtype)
    assert bool((spread >= 0).all())
    for k in (-1.0, -0.5, 0.5, 1.0):
        rs = C.round16(v + k * beta, dtype)
        assert torch.equal(rs[spread == 0], r[spread == 0])
        assert bool(((rs - r).abs() <= spread).all())
    fine = (spread > 0) & (2 * beta < C.ulp16(r, dtype) / 2)
    assert bool((spread[fine] <= C.ulp16(r, dtype)[fine]).all()) and int(fine.sum()) > 0
    assert int((spread > 0).sum()) < v.numel() // 20


def test_pointwise_helpers():
    gen = torch.Generator().manual_seed(5)
    n = 8 * 37
    for dtype in DTYPES:
        g = C.pm16(gen, dtype, 2, n).double()
        e = C.pm16(gen, dtype, n).double()
        prev = C.pm16(gen, dtype, n).double()
        s = -0.8125
        v, S, K = C.skip_join_fwd(g, e, s, 2)
        assert torch.equal(v, g + s * e) and bool((S >= v.abs()).all()) and K == 1
        for gate in range(4):
            de, bar, ds, Sd, Kd = C.skip_join_bwd(g, e, s, gate, prev)
            t = g[0] + g[1]
            want = s * t * (torch.where(e > 0, torch.ones_like(e), e + 1) if gate & 1 else 1.0) + (prev if gate & 2 else 0.0)
            _close(de, want, want.abs() + 1, 'de, gate %d' % gate)
            _close(ds, (t * e).sum(), Sd, 'ds')
            assert Kd == n and bool((bar >= de.abs() - 1e-12).all())
        v, S, K = C.gate16(g[0], e)
        assert torch.equal(v, torch.where(e > 0, g[0], g[0] * (e + 1)))
        # the gate of two 16-bit values in +-[0.5, 1] is exact in fp32: its 16-bit rounding is known exactly
        assert torch.equal(v.float().double(), v)
        v, S, K = C.scaled_add(g[0], g[1], s)
        assert torch.equal(v, g[0] + s * g[1])
        assert torch.equal(C.scaled_add(None, g[1], s)[0], s * g[1])
        v, S, K = C.dot(g[0], g[1])
        assert K == n and abs(float(v - (g[0] * g[1]).sum())) <= TOL * float(S)


@pytest.mark.parametrize('dtype', DTYPES)
def test_operands(dtype):
    gen = torch.Generator().manual_seed(7)
    x = C.pm16(gen, dtype, 4096)
    assert x.dtype == dtype and bool((x.float().abs() >= 0.5).all()) and bool((x.float().abs() <= 1).all())
    assert 0.3 < float((x.float() > 0).float().mean()) < 0.7
    for K in (9, 18, 36, 31 * 32, 144):
        w = C.exact_weights(gen, K, 4096)
        assert torch.equal(w.to(dtype).float(), w), 'weights are exact in the element type'
        scaled = w.abs() * 2.0 ** -round(torch.log2(torch.tensor(K ** -0.5)).item())
        assert bool((scaled >= 0.5).all()) and bool((scaled < 1).all())
        assert torch.equal((w.double() * x.double()).float().double(), w.double() * x.double()), 'a product is exact in fp32'
    t = C.pm16(gen, dtype, 2, 3, 5, 7)
    assert torch.equal(C.from_cl(C.to_cl(t.double(), dtype)), t.double())
    assert C.to_cl(t.double(), dtype).shape == (2, 5, 7, 3)


@pytest.mark.parametrize('dtype', DTYPES)
def test_rounding_term(dtype):
    """A correctly rounded store stays within the unit roundoff 2^-p |v| and does NOT stay within half of it."""
    gen = torch.Generator().manual_seed(11)
    v = (1 + torch.rand(100000, generator=gen)).double()                  # [1, 2): the binade's low end is where the relative error peaks
    r = C.round16(v, dtype)
    rel = ((r - v).abs() / v.abs()).max().item()
    e = C.roundoff16(dtype)
    assert rel <= e
    assert rel > 0.9 * e > e / 2
    assert bool(((r - v).abs() <= C.bar16(v, torch.zeros_like(v), dtype)).all())
    # below the smallest normal number the spacing stops shrinking: the relative term alone is missed, half the spacing holds
    tiny = (torch.rand(100000, generator=gen).double() - 0.5) * 2.0 ** (-13 if dtype == torch.float16 else -125)
    rt = C.round16(tiny, dtype)
    assert bool(((rt - tiny).abs() <= C.bar16(tiny, torch.zeros_like(tiny), dtype)).all())
    assert float((rt - tiny).abs().max()) > 0.9 * C.half_spacing16(dtype)
    assert not bool(((rt - tiny).abs() <= e * tiny.abs()).all())
    # the fill patterns read as the issue says
    for fill, check in ((C.FILL_NAN, torch.isnan), (C.FILL_BIG, lambda t: torch.isfinite(t) & (t > 6))):
        raw = torch.full((8,), fill, dtype=torch.uint8)
        for ty in (torch.bfloat16, torch.float16, torch.float32):
            assert bool(check(raw.view(ty).float()).all())


# ---- the arena --------------------------------------------------------------------------------------------------------------------
def _arena(fill, shift=0):
    gen = torch.Generator().manual_seed(1)
    A = C.Arena(fill)
    A.inp('x', C.pm16(gen, torch.bfloat16, 2, 3, 5, 4), shift)
    A.inp('w', C.pm32(gen, 4, 2, 3, 3))
    A.out('y', (2, 3, 5, 4), torch.float16)
    A.out('z', (7,), torch.float32, 4)
    A.acc('dw', C.pm32(gen, 9))
    A.scratch('ws', 100)
    return A.build()


def _kernel(A):
    """What a correct call leaves: outputs written, accumulators added to, scratch used."""
    A.view('y').copy_(torch.ones(2, 3, 5, 4).half())
    A.view('z').fill_(2.0)
    A.view('dw').add_(1.0)
    A.view('ws').fill_(7)


@pytest.mark.parametrize('fill', [C.FILL_NAN, C.FILL_BIG])
def test_arena_layout_and_a_clean_call(fill):
    A = _arena(fill, shift=8)
    ends = 0
    for name, w in A.win.items():
        want_mod = {'x': 8, 'z': 4}.get(name, 0)
        assert w['start'] % 16 == want_mod and w['start'] - ends >= C.GUARD, name
        ends = w['start'] + w['nbytes']
        assert A.ptr(name).value == A.dev.data_ptr() + w['start']
    assert A.dev.numel() - ends >= C.GUARD and A.ptr('nothing') is None
    assert A.ptr('z', 2).value == A.ptr('z').value + 8
    if fill == C.FILL_NAN:
        assert bool(torch.isnan(A.view('y').float()).all()) and bool(torch.isnan(A.view('z')).all())
    else:
        assert bool(torch.isfinite(A.view('y').float()).all()) and float(A.view('z')[0]) > 1e4
    assert bool((A.view('dw') != 0).all())
    A.untouched('before the call')
    _kernel(A)
    A.verify('clean')
    assert torch.equal(A.get('z'), torch.full((7,), 2.0))
    with pytest.raises(AssertionError, match=r'a refused call wrote byte \d+ of the buffer \(y\)'):
        A.untouched('after it')


@pytest.mark.parametrize('fill', [C.FILL_NAN, C.FILL_BIG])
def test_arena_sees_a_write_into_a_guard_band(fill):
    for name, where in (('y', -1), ('y', None), ('x', -1), ('ws', None)):
        A = _arena(fill)
        _kernel(A)
        w = A.win[name]
        at = w['start'] - 1 if where == -1 else w['start'] + w['nbytes']
        A.dev[at] = 0
        with pytest.raises(AssertionError, match='guard band next to %s .* was written' % name):
            A.verify('guard')


@pytest.mark.parametrize('fill', [C.FILL_NAN, C.FILL_BIG])
def test_arena_sees_a_changed_input(fill):
    A = _arena(fill)
    _kernel(A)
    A.view('w')[1, 1, 1, 1] += 1
    with pytest.raises(AssertionError, match='input w was changed'):
        A.verify('input')
    A = _arena(fill)
    _kernel(A)
    A.view('x')[0, 0, 0, 0] = -A.view('x')[0, 0, 0, 0]                     # one sign bit
    with pytest.raises(AssertionError, match='input x was changed'):
        A.verify('input')


@pytest.mark.parametrize('fill', [C.FILL_NAN, C.FILL_BIG])
def test_arena_sees_an_untouched_output(fill):
    A = _arena(fill)
    A.view('z').fill_(2.0)
    A.view('dw').add_(1.0)
    with pytest.raises(AssertionError, match='output y was not written everywhere'):
        A.verify('untouched')
    A = _arena(fill)
    _kernel(A)
    A.dev[A.win['z']['start'] + 8:A.win['z']['start'] + 12] = fill              # one element of z left out
    with pytest.raises(AssertionError, match=r'output z was not written everywhere \(element 2 of 7'):
        A.verify('one element')
    A = _arena(fill)
    _kernel(A)
    A.view('dw')[3] = float('inf')
    with pytest.raises(AssertionError, match='non-finite element in dw'):
        A.verify('non-finite')
