"""
The fp32 convolution kernels (csrc/conv_generic.hip, conv_small.hip, conv_mfma.hip) called through the C ABI of include/ttrap.h, every
element held to a derived rounding bound against the float64 restatement of tests/conv_ref.py (pinned against torch by
tests/test_conv_restatement.py).  The model for this file is tests/test_gpu_gemm.py.

Harness.  Every device operand of a call is a window of ONE flat buffer filled with NaN, at least 8 NaN between and around the windows
(a window that starts one float off a 16-byte boundary has them in front as well); scratch is sized exactly as the header prescribes and
guarded the same way.  After the call: everything outside the output and scratch windows is still NaN, the inputs are bit-unchanged,
every output element is finite.  A write past a ragged tile edge, a read of a halo column that is not there, or a store where the
contract says += shows here, where the tensors of the autograd tests sit in the allocator's slack.

Values are uniform in +-[0.5, 1], weights scaled by 1 / sqrt(K): one dropped, doubled or mis-addressed product moves a result by at
least 0.25 / sqrt(K), the bars are about K 2^-24.

Bars (u = 2^-24, S = the sum of absolute products that conv_ref returns, K = the number of products of the sum: channels x taps that
land in the image, or B x rows x frames of a weight / bias gradient restricted in the same way -- whatever the order of summation,
atomics and matrix instructions included):
    a direct result              K u S  +  3 u (|bias| + |residual| + |previous content|)
    ELU                          + 4 u max(1, |v|)              (__expf(a) - 1, as in test_gpu_gemm.py)
    ELU' through the output      + u |g| (and u |dy| for the y + 1 of the gate)
    an unobservable intermediate its bar carried to first order through the next stage in float64 (|W| . bar; ELU and ELU' are
                                 1-Lipschitz): h1 of a forward without h1, h1 recomputed in the backward, dA1 that the fused narrow
                                 backward keeps in LDS, the gated gradient of the strided pair
    a stored intermediate        the kernel's own tensor feeds the next stage of the restatement: h1 of the forward, dA1 in the first
                                 B C H T floats of ws on the three-kernel backward paths (taken where that region came back finite)

Every check prints its ratio to the bar (pytest -rP); the worst ones measured are at the end of this docstring.

Misaligned pointers (one pointer one float off a 16-byte boundary, the others aligned): read from the code before the first run --
LDS-DMA (global_load_lds, 16 bytes per lane) is only ever issued on pointers that the host side tested (x of the forward and of the
3x3 LDS kernels; x, h1, dy of the fused narrow backward; ws / g and x of the DMA gradients), every other tensor is reached by 4-byte
accesses or by 16-byte vector loads / stores at a 4-byte aligned address, which the hardware splits.  The one exception was the gate
pre-pass of tt_sconv_bwd / tt_tconv_bwd (k_gate_and_sum), which read the saved output y as float4 while only x, dy and the scratch had
been asked about: the host condition now includes y.  Outcome of every (entry point, pointer) pair: meets the same bars.

Worst ratios measured on an MI355X (629 cases, 6 s), per family and output:
    tt_resblock_fwd        h1 0.22, y 0.44 (C = 4); C = 8: 0.22 / 0.35; C = 16: 0.08 / 0.21; C = 32: 0.06 / 0.12; multi-tile loop y 0.38
    tt_resblock_bwd        dA1 0.14, dx 0.25, dw1 0.56, db1 0.51, dw2 0.13, db2 0.05; multi-tile loop dx 0.15; TTRAP_SMALL_VALU_FMA and
                           TTRAP_SMALL_FUSED_BWD_C8: y 0.35, dx 0.22
    tt_sconv_fwd / _bwd    y 0.22, dx 0.28, dw 0.52, db 0.34          tt_tconv_fwd / _bwd    y 0.41, dx 0.18, dw 0.48, db 0.12
    tt_conv2d              3x3 specialisations 0.28, 2 <-> 4 on the LDS / small kernel 0.23, flipped data-gradient form 0.32,
                           k_conv_generic 0.70 (data-gradient forms 0.34)
    tt_conv2d_wgrad        k_wgrad3x3_small dw 0.33, db 0.02; k_wgrad_generic dw 0.07, db 0.04
    tt_channel_sum, _ws    0.32
    one pointer misaligned y 0.35, dx 0.22, tt_conv2d 0.22; every (entry point, pointer) pair met the bar, none was refused
(The bars of the weight and bias gradients grow with K = B x rows x frames, so on the larger planes they only catch a lost tile or a
lost previous content; the 1 x 1, 2 x 3 and 3 x 4 planes, where K is 2 to 24, are the ones that catch a single product.)

Broken on purpose in a scratch copy of the sources, one break per kernel family, each made named cases here fail: the right halo column
of k_conv3x3_lds read one column to the left (test_conv2d_3x3_edge_layers[2-4-16-64] and seven more, 1e5 bars off, while every
tt_conv2d case of tests/test_gpu_conv.py still passed: none of its shapes reaches that kernel); the ``hh < H`` test of the bottom tap of
k_conv3x3_small dropped (all 40 cases of test_conv2d_3x3_edge_layers: the row behind the plane is another channel or a NaN guard band);
the atomicAdd of k_gate_and_sum turned into a store (test_sconv / test_tconv at T % 4 == 0, the bias gradient loses what db held);
the store of k_small_lds let through at t == T (test_resblock[4-1-17-68] and 41 more: "guard band next to y ... was written").
"""

import ctypes
import functools
import math

import pytest
import torch

import conv_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PAD = 8
BADARG, UNSUPPORTED = -1, -2
NAN = float('nan')


def _api():
    from timbre_trap import _hip
    return _hip.lib(), _hip.stream_ptr()


_worst = {}


def _note(key, ratio):
    _worst[key] = max(_worst.get(key, 0.0), ratio)
    print('ratio to bar: %-34s %.3f (worst so far %.3f)' % (key, ratio, _worst[key]))


def _pm(gen, *shape):
    """uniform in +-[0.5, 1]"""
    return (0.5 + 0.5 * torch.rand(*shape, generator=gen)) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)


def _hold(key, got, want, bar, what=''):
    e = (got.double() - want).abs()
    ratio = float((e / bar.clamp_min(1e-300)).max()) if e.numel() else 0.0
    _note(key, ratio)
    assert bool((e <= bar).all()), '%s %s: %.3f of the bar (worst element off by %.3e)' % (key, what, ratio, float(e.max()))


def _elu(v):
    return torch.where(v > 0, v, torch.expm1(v))


def _gate(y):
    """ELU' through the output: 1 where y > 0, else y + 1."""
    return torch.where(y > 0, torch.ones_like(y), y + 1)


class _Arena:
    """The operands of one call as windows of a flat NaN-filled device buffer.  kinds: 'in' (must come back bit-unchanged), 'out' (NaN
    before, finite after), 'acc' (a non-zero pattern before, finite after), 'scratch' (NaN before, anything after).  A window starts on
    a 16-byte boundary plus ``shift`` floats, with at least PAD NaN in front of it and behind it."""

    def __init__(self):
        self.win = {}
        self.pos = PAD

    def _add(self, name, kind, shape, vals, shift):
        n = int(math.prod(shape))
        start = (self.pos + 3) // 4 * 4 + shift
        self.win[name] = dict(start=start, n=n, kind=kind, vals=None if vals is None else vals.float().contiguous().reshape(-1), shape=tuple(shape))
        self.pos = start + n + PAD

    def inp(self, name, vals, shift=0):
        self._add(name, 'in', vals.shape, vals, shift)

    def out(self, name, shape, shift=0):
        self._add(name, 'out', shape, None, shift)

    def acc(self, name, vals, shift=0):
        self._add(name, 'acc', vals.shape, vals, shift)

    def scratch(self, name, n, shift=0):
        self._add(name, 'scratch', (n,), None, shift)

    def build(self):
        self.dev = torch.full((self.pos,), NAN, device='cuda')
        assert self.dev.data_ptr() % 16 == 0
        self.inside = torch.zeros(self.pos, dtype=torch.bool, device='cuda')
        for w in self.win.values():
            if w['kind'] != 'in':
                self.inside[w['start']:w['start'] + w['n']] = True
            if w['vals'] is not None:
                self.dev[w['start']:w['start'] + w['n']] = w['vals'].cuda()
        self.before = self.dev.clone()
        return self

    def ptr(self, name, offset=0):
        if name not in self.win:
            return None
        return ctypes.c_void_p(self.dev.data_ptr() + 4 * (self.win[name]['start'] + offset))

    def get(self, name):
        w = self.win[name]
        return self.dev[w['start']:w['start'] + w['n']].cpu().view(w['shape'])

    def verify(self, what):
        """Nothing outside the output and scratch windows changed (guard bands still NaN, inputs bit-unchanged); outputs finite."""
        torch.cuda.synchronize()
        same = (self.dev.view(torch.int32) == self.before.view(torch.int32)) | self.inside
        if not bool(same.all()):
            i = int((~same).nonzero()[0])
            owner = [n for n, w in self.win.items() if w['start'] <= i < w['start'] + w['n']]
            near = min(self.win.items(), key=lambda kv: min(abs(i - kv[1]['start']), abs(i - kv[1]['start'] - kv[1]['n'])))
            raise AssertionError('%s: element %d of the buffer was written: %s' % (
                what, i, 'input %s' % owner[0] if owner else 'guard band next to %s (window %d..%d)' % (
                    near[0], near[1]['start'], near[1]['start'] + near[1]['n'] - 1)))
        for name, w in self.win.items():
            if w['kind'] in ('out', 'acc'):
                assert bool(torch.isfinite(self.dev[w['start']:w['start'] + w['n']]).all()), '%s: non-finite element in %s' % (what, name)


@pytest.fixture
def cu_limit():
    """Cap the CU count the persistent grids are sized with; restored afterwards."""
    lib, _ = _api()
    prev = lib.tt_set_cu_limit(0)
    yield lib.tt_set_cu_limit
    lib.tt_set_cu_limit(prev)


# ---- 1. the fused residual block ------------------------------------------------------------------------------------------------------------
def _rb_geom(C, d):
    return dict(KH=3, KW=3, stride_h=1, dil_h=d, dil_w=d, pad_h=d, pad_w=d)


@functools.lru_cache(maxsize=2)
def _rb_setup(C, d, B, H, T):
    """Operands of one block and the float64 first stage, shared (unchanged) by the forward and backward checks of a case."""
    gen = torch.Generator().manual_seed(1000 * C + 100 * d + 7 * H + T)
    s = dict(x=_pm(gen, B, C, H, T), w1=_pm(gen, C, C, 3, 3) / math.sqrt(9 * C), b1=_pm(gen, C), w2=_pm(gen, C, C, 1, 1) / math.sqrt(C),
             b2=_pm(gen, C), dy=_pm(gen, B, C, H, T), dw1=_pm(gen, C, C, 3, 3), db1=_pm(gen, C), dw2=_pm(gen, C, C, 1, 1), db2=_pm(gen, C))
    _, a1, S1 = R.conv2d(s['x'], s['w1'].reshape(-1), s['b1'], None, Cout=C, Hout=H, transposed=0, ws_co=9 * C, ws_ci=9, ws_kh=3, ws_kw=1,
                         **_rb_geom(C, d))
    K1 = C * R.tap_count(H, H, T, 3, 3, 1, d, d, d, d, 0)
    s['a1'] = a1
    s['bar_a1'] = K1 * U * S1 + 3 * U * s['b1'].double().abs().view(1, C, 1, 1)
    s['h1'] = _elu(a1)
    s['bar_h1'] = s['bar_a1'] + 4 * U * a1.abs().clamp_min(1.0)
    return s


def _rb_forward(C, d, B, H, T, with_h1, key, shifts=None):
    lib, st = _api()
    shifts = shifts or {}
    s = _rb_setup(C, d, B, H, T)
    A = _Arena()
    A.inp('x', s['x'], shifts.get('x', 0))
    for n in ('w1', 'b1', 'w2', 'b2'):
        A.inp(n, s[n])
    A.out('y', (B, C, H, T), shifts.get('y', 0))
    if with_h1:
        A.out('h1', (B, C, H, T), shifts.get('h1', 0))
    A.build()
    rc = lib.tt_resblock_fwd(A.ptr('x'), A.ptr('w1'), A.ptr('b1'), A.ptr('w2'), A.ptr('b2'), A.ptr('y'), A.ptr('h1'), B, C, H, T, d, 0, st)
    what = 'tt_resblock_fwd C %d d %d plane (%d, %d) %s h1' % (C, d, H, T, 'with' if with_h1 else 'without')
    if rc != 0:
        A.verify(what + ' (refused)')
        return rc
    A.verify(what)
    W2 = s['w2'].double().view(C, C)
    x, b2 = s['x'].double(), s['b2'].double().view(1, C, 1, 1)
    if with_h1:                  # stored: held to its own bar, then it feeds the second stage as the kernel's registers did
        hh = A.get('h1').double()
        _hold(key + ' h1', hh, s['h1'], s['bar_h1'], what)
        carried = 0.0
    else:                        # unobservable: its bar is carried through |W2|
        hh = s['h1']
        carried = torch.einsum('oc,bcht->boht', W2.abs(), s['bar_h1'])
    a2 = torch.einsum('oc,bcht->boht', W2, hh) + b2
    S2 = torch.einsum('oc,bcht->boht', W2.abs(), hh.abs())
    bar = C * U * S2 + 3 * U * (b2.abs() + x.abs()) + 4 * U * a2.abs().clamp_min(1.0) + carried
    _hold(key + ' y', A.get('y'), _elu(a2) + x, bar, what)
    return 0


def _rb_backward(C, d, B, H, T, with_h1, key, shifts=None):
    lib, st = _api()
    shifts = shifts or {}
    s = _rb_setup(C, d, B, H, T)
    n = B * C * H * T
    A = _Arena()
    A.inp('x', s['x'], shifts.get('x', 0))
    if with_h1:
        A.inp('h1', s['h1'].float(), shifts.get('h1', 0))         # what a forward saved: the fp32 rounding of the reference's
    A.inp('dy', s['dy'], shifts.get('dy', 0))
    for name in ('w1', 'b1', 'w2', 'b2'):
        A.inp(name, s[name])
    A.out('dx', (B, C, H, T), shifts.get('dx', 0))
    for name in ('dw1', 'db1', 'dw2', 'db2'):
        A.acc(name, s[name])
    A.scratch('ws', n + int(lib.tt_wgrad_scratch_floats()), shifts.get('ws', 0))
    A.build()
    rc = lib.tt_resblock_bwd(A.ptr('x'), A.ptr('h1'), A.ptr('dy'), A.ptr('w1'), A.ptr('b1'), A.ptr('w2'), A.ptr('b2'), A.ptr('dx'),
                             A.ptr('dw1'), A.ptr('db1'), A.ptr('dw2'), A.ptr('db2'), A.ptr('ws'), B, C, H, T, d, 0, st)
    what = 'tt_resblock_bwd C %d d %d plane (%d, %d) %s h1' % (C, d, H, T, 'saved' if with_h1 else 'recomputed')
    if rc != 0:
        A.verify(what + ' (refused)')
        return rc
    A.verify(what)

    x, dy = s['x'].double(), s['dy'].double()
    W2 = s['w2'].double().view(C, C)
    b2 = s['b2'].double().view(1, C, 1, 1)
    N = B * H * T
    if with_h1:
        h, bh = s['h1'].float().double(), torch.zeros((), dtype=torch.float64)
    else:
        h, bh = s['h1'], s['bar_h1']
    # pointwise chain: a2 = W2 h + b2, dA2 = dy ELU'(a2), dH1 = W2^T dA2, dA1 = dH1 ELU'(h) -- all in registers, bars carried
    a2 = torch.einsum('oc,bcht->boht', W2, h) + b2
    bar_a2 = C * U * torch.einsum('oc,bcht->boht', W2.abs(), h.abs()) + 3 * U * b2.abs() + torch.einsum('oc,bcht->boht', W2.abs(), bh.expand_as(h))
    g2 = dy * _gate(_elu(a2))
    bar_g2 = dy.abs() * (bar_a2 + 5 * U) + U * g2.abs()                       # ELU (4u), its + 1 (u), the product (u |g2|)
    prev = {k: s[k].double() for k in ('dw1', 'db1', 'dw2', 'db2')}
    _hold(key + ' db2', A.get('db2'), prev['db2'] + g2.sum((0, 2, 3)),
          N * U * g2.abs().sum((0, 2, 3)) + bar_g2.sum((0, 2, 3)) + 3 * U * prev['db2'].abs(), what)
    dw2 = torch.einsum('boht,bcht->oc', g2, h)
    bar_dw2 = (N * U * torch.einsum('boht,bcht->oc', g2.abs(), h.abs()) + torch.einsum('boht,bcht->oc', bar_g2, h.abs())
               + torch.einsum('boht,bcht->oc', g2.abs(), bh.expand_as(h)) + 3 * U * prev['dw2'].view(C, C).abs())
    _hold(key + ' dw2', A.get('dw2').view(C, C), prev['dw2'].view(C, C) + dw2, bar_dw2, what)
    dh = torch.einsum('oc,boht->bcht', W2, g2)
    bar_dh = C * U * torch.einsum('oc,boht->bcht', W2.abs(), g2.abs()) + torch.einsum('oc,boht->bcht', W2.abs(), bar_g2)
    gp1 = _gate(h)
    da1 = dh * gp1
    bar_da1 = bar_dh * gp1.abs() + dh.abs() * (bh + U) + U * da1.abs()
    stored = A.get('ws').view(-1)[:n].view(B, C, H, T)
    if bool(torch.isfinite(stored).all()):       # three-kernel path: dA1 went through memory, the kernel's own tensor feeds the rest
        print('dA1 stored in ws (three-kernel path)')
        _hold(key + ' dA1', stored, da1, bar_da1, what)
        g1, bg = stored.double(), None
    else:                                        # fused narrow backward: dA1 never left the LDS
        print('dA1 not stored (fused narrow backward)')
        assert bool(torch.isnan(stored).all()), 'the dA1 region of ws is partly written'
        g1, bg = da1, bar_da1
    _hold(key + ' db1', A.get('db1'), prev['db1'] + g1.sum((0, 2, 3)),
          N * U * g1.abs().sum((0, 2, 3)) + (bg.sum((0, 2, 3)) if bg is not None else 0.0) + 3 * U * prev['db1'].abs(), what)
    dw1, S, K, _, _ = R.conv2d_wgrad(x, g1, **_rb_geom(C, d))
    bar = K.view(1, 1, 3, 3) * U * S + 3 * U * prev['dw1'].abs()
    if bg is not None:
        bar = bar + R.conv2d_wgrad(x.abs(), bg, **_rb_geom(C, d))[0]
    _hold(key + ' dw1', A.get('dw1'), prev['dw1'] + dw1, bar, what)
    flip = R.dgrad_args('conv', C, C, 3, 3, 1, d, d, d)
    dx, _, S = R.conv2d(g1, s['w1'].reshape(-1), None, dy, Hout=H, **flip)
    bar = C * R.tap_count(H, H, T, 3, 3, 1, d, d, d, d, 0) * U * S + 3 * U * dy.abs()
    if bg is not None:
        bar = bar + R.conv2d(bg, s['w1'].reshape(-1).abs(), None, None, Hout=H, **flip)[0]
    _hold(key + ' dx', A.get('dx'), dx, bar, what)
    return 0


RB_PLANES = [(1, 1), (2, 3), (3, 4),              # smaller than the halo: with dilation 3 every tap but the centre is outside
             (8, 64), (16, 64),                   # exactly one tile (8 x 64 MFMA, 16 x 64 narrow / 3x3 LDS kernels)
             (9, 65), (17, 68), (7, 132)]         # one past the tile in H, T or both; T % 4 both 0 and not


@pytest.mark.parametrize('H,T', RB_PLANES)
@pytest.mark.parametrize('d', [1, 2, 3])
@pytest.mark.parametrize('C', [4, 8, 16, 32])
def test_resblock(C, d, H, T, B=2):
    """tt_resblock_fwd with and without h1 (both held to their bars: the four-pixel narrow forward needs an aligned h1 and NULL counts
    as aligned, but the wide forward stores h1 between the two stages, so the two runs are not one instruction sequence everywhere),
    tt_resblock_bwd from the saved h1 and with h1 = NULL, gradients accumulated onto a non-zero pattern, dx written over NaN."""
    fam = 'resblock C%d' % C
    for with_h1 in (True, False):
        assert _rb_forward(C, d, B, H, T, with_h1, fam + ' fwd') == 0
        assert _rb_backward(C, d, B, H, T, with_h1, fam + ' bwd') == 0


@pytest.mark.parametrize('d', [1, 2, 3])
@pytest.mark.parametrize('C', [4, 8, 16, 32])
def test_resblock_persistent_loop(C, d, cu_limit, B=1, H=33, T=200):
    """One CU's worth of workgroups walks all the tiles of a (33, 200) plane: the multi-tile loops with their prefetch of the next tile."""
    cu_limit(1)
    fam = 'resblock C%d multi-tile' % C
    for with_h1 in (True, False):
        assert _rb_forward(C, d, B, H, T, with_h1, fam + ' fwd') == 0
        assert _rb_backward(C, d, B, H, T, with_h1, fam + ' bwd') == 0


@pytest.mark.parametrize('H,T', [(16, 64), (17, 68)])
@pytest.mark.parametrize('d', [1, 2, 3])
@pytest.mark.parametrize('C,switch', [(4, 'TTRAP_SMALL_VALU_FMA'), (8, 'TTRAP_SMALL_VALU_FMA'), (8, 'TTRAP_SMALL_FUSED_BWD_C8')])
def test_resblock_narrow_switches(C, switch, d, H, T, monkeypatch, B=2):
    """The per-call switches of csrc/conv_small.hip: the vector-ALU form of the LDS kernels, and the fused backward at C = 8."""
    monkeypatch.setenv(switch, '1')
    fam = 'resblock C%d %s' % (C, switch)
    for with_h1 in (True, False):
        assert _rb_forward(C, d, B, H, T, with_h1, fam + ' fwd') == 0
        assert _rb_backward(C, d, B, H, T, with_h1, fam + ' bwd') == 0


# ---- 5. the strided pair ---------------------------------------------------------------------------------------------------------------------
def _stride_layer(kind, C):
    """(layer description for conv_ref, channels in, channels out): EncoderBlock.sconv C -> 2C, DecoderBlock.tconv 2C -> C."""
    if kind == 'sconv':
        return ('conv', C, 2 * C, 4, 1, 2, 1, 0, 0), C, 2 * C
    return ('tconv', 2 * C, C, 4, 1, 2, 1, 0, 0), 2 * C, C


@functools.lru_cache(maxsize=2)
def _stride_setup(kind, C, B, H, T, out_pad):
    layer, Ci, Co = _stride_layer(kind, C)
    gen = torch.Generator().manual_seed(10000 * (kind == 'sconv') + 100 * C + 10 * H + T + out_pad)
    Hout = R.out_rows(layer[0], H, 4, 2, 1, 0, out_pad)
    s = dict(x=_pm(gen, B, Ci, H, T), w=_pm(gen, 2 * C, C, 4, 1) / math.sqrt(4 * Ci), b=_pm(gen, Co), dy=_pm(gen, B, Co, Hout, T),
             dw=_pm(gen, 2 * C, C, 4, 1), db=_pm(gen, Co), Hout=Hout)
    fa = R.forward_args(*layer)
    y, v, S = R.conv2d(s['x'], s['w'].reshape(-1), s['b'], None, Hout=Hout, act=R.ACT_ELU, **fa)
    K = Ci * R.tap_count(H, Hout, T, 4, 1, 2, 1, 1, 0, 0, fa['transposed'])
    s['y'] = y
    s['bar_y'] = K * U * S + 3 * U * s['b'].double().abs().view(1, Co, 1, 1) + 4 * U * v.abs().clamp_min(1.0)
    return s


def _stride_call(kind, entry, args, B, C, H, T, out_pad, st):
    lib, _ = _api()
    fn = getattr(lib, 'tt_%s_%s' % (kind, entry))
    tail = (B, C, H, T) + ((out_pad,) if kind == 'tconv' else ()) + (st,)
    return fn(*args, *tail)


def _stride_forward(kind, C, B, H, T, out_pad, key, shifts=None):
    lib, st = _api()
    shifts = shifts or {}
    layer, Ci, Co = _stride_layer(kind, C)
    s = _stride_setup(kind, C, B, H, T, out_pad)
    A = _Arena()
    A.inp('x', s['x'], shifts.get('x', 0))
    A.inp('w', s['w'])
    A.inp('b', s['b'])
    A.out('y', (B, Co, s['Hout'], T), shifts.get('y', 0))
    A.build()
    what = 'tt_%s_fwd C %d plane (%d, %d) out_pad %d' % (kind, C, H, T, out_pad)
    rc = _stride_call(kind, 'fwd', [A.ptr('x'), A.ptr('w'), A.ptr('b'), A.ptr('y')], B, C, H, T, out_pad, st)
    if rc != 0:
        A.verify(what + ' (refused)')
        return rc
    A.verify(what)
    _hold(key + ' y', A.get('y'), s['y'], s['bar_y'], what)
    return 0


def _stride_backward(kind, C, B, H, T, out_pad, key, shifts=None, with_dx=True):
    lib, st = _api()
    shifts = shifts or {}
    layer, Ci, Co = _stride_layer(kind, C)
    s = _stride_setup(kind, C, B, H, T, out_pad)
    Hout = s['Hout']
    y32 = s['y'].float()                                   # the saved output: the fp32 rounding of the reference's
    A = _Arena()
    A.inp('x', s['x'], shifts.get('x', 0))
    A.inp('y', y32, shifts.get('y', 0))
    A.inp('dy', s['dy'], shifts.get('dy', 0))
    A.inp('w', s['w'])
    if with_dx:
        A.out('dx', (B, Ci, H, T), shifts.get('dx', 0))
    A.acc('dw', s['dw'])
    A.acc('db', s['db'])
    A.scratch('scratch', int(lib.tt_wgrad_scratch_floats()) + B * Co * Hout * T, shifts.get('scratch', 0))
    A.build()
    what = 'tt_%s_bwd C %d plane (%d, %d) out_pad %d%s' % (kind, C, H, T, out_pad, '' if with_dx else ' dx = NULL')
    rc = _stride_call(kind, 'bwd', [A.ptr('x'), A.ptr('y'), A.ptr('dy'), A.ptr('w'), A.ptr('dx'), A.ptr('dw'), A.ptr('db'), A.ptr('scratch')],
                      B, C, H, T, out_pad, st)
    if rc != 0:
        A.verify(what + ' (refused)')
        return rc
    A.verify(what)
    x, dy = s['x'].double(), s['dy'].double()
    g = dy * _gate(y32.double())
    bar_g = U * dy.abs() + U * g.abs()                     # the y + 1 of the gate, the product; carried through the three sums below
    N = B * Hout * T
    prev_w, prev_b = s['dw'].double(), s['db'].double()
    _hold(key + ' db', A.get('db'), prev_b + g.sum((0, 2, 3)), N * U * g.abs().sum((0, 2, 3)) + bar_g.sum((0, 2, 3)) + 3 * U * prev_b.abs(), what)
    swap, wg, _ = R.wgrad_args(*layer)
    p, q = (g, x) if swap else (x, g)
    dw, S, K, _, _ = R.conv2d_wgrad(p, q, **wg)
    bp, bq = (bar_g, x.abs()) if swap else (x.abs(), bar_g)
    bar = K.view(1, 1, 4, 1) * U * S + R.conv2d_wgrad(bp, bq, **wg)[0] + 3 * U * prev_w.abs()
    _hold(key + ' dw', A.get('dw'), prev_w + dw, bar, what)
    if with_dx:
        da = R.dgrad_args(*layer)
        dx, _, S = R.conv2d(g, s['w'].reshape(-1), None, None, Hout=H, **da)
        K = Co * R.tap_count(Hout, H, T, 4, 1, 2, 1, 1, 0, 0, da['transposed'])
        bar = K * U * S + R.conv2d(bar_g, s['w'].reshape(-1).abs(), None, None, Hout=H, **da)[0]
        got = A.get('dx')
        _hold(key + ' dx', got, dx, bar, what)
        if kind == 'sconv' and H % 2 == 1:
            assert bool((got[:, :, -1] == 0).all()), 'the unused last input row has no term: its dx is 0'
    return 0


STRIDE_T = [1, 4, 64, 66, 132]        # T % 4 == 0: both operands by LDS-DMA behind the gate pre-pass; else staged through registers


@pytest.mark.parametrize('T', STRIDE_T)
@pytest.mark.parametrize('H', [4, 5, 6, 19])
@pytest.mark.parametrize('C', [4, 8, 16, 32])
def test_sconv(C, H, T, B=2):
    """tt_sconv_fwd / tt_sconv_bwd: the minimum height, an odd one (the last input row is unused: its dx row is exactly 0), an even one,
    one past a tile; dw and db accumulate onto a non-zero pattern on both staging paths; dx = NULL leaves the rest correct."""
    fam = 'sconv C%d' % C
    assert _stride_forward('sconv', C, B, H, T, 0, fam + ' fwd') == 0
    assert _stride_backward('sconv', C, B, H, T, 0, fam + ' bwd') == 0
    if H in (5, 19):
        assert _stride_backward('sconv', C, B, H, T, 0, fam + ' bwd', with_dx=False) == 0


@pytest.mark.parametrize('T', STRIDE_T)
@pytest.mark.parametrize('H,out_pad', [(1, 0), (1, 1), (2, 0), (2, 1), (9, 0), (9, 1)])
@pytest.mark.parametrize('C', [4, 8, 16, 32])
def test_tconv(C, H, out_pad, T, B=2):
    fam = 'tconv C%d' % C
    assert _stride_forward('tconv', C, B, H, T, out_pad, fam + ' fwd') == 0
    assert _stride_backward('tconv', C, B, H, T, out_pad, fam + ' bwd') == 0
    if H == 2:
        assert _stride_backward('tconv', C, B, H, T, out_pad, fam + ' bwd', with_dx=False) == 0


def test_sconv_refuses_three_rows():
    lib, st = _api()
    C, B, T = 4, 1, 8
    t = torch.ones(B * 2 * C * 3 * T + int(lib.tt_wgrad_scratch_floats()), device='cuda')
    p = ctypes.c_void_p(t.data_ptr())
    assert lib.tt_sconv_fwd(p, p, p, p, B, C, 3, T, st) == BADARG
    assert lib.tt_sconv_bwd(p, p, p, p, p, p, p, p, B, C, 3, T, st) == BADARG
    torch.cuda.synchronize()
    assert bool((t == 1).all())


# ---- 2. one pointer off a 16-byte boundary ---------------------------------------------------------------------------------------------------
def _outcome(entry, pointer, rc):
    print('misaligned %-16s %-8s: %s' % (entry, pointer, 'meets the bar' if rc == 0 else 'refused with status %d' % rc))


@pytest.mark.parametrize('H,T', [(16, 64), (17, 68)])
@pytest.mark.parametrize('pointer', ['x', 'y', 'h1', 'dy', 'dx', 'ws'])
@pytest.mark.parametrize('C', [4, 8, 16])
def test_resblock_one_pointer_misaligned(C, pointer, H, T, B=2, d=2):
    """Each pointer in turn one float off a 16-byte boundary: the call meets the same bars or returns a non-zero status (and then writes
    nothing).  The dispatch falls back to register staging where the pointer would have fed the LDS-DMA."""
    fam = 'misaligned resblock C%d' % C
    if pointer in ('x', 'y', 'h1'):
        _outcome('tt_resblock_fwd', pointer, _rb_forward(C, d, B, H, T, True, fam + ' fwd', {pointer: 1}))
        if pointer != 'h1':
            _outcome('tt_resblock_fwd', pointer + ' (no h1)', _rb_forward(C, d, B, H, T, False, fam + ' fwd', {pointer: 1}))
    if pointer in ('x', 'h1', 'dy', 'dx', 'ws'):
        _outcome('tt_resblock_bwd', pointer, _rb_backward(C, d, B, H, T, True, fam + ' bwd', {pointer: 1}))
        if pointer != 'h1':
            _outcome('tt_resblock_bwd', pointer + ' (no h1)', _rb_backward(C, d, B, H, T, False, fam + ' bwd', {pointer: 1}))


@pytest.mark.parametrize('T', [64, 68])
@pytest.mark.parametrize('pointer', ['x', 'y', 'dy', 'dx', 'scratch'])
@pytest.mark.parametrize('C', [4, 16])
@pytest.mark.parametrize('kind', ['sconv', 'tconv'])
def test_strided_backward_one_pointer_misaligned(kind, C, pointer, T, B=2):
    H = 17 if kind == 'sconv' else 8
    _outcome('tt_%s_bwd' % kind, pointer, _stride_backward(kind, C, B, H, T, 1 if kind == 'tconv' else 0, 'misaligned %s C%d bwd' % (kind, C),
                                                          {pointer: 1}))


# ---- 3. tt_conv2d ----------------------------------------------------------------------------------------------------------------------------
def _conv2d(key, B, Cin, Hin, T, Hout, a, wdense, act=R.ACT_NONE, bias=True, res=False, seed=0, shifts=None):
    """One tt_conv2d call with the argument set ``a`` (conv_ref.forward_args / dgrad_args) over the dense weight ``wdense``, whose
    flat storage the strides and the base of ``a`` address."""
    lib, st = _api()
    shifts = shifts or {}
    gen = torch.Generator().manual_seed(seed)
    Cout = a['Cout']
    x = _pm(gen, B, Cin, Hin, T)
    bv = _pm(gen, Cout) if bias else None
    rv = _pm(gen, B, Cout, Hout, T) if res else None
    A = _Arena()
    A.inp('x', x, shifts.get('x', 0))
    A.inp('w', wdense)
    if bias:
        A.inp('b', bv)
    if res:
        A.inp('res', rv)
    A.out('y', (B, Cout, Hout, T), shifts.get('y', 0))
    A.build()
    what = 'tt_conv2d %d -> %d, %dx%d stride %d dil %d transposed %d, plane (%d, %d), act %d' % (
        Cin, Cout, a['KH'], a['KW'], a['stride_h'], a['dil_h'], a['transposed'], Hin, T, act)
    rc = lib.tt_conv2d(A.ptr('x'), A.ptr('w', a['base']), A.ptr('b'), A.ptr('res'), A.ptr('y'), B, Cin, Hin, T, Cout, Hout, a['KH'], a['KW'],
                       a['stride_h'], a['dil_h'], a['dil_w'], a['pad_h'], a['pad_w'], a['transposed'], a['ws_co'], a['ws_ci'], a['ws_kh'],
                       a['ws_kw'], act, st)
    if rc != 0:
        A.verify(what + ' (refused)')
        return rc
    A.verify(what)
    y, v, S = R.conv2d(x, wdense.reshape(-1), bv, rv, Hout=Hout, act=act, **a)
    K = Cin * R.tap_count(Hin, Hout, T, a['KH'], a['KW'], a['stride_h'], a['dil_h'], a['dil_w'], a['pad_h'], a['pad_w'], a['transposed'])
    bar = K * U * S
    if bias:
        bar = bar + 3 * U * bv.double().abs().view(1, Cout, 1, 1)
    if res:
        bar = bar + 3 * U * rv.double().abs()
    if act == R.ACT_ELU:
        bar = bar + 4 * U * v.abs().clamp_min(1.0)
    elif act == R.ACT_SIGMOID:
        bar = bar + 4 * U                 # 1 / (1 + expf(-v)): exp, sum and quotient each within an ulp of a value below 1; 1/4-Lipschitz
    _hold(key, A.get('y'), y, bar, what)
    return 0


def _w(gen, Cout, Cin, KH, KW, transposed_layout=False):
    shape = (Cin, Cout, KH, KW) if transposed_layout else (Cout, Cin, KH, KW)
    return _pm(gen, *shape) / math.sqrt(Cin * KH * KW)


@pytest.mark.parametrize('H,T', [(1, 1), (2, 3), (5, 66), (16, 64), (17, 68)])
@pytest.mark.parametrize('Cin,Cout', [(1, 2), (1, 4), (2, 1), (2, 2), (2, 4), (4, 1), (4, 2), (4, 4)])
def test_conv2d_3x3_edge_layers(Cin, Cout, H, T, B=2):
    """The 3x3 'same' specialisations for all eight channel pairs.  (2, 4) and (4, 2) take the LDS-tiled kernel where T % 4 == 0 and x is
    aligned and k_conv3x3_small otherwise (T = 66, T = 1, 3, or x one float off); both also in the flipped-kernel data-gradient form
    (negative ws_kh / ws_kw, w pointing at the last tap).  ELU, bias, and a residual on every other case."""
    gen = torch.Generator().manual_seed(Cin * 10 + Cout)
    key = 'conv2d 3x3 %s' % ('2<->4' if Cin * Cout == 8 else 'small')
    w = _w(gen, Cout, Cin, 3, 3)
    fa = R.forward_args('conv', Cin, Cout, 3, 3, 1, 1, 1, 1)
    assert _conv2d(key, B, Cin, H, T, H, fa, w, act=R.ACT_ELU, res=(H + T) % 2 == 0, seed=H * T) == 0
    if Cin * Cout == 8:
        assert _conv2d(key + ' x+1', B, Cin, H, T, H, fa, w, act=R.ACT_ELU, seed=H * T, shifts={'x': 1}) == 0
        # the data gradient of the layer Cout -> Cin that shares these channel counts: g has Cin channels here, the weight is (Cin, Cout, 3, 3)
        wl = _w(gen, Cin, Cout, 3, 3)
        da = R.dgrad_args('conv', Cout, Cin, 3, 3, 1, 1, 1, 1)
        assert da['Cout'] == Cout and da['ws_kh'] == -3 and da['ws_kw'] == -1 and da['base'] == 8
        assert _conv2d(key + ' flipped', B, Cin, H, T, H, da, wl, bias=False, seed=H * T + 1) == 0
        assert _conv2d(key + ' flipped x+1', B, Cin, H, T, H, da, wl, bias=False, seed=H * T + 1, shifts={'x': 1}) == 0


GENERIC_KERNELS = [
    # name, kind, KH, KW, stride, dil, pad, out_pad
    ('1x1', 'conv', 1, 1, 1, 1, 0, 0),
    ('3x3 d2', 'conv', 3, 3, 1, 2, 2, 0),
    ('3x3 d3', 'conv', 3, 3, 1, 3, 3, 0),
    ('4x1 s2', 'conv', 4, 1, 2, 1, 0, 0),
    ('4x1 s2 T', 'tconv', 4, 1, 2, 1, 0, 0),
    ('4x1 s2 T+1', 'tconv', 4, 1, 2, 1, 0, 1),
]


@pytest.mark.parametrize('T', [3, 64, 65, 130, 256, 259])
@pytest.mark.parametrize('kernel', GENERIC_KERNELS, ids=[k[0].replace(' ', '-') for k in GENERIC_KERNELS])
@pytest.mark.parametrize('Cout', [2, 8, 16, 24])
def test_conv2d_generic(Cout, kernel, T, B=2, Cin=3, H=5):
    """k_conv_generic<4 | 8 | 16> (Cout 2, 8, 16 and 24 = one full and one partial register tile) at the three block sizes and their
    tails; the activation, a missing bias and a residual rotate through the cases (all four activations, bias = NULL and res != NULL
    meet every kernel shape and every Cout)."""
    name, kind, KH, KW, stride, dil, pad, out_pad = kernel
    idx = GENERIC_KERNELS.index(kernel) + [3, 64, 65, 130, 256, 259].index(T) + Cout // 8
    gen = torch.Generator().manual_seed(idx)
    pad_w = pad if KW > 1 else 0
    Hout = R.out_rows(kind, H, KH, stride, dil, pad, out_pad)
    w = _w(gen, Cout, Cin, KH, KW, transposed_layout=kind == 'tconv')
    fa = R.forward_args(kind, Cin, Cout, KH, KW, stride, dil, pad, pad_w)
    assert _conv2d('conv2d generic', B, Cin, H, T, Hout, fa, w, act=idx % 4, bias=idx % 3 != 0, res=idx % 2 == 1, seed=idx) == 0


@pytest.mark.parametrize('kernel', GENERIC_KERNELS[:4], ids=[k[0].replace(' ', '-') for k in GENERIC_KERNELS[:4]])
def test_conv2d_generic_data_gradient_forms(kernel, B=2, Cin=3, Cout=6, H=7, T=65):
    """The data-gradient argument sets of ops/fp32.py on the generic kernel: flipped through negative strides (unit stride), the
    transposed form of a strided conv, and the strided conv that is the gradient of a transposed one."""
    name, kind, KH, KW, stride, dil, pad, out_pad = kernel
    gen = torch.Generator().manual_seed(KH * 10 + dil)
    pad_w = pad if KW > 1 else 0
    Hout = R.out_rows(kind, H, KH, stride, dil, pad, out_pad)
    w = _w(gen, Cout, Cin, KH, KW)
    assert _conv2d('conv2d generic dgrad', B, Cout, Hout, T, H, R.dgrad_args(kind, Cin, Cout, KH, KW, stride, dil, pad, pad_w), w, bias=False,
                   seed=KH) == 0
    if KH == 4:
        wt = _w(gen, Cout, Cin, KH, KW, transposed_layout=True)
        Ht = R.out_rows('tconv', H, KH, stride, 1, 0, 1)
        assert _conv2d('conv2d generic dgrad', B, Cout, Ht, T, H, R.dgrad_args('tconv', Cin, Cout, KH, KW, stride, 1, 0, 0), wt, bias=False,
                       seed=KH + 1) == 0


def test_conv2d_argument_checks():
    lib, st = _api()
    t = torch.ones(4096, device='cuda')
    p = ctypes.c_void_p(t.data_ptr())

    def call(x=p, w=p, y=p, transposed=0, dil_h=1, B=1, stride=1):
        return lib.tt_conv2d(x, w, None, None, y, B, 2, 4, 8, 2, 4, 3, 3, stride, dil_h, 1, 1, 1, transposed, 18, 9, 3, 1, 0, st)
    assert call(x=None) == BADARG and call(w=None) == BADARG and call(y=None) == BADARG
    assert call(B=0) == BADARG and call(stride=0) == BADARG
    assert call(transposed=1, dil_h=2) == UNSUPPORTED
    assert lib.tt_conv2d_wgrad(None, p, p, None, 1, 2, 4, 8, 2, 4, 3, 3, 1, 1, 1, 1, 1, 18, 9, 3, 1, st) == BADARG
    assert lib.tt_conv2d_wgrad(p, p, None, None, 1, 2, 4, 8, 2, 4, 3, 3, 1, 1, 1, 1, 1, 18, 9, 3, 1, st) == BADARG
    assert lib.tt_conv2d_wgrad(p, p, p, None, 1, 2, 4, 8, 2, 4, 3, 4, 1, 1, 1, 1, 1, 24, 12, 4, 1, st) == UNSUPPORTED      # KW > 3
    torch.cuda.synchronize()
    assert bool((t == 1).all())


@pytest.mark.parametrize('pointer', ['x', 'y'])
@pytest.mark.parametrize('Cin,Cout', [(2, 4), (4, 2)])
@pytest.mark.parametrize('H,T', [(16, 64), (17, 68)])
def test_conv2d_one_pointer_misaligned(Cin, Cout, pointer, H, T, B=2):
    gen = torch.Generator().manual_seed(Cin)
    w = _w(gen, Cout, Cin, 3, 3)
    rc = _conv2d('misaligned conv2d', B, Cin, H, T, H, R.forward_args('conv', Cin, Cout, 3, 3, 1, 1, 1, 1), w, act=R.ACT_ELU, res=True, seed=T,
                 shifts={pointer: 1})
    _outcome('tt_conv2d %dto%d' % (Cin, Cout), pointer, rc)


# ---- 4. tt_conv2d_wgrad ----------------------------------------------------------------------------------------------------------------------
def _wgrad(key, B, layer, Hin, T, out_pad=0, with_bias=True, seed=0):
    """tt_conv2d_wgrad with the argument set ops/fp32.py builds for ``layer`` (conv_ref.wgrad_args: the plain form, or the role-swapped
    one of a transposed layer), dw and dbias accumulated onto a non-zero pattern."""
    lib, st = _api()
    kind, Cin, Cout, KH, KW, stride, dil, pad_h, pad_w = layer
    gen = torch.Generator().manual_seed(seed)
    Hout = R.out_rows(kind, Hin, KH, stride, dil, pad_h, out_pad)
    x = _pm(gen, B, Cin, Hin, T)
    g = _pm(gen, B, Cout, Hout, T)
    wshape = (Cout, Cin, KH, KW) if kind == 'conv' else (Cin, Cout, KH, KW)
    prev_w, prev_b = _pm(gen, *wshape), _pm(gen, wshape[0])
    swap, wg, strides = R.wgrad_args(*layer)
    p, q = (g, x) if swap else (x, g)                     # the kernel's "x" and "g"
    A = _Arena()
    A.inp('p', p)
    A.inp('q', q)
    A.acc('dw', prev_w)
    if with_bias:
        A.acc('db', prev_b)
    A.build()
    what = 'tt_conv2d_wgrad %s %d -> %d, %dx%d stride %d dil %d, B %d plane (%d, %d)%s' % (kind, Cin, Cout, KH, KW, stride, dil, B, Hin, T,
                                                                                        '' if with_bias else ', dbias NULL')
    rc = lib.tt_conv2d_wgrad(A.ptr('p'), A.ptr('q'), A.ptr('dw'), A.ptr('db'), B, p.size(1), p.size(2), T, q.size(1), q.size(2), KH, KW,
                             wg['stride_h'], wg['dil_h'], wg['dil_w'], wg['pad_h'], wg['pad_w'], strides['ws_co'], strides['ws_ci'],
                             strides['ws_kh'], strides['ws_kw'], st)
    assert rc == 0, what
    A.verify(what)
    dw, S, K, db, Sb = R.conv2d_wgrad(p, q, **wg)
    idx = R.weight_index(q.size(1), p.size(1), KH, KW, **strides)
    assert torch.equal(idx.reshape(-1), torch.arange(dw.numel()))
    pw = prev_w.double()
    _hold(key + ' dw', A.get('dw'), pw + dw, K.view(1, 1, KH, KW) * U * S + 3 * U * pw.abs(), what)
    if with_bias:
        pb = prev_b.double()
        _hold(key + ' db', A.get('db'), pb + db, B * q.size(2) * T * U * Sb + 3 * U * pb.abs(), what)


@pytest.mark.parametrize('T', [5, 256, 257])
@pytest.mark.parametrize('Cin,Cout', [(2, 4), (4, 2)])
def test_wgrad_3x3_edge_layers(Cin, Cout, T, cu_limit):
    """k_wgrad3x3_small (tiles of 256 frames), both directions; with the grid capped one workgroup walks several tiles."""
    layer = ('conv', Cin, Cout, 3, 3, 1, 1, 1, 1)
    _wgrad('wgrad 3x3 2<->4', 2, layer, 3, T, seed=T)
    _wgrad('wgrad 3x3 2<->4', 1, layer, 1, T, with_bias=False, seed=T + 1)
    cu_limit(1)
    _wgrad('wgrad 3x3 2<->4', 3, layer, 9, T, seed=T + 2)


WGRAD_LAYERS = [
    # layer (kind, Cin, Cout, KH, KW, stride, dil, pad_h, pad_w), B, Hin, T
    (('conv', 3, 6, 1, 1, 1, 1, 0, 0), 2, 5, 65),
    (('conv', 3, 6, 3, 3, 1, 1, 1, 1), 2, 5, 65),
    (('conv', 3, 6, 3, 3, 1, 3, 3, 3), 2, 2, 3),          # a plane inside the halo: only the centre tap sums anything
    (('conv', 3, 6, 3, 3, 1, 2, 2, 2), 1, 7, 130),
    (('conv', 3, 6, 4, 1, 2, 1, 0, 0), 2, 9, 64),
    (('conv', 5, 7, 4, 1, 2, 1, 0, 0), 3, 6, 259),
    (('tconv', 6, 3, 4, 1, 2, 1, 0, 0), 2, 5, 65),        # the role-swapped form of a transposed layer
    (('tconv', 7, 5, 4, 1, 2, 1, 0, 0), 1, 3, 256),
    (('conv', 32, 64, 4, 1, 2, 1, 0, 0), 1, 20, 5),       # 1024 column blocks: 8 chunks wanted, 9 rows -> 2 rows per chunk, the last chunk 1
    (('conv', 32, 64, 4, 1, 2, 1, 0, 0), 1, 12, 5),       # 5 rows: fewer rows than the 8 chunks
    (('conv', 3, 6, 3, 3, 1, 1, 1, 1), 1, 683, 3),        # 12 column blocks: 341 chunks wanted, 683 rows -> 3 per chunk, the last chunk 2
]


@pytest.mark.parametrize('case', WGRAD_LAYERS, ids=['%s-%dto%d-k%d-s%d-d%d-B%d-H%d-T%d' % (c[0][0], c[0][1], c[0][2], c[0][3], c[0][5], c[0][6],
                                                                                         c[1], c[2], c[3]) for c in WGRAD_LAYERS])
def test_wgrad_generic(case):
    """k_wgrad_generic: channel counts that are no multiples of its 2 x 4 register tile, KH 1 / 3 / 4, stride 2, the role-swapped
    transposed form, ragged row chunks, dbias NULL and non-NULL; += from a non-zero start everywhere."""
    layer, B, H, T = case
    out_pad = 1 if layer[0] == 'tconv' and T == 256 else 0
    _wgrad('wgrad generic', B, layer, H, T, out_pad=out_pad, with_bias=layer[0] == 'conv', seed=H + T)
    if layer[0] == 'conv':
        _wgrad('wgrad generic', B, layer, H, T, with_bias=False, seed=H + T + 1)


# ---- 6. channel sums -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('inner', [1, 3, 65, 4 * 64 + 1])
@pytest.mark.parametrize('B,C', [(1, 1), (3, 8), (2, 31)])
def test_channel_sums(B, C, inner):
    """out[c] += sum over (b, inner) onto a non-zero out: the atomic form and the fixed-order form with its 2 C + 2048 floats of scratch."""
    lib, st = _api()
    gen = torch.Generator().manual_seed(B * 1000 + C * 10 + inner)
    x, prev = _pm(gen, B, C, inner), _pm(gen, C)
    want = prev.double() + x.double().sum((0, 2))
    bar = (B * inner + 1) * U * (x.double().abs().sum((0, 2)) + prev.double().abs())
    for entry in ('tt_channel_sum', 'tt_channel_sum_ws'):
        A = _Arena()
        A.inp('x', x)
        A.acc('out', prev)
        if entry.endswith('_ws'):
            A.scratch('ws', 2 * C + 2048)
        A.build()
        if entry.endswith('_ws'):
            rc = lib.tt_channel_sum_ws(A.ptr('x'), A.ptr('out'), B, C, inner, A.ptr('ws'), st)
        else:
            rc = lib.tt_channel_sum(A.ptr('x'), A.ptr('out'), B, C, inner, st)
        what = '%s B %d C %d inner %d' % (entry, B, C, inner)
        assert rc == 0, what
        A.verify(what)
        _hold(entry[3:], A.get('out'), want, bar, what)
