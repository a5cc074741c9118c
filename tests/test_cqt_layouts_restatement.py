"""
CPU side of tests/test_gpu_cqt_abi_parity.py: the plans of nsgt_plan.build_plan for every layout of tests/cqt_abi_ref.py against the oracle's
tables, the table sizes include/ttrap.h states, the two layouts build_plan refuses, the scratch sizes against the carve written out in
cqt_abi_ref.scratch_carve (the library is loaded, no device is touched), and every constant K of cqt_abi_ref against its definition: 4 times
what the float32 restatement of the oracle reaches, re-measured here and held to K / 4 within 25 % (the convention of
test_constants_follow_the_restatement in tests/test_gpu_cqt_parity.py).
"""

import ctypes

import numpy as np
import pytest

import cqt_abi_ref as R

ALL = tuple(R.FAST) + tuple(R.ANY)


@pytest.mark.parametrize('layout', ALL, ids=str)
def test_plan_tables_equal_the_oracle(layout):
    p, tab = R.plan(layout), R.tables(layout)
    F, M = (R.FAST if layout in R.FAST else R.ANY)[layout]
    assert (p['n_bins'], p['M'], p['N']) == (F, M, layout[2]) == (tab['n_bins'], tab['max_window_length'], tab['block_length'])
    for name in ('lengths', 'positions', 'spec_index', 'pad', 'win_off'):
        assert np.array_equal(p[name], tab[name]), name
    assert np.array_equal(p['window'], tab['window']) and np.allclose(p['dual'], tab['dual'], rtol=1e-15, atol=0)
    assert p['fast'] == (layout[2] == 66150 and M == 1024) == (layout in R.FAST)
    if not p['fast']:
        assert p['P'] >= 2 * p['N'] - 1 and p['P'] & (p['P'] - 1) == 0 and p['P'] < 4 * p['N']
    assert p['sum_len'] == int(tab['lengths'].sum())


def test_the_layouts_are_what_they_are_in_the_set_for():
    """the properties the GPU file relies on: F % 4 of the fast layouts, the one-sample windows, P = 2 N at N = 4096, the only M > 1024"""
    assert [F % 4 for F, _ in R.FAST.values()] == [1, 3, 0, 0]
    assert int((R.tables((9, 61, 66150))['lengths'] == 1).sum()) == 2
    assert int(R.tables((7, 60, 66150))['spec_index'].min()) > 64 * 3
    assert int((R.tables((9, 120, 2205))['lengths'] == 1).sum()) == 710
    assert R.plan((9, 59, 4096))['P'] == 2 * 4096 and R.plan((4, 9, 1001))['N'] % 2 == 1
    assert [l for l in R.ANY if R.ANY[l][1] > 1024] == [(9, 24, 66150)]


@pytest.mark.parametrize('layout', R.REFUSED_LAYOUTS, ids=str)
def test_build_plan_refuses_a_window_outside_the_half_spectrum(layout):
    from timbre_trap.framework import nsgt_plan
    with pytest.raises(ValueError, match='window leaves the open positive half-spectrum'):
        nsgt_plan.build_plan(layout[0], layout[1], R.SR, layout[2])


@pytest.mark.parametrize('layout', ALL, ids=str)
def test_every_table_fits_its_header_size(layout):
    """plan_tensors asserts table length == header size; here also what the kernels index with stays inside those sizes"""
    p, t = R.plan(layout), R.plan_tensors(layout)
    F, S, N = p['n_bins'], p['sum_len'], p['N']
    assert set(t) == set(R.FAST_TABLES if p['fast'] else R.ANY_TABLES)
    bt = t['bin_tab'].view(F, 4).numpy()
    assert (bt[:, 0] > 0).all() and (bt[:, 0] + bt[:, 2] <= N // 2).all()            # spec_start .. + length inside the half spectrum
    assert (bt[:, 1] >= 0).all() and (bt[:, 1] + bt[:, 2] <= p['M']).all()             # pad + length inside the M frames
    assert (bt[:, 3] >= 0).all() and (bt[:, 3] + bt[:, 2] <= S).all() and int(bt[-1, 3] + bt[-1, 2]) == S
    go, gi = t['gat_off'].numpy(), t['gat_idx'].numpy()
    assert go[0] == 0 and go[-1] == S and (np.diff(go) >= 0).all() and go.size == N // 2 + 2
    assert np.array_equal(np.sort(gi), np.arange(S))
    if not p['fast']:
        pb = t['pos_bin'].numpy()
        assert pb.min() == 0 and pb.max() == F - 1 and (np.diff(pb) >= 0).all()


def test_scratch_sizes_follow_the_carve():
    from timbre_trap import _hip
    lib = _hip.lib()
    for layout in ALL:
        p = R.plan(layout)
        F, S = p['n_bins'], p['sum_len']
        for Q in (1, 2, 4, 6):
            if p['fast']:
                assert lib.tt_cqt_scratch_bytes(Q, F, S) == R.scratch_carve(layout, Q)
                assert lib.tt_cqt_griffin_lim_scratch_bytes(Q, F, S) == R.scratch_carve(layout, Q, griffin_lim=True)
            else:
                ps = _hip.CqtGenericPlan()
                for name in R.ANY_TABLES:
                    setattr(ps, name, 16)                                              # any non-NULL value: the size needs no table
                ps.n_bins, ps.sum_len, ps.N, ps.M, ps.P = F, S, p['N'], p['M'], p['P']
                assert lib.tt_cqt_generic_scratch_bytes(ctypes.byref(ps), Q) == R.scratch_carve(layout, Q)
                assert lib.tt_cqt_generic_scratch_bytes(ctypes.byref(ps), 0) == 0 == lib.tt_cqt_generic_scratch_bytes(ctypes.byref(ps), -3)
                ps.M = p['M'] + 1
                assert lib.tt_cqt_generic_scratch_bytes(ctypes.byref(ps), Q) == -1     # a plan the entry points refuse
    for n in (0, -1):
        assert lib.tt_cqt_scratch_bytes(n, 549, 60000) == 0 and lib.tt_cqt_griffin_lim_scratch_bytes(n, 549, 60000) == 0
    assert lib.tt_cqt_scratch_bytes(2, 0, 60000) == 0 and lib.tt_cqt_scratch_bytes(2, 549, 0) == 0
    assert lib.tt_cqt_generic_scratch_bytes(None, 2) == -1


def test_every_constant_is_listed():
    assert set(R.K) == set(R.constant_keys())


@pytest.mark.parametrize('key', R.constant_keys(), ids=lambda k: '-'.join(k))
def test_constants_follow_the_restatement(key):
    """K / 4 is what torch.fft in complex64 reaches over the layouts of the path, re-measured here: a literal that drifted from its
    definition (inputs, tables or bars changed without re-measuring) fails."""
    k, measured = R.K[key]
    r = R.restatement(*key)
    print('float32 restatement, %-40s worst ratio %.4g (literal %.4g, K %.4g)' % (' '.join(key), r, measured, k))
    assert 4 * measured <= k <= 4 * measured * 1.01
    assert r <= k / 4 * 1.25, (r, k)
