"""
CPU-only tests of the surface of the package timbre_trap.framework.ops (formerly the single file ops.py): every name its callers use is
an attribute of the package, the switches live in the package alone and are read at call time, every family module can be imported first,
and the Functions registered for the loss-scaled backward and for bench.py's event log are the ones that were registered before the split.
"""

import glob
import os
import re
import subprocess
import sys

import pytest
import torch

from timbre_trap.framework import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'timbre-trap_amd')
FAMILIES = ('_common', 'fp32', 'cl16', 'level16', 'skip', 'x3', 'losses')

# switch -> (environment variable, value with the variable unset)
SWITCHES = {
    'FUSED_RESBLOCK': ('TTRAP_FUSED', True), 'SAVE_HIDDEN': ('TTRAP_SAVE_HIDDEN', True), 'PRECISION': ('TTRAP_PRECISION', 'auto'),
    'WIDE_STORAGE': ('TTRAP_WIDE_STORAGE', ''), 'FP16_LOSS_SCALE': ('TTRAP_FP16_LOSS_SCALE', 4096.0),
    'RECOMPUTE_CHANNELS': ('TTRAP_LEVEL_RECOMPUTE', ()), 'LEVEL_BWD': ('TTRAP_LEVEL_BWD', True), 'PREGATE': ('TTRAP_PREGATE', True),
    'SKIP_FUSED': ('TTRAP_SKIP_FUSED', True), 'SKIP_DEFER': ('TTRAP_SKIP_DEFER', True), 'SKIP_RIDE': ('TTRAP_SKIP_RIDE', True),
    'SKIP_FOLD': ('TTRAP_SKIP_FOLD', True), 'X3_INFER': ('TTRAP_X3_INFER', True), 'X3N_INFER': ('TTRAP_X3N_INFER', True),
    'LOSS_FUSED': ('TTRAP_LOSS_FUSED', True),
}
TABLES = {'FUSED_CHANNELS': (4, 8, 16, 32), 'WIDE_CHANNELS': (4, 8, 16, 32), 'CL16_CHANNELS': (4, 8, 16, 32, 64), 'X3_CHANNELS': (16, 32),
          'X3N_CHANNELS': (4, 8), 'X3_LATENT_SHAPES': ((64, 128), (32, 32)), 'X3_SHAPES': {}}

# The registration lists at the bottom of ops.py before the split: event name and shape tags per class, and the loss-scaled classes.
EVENTS = {
    'ConvFn': 'conv', 'ResBlockFn': 'rb', 'WideLevelFn': 'widelevel', 'ConvIn16Fn': 'edge16', 'ConvOut16Fn': 'edge16', 'ConvOut16PairFn': 'edge16',
    'ConvIn16x1Fn': 'edge16', 'ConvOut16x1Fn': 'edge16', 'ConvOut16x1PairFn': 'edge16', 'Level16Fn': 'widelevel', 'Level16JoinFn': 'widelevel',
    'SConv16Fn': 'sconv16', 'TConv16Fn': 'tconv16', 'ToCL16Fn': 'tocl16', 'ToPlanar32Fn': 'toplanar', 'StridedConvFn': 'sconv',
    'TransposedConvFn': 'tconv', 'SkipJoin16Fn': 'skipjoin16', 'LatEnc16Fn': 'latenc16', 'LatDec16Fn': 'latdec16', 'LatentEncodeFn': 'latenc',
    'LatentDecodeFn': 'latdec', 'SqDiffLossFn': 'sqdiff', 'SqDiff2Fn': 'sqdiff2', 'ActivationsFn': 'act', 'Activations1Fn': 'act1',
    'TranscriptionLossFn': 'trn',
}
LOSS_SCALED = {'Level16Fn', 'Level16JoinFn', 'WideLevelFn', 'SConv16Fn', 'TConv16Fn', 'LatEnc16Fn', 'LatDec16Fn', 'SkipJoin16Fn'}


def _functions():
    return {n: c for n, c in vars(ops).items() if isinstance(c, type) and issubclass(c, torch.autograd.Function)}


def _callers():
    files = [os.path.join(ROOT, 'bench.py')] + glob.glob(os.path.join(ROOT, 'tests', '*.py'))
    files += glob.glob(os.path.join(ROOT, 'tools', '**', '*.py'), recursive=True)
    files += [os.path.join(PKG, 'timbre_trap', 'framework', n + '.py') for n in ('modules', 'objectives', 'cqtwrapper')]
    return sorted(files)


def test_every_name_the_callers_use_is_an_attribute_of_the_package():
    missing, seen = [], set()
    for path in _callers():
        with open(path) as f:
            for name in re.findall(r'\bops\.([A-Za-z_]\w*)', f.read()):
                seen.add(name)
                if name != 'py' and not hasattr(ops, name):                  # 'py': the prose that still says "ops.py"
                    missing.append((os.path.relpath(path, ROOT), name))
    assert not missing, missing
    assert len(_callers()) > 40 and len(seen) > 50, (len(_callers()), len(seen))          # the scan really read the callers


def test_switches_live_in_the_package_alone():
    families = [getattr(ops, m) for m in FAMILIES]
    for name in list(SWITCHES) + list(TABLES):
        assert name in vars(ops), name
        for mod in families:
            assert name not in vars(mod), '%s binds a copy of ops.%s' % (mod.__name__, name)
    for name, want in TABLES.items():
        assert getattr(ops, name) == want, name


def test_switch_defaults_and_environment_variables():
    code = 'from timbre_trap.framework import ops; print(repr({n: getattr(ops, n) for n in %r}))' % (sorted(SWITCHES),)
    env = {k: v for k, v in os.environ.items() if not k.startswith('TTRAP_')}
    env['PYTHONPATH'] = PKG
    assert eval(subprocess.check_output([sys.executable, '-c', code], env=env, text=True)) == {n: d for n, (_, d) in SWITCHES.items()}
    flipped = {'PRECISION': 'bf16x3', 'WIDE_STORAGE': 'fp16', 'FP16_LOSS_SCALE': 256.0, 'RECOMPUTE_CHANNELS': (16, 32)}
    for n, (var, default) in SWITCHES.items():
        env[var] = {'PRECISION': 'bf16x3', 'WIDE_STORAGE': 'fp16', 'FP16_LOSS_SCALE': '256', 'RECOMPUTE_CHANNELS': '1'}.get(n, '0')
    want = {n: flipped.get(n, False) for n in SWITCHES}
    assert eval(subprocess.check_output([sys.executable, '-c', code], env=env, text=True)) == want


def test_assigning_a_switch_on_the_package_reaches_the_code_that_reads_it(monkeypatch):
    h, b = torch.float16, torch.bfloat16
    for p in ('fp32', 'bf16', 'fp16', 'bf16x3'):
        monkeypatch.setattr(ops, 'PRECISION', p)
        monkeypatch.setattr(ops, 'WIDE_STORAGE', '')
        assert ops.precision() == p and ops.wide_storage() == (p if p in ('bf16', 'fp16') else 'fp32')
        assert ops.cl16_mode() == (p in ('bf16', 'fp16')) and ops.cl16_dtype() == (h if p == 'fp16' else b)
    monkeypatch.setattr(ops, 'PRECISION', 'fp32')
    monkeypatch.setattr(ops, 'WIDE_STORAGE', 'fp16')
    assert ops.wide_storage() == 'fp16' and ops.cl16_mode() and ops.cl16_dtype() == h
    monkeypatch.setattr(ops, 'WIDE_STORAGE', 'int8')
    with pytest.raises(ValueError):
        ops.wide_storage()
    monkeypatch.setattr(ops, 'PRECISION', 'auto')
    monkeypatch.setattr(ops, 'WIDE_STORAGE', '')
    assert ops.precision() == 'fp32' and not ops.cl16_mode()                     # no autocast region
    # cl16.gate_link reads ops.PREGATE
    monkeypatch.setattr(ops, 'PREGATE', False)
    assert ops.gate_link() is None
    monkeypatch.setattr(ops, 'PREGATE', True)
    assert isinstance(ops.gate_link(), ops.GateLink)
    # _common.loss_scaled reads ops.loss_scale, which reads ops.FP16_LOSS_SCALE
    monkeypatch.setattr(ops, 'FP16_LOSS_SCALE', 8.0)
    assert ops.loss_scale(h) == 8.0 and ops.loss_scale(b) == 1.0 and ops.loss_scaled(h).s == 8.0 and ops.loss_scaled(b).s == 1.0
    monkeypatch.setattr(ops, 'FP16_LOSS_SCALE', 1.0)
    assert ops.loss_scale(h) == 1.0 and ops.loss_scaled(h).s == 1.0
    monkeypatch.setattr(ops, 'FP16_LOSS_SCALE', 3.0)
    with pytest.raises(ValueError):
        ops.loss_scale(h)
    # x3.x3_inference reads ops.X3_INFER and the mode functions
    with torch.no_grad():
        assert ops.x3_inference()
        with ops.x3_disabled():
            assert not ops.x3_inference()
        assert ops.x3_inference() and not ops.x3_chain() and not ops.x3_vouched()
        with ops.x3_chain_scope(), ops.x3_vouched_scope():
            assert ops.x3_chain() and ops.x3_vouched()
        with ops.x3_chain_scope(False):
            assert not ops.x3_chain()
        monkeypatch.setattr(ops, 'X3_INFER', False)
        assert not ops.x3_inference()
        monkeypatch.setattr(ops, 'X3_INFER', True)
        monkeypatch.setattr(ops, 'PRECISION', 'bf16')
        assert not ops.x3_inference()
    assert not ops.x3_inference()                                                # grad enabled


@pytest.mark.parametrize('family', FAMILIES)
def test_a_family_module_can_be_imported_first(family):
    code = 'import timbre_trap.framework.ops.%s as m; from timbre_trap.framework import ops; assert m is ops.%s and ops.residual_level' % (family, family)
    subprocess.check_call([sys.executable, '-c', code], env=dict(os.environ, PYTHONPATH=PKG))


def test_registered_functions_are_the_ones_registered_before_the_split():
    fns = _functions()
    assert {n: c._tt_event for n, c in fns.items() if '_tt_event' in vars(c)} == EVENTS
    assert {n for n, c in fns.items() if vars(c).get('_tt_loss_scaled')} == LOSS_SCALED
    # the six edge convolutions are classes of their own (routes are counted per class)
    edges = [fns[n] for n in ('ConvIn16Fn', 'ConvIn16x1Fn', 'ConvOut16Fn', 'ConvOut16PairFn', 'ConvOut16x1Fn', 'ConvOut16x1PairFn')]
    assert all(c.__bases__ == (torch.autograd.Function,) for c in edges)


def test_event_keys_of_the_edge_convolutions():
    """The shape tags bench.py's ``families`` reads for 'edge16': in / out for the two-plane edges, in1 / out1 for the one-plane ones."""
    import timbre_trap._hip as _hip
    tags = {'ConvIn16Fn': 'in', 'ConvIn16x1Fn': 'in1', 'ConvOut16Fn': 'out', 'ConvOut16PairFn': 'out', 'ConvOut16x1Fn': 'out1', 'ConvOut16x1PairFn': 'out1'}
    seen = []

    class Stop(Exception):
        pass

    class Timed:
        def __init__(self, key, clips=None):
            seen.append(key)

        def __enter__(self):
            raise Stop

        def __exit__(self, *exc):
            return False

    class Ctx:
        pass
    log, timed = _hip.EVENT_LOG, _hip.timed
    _hip.EVENT_LOG, _hip.timed = {}, Timed
    try:
        for name, tag in tags.items():
            with pytest.raises(Stop):
                getattr(ops, name).forward(Ctx(), torch.zeros(2, 4, 2, 2), None, None)
            assert seen[-1] == 'edge16_fwd_' + tag, (name, seen[-1])
    finally:
        _hip.EVENT_LOG, _hip.timed = log, timed
