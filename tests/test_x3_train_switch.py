"""CPU tests of the switch of the split-operand training route (ops.X3_TRAIN, TTRAP_X3_TRAIN): off by default, read from the environment
once, defined in the package alone (the family modules read it through the package), and -- without a GPU -- never taken."""

import os
import subprocess
import sys

import torch

from timbre_trap.framework import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'timbre-trap_amd')
CODE = 'from timbre_trap.framework import ops; print(repr((ops.X3_TRAIN, ops.X3_TRAIN_CHANNELS, ops.X3_CHANNELS)))'


def _child(**env_extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith('TTRAP_')}
    env['PYTHONPATH'] = PKG
    env.update(env_extra)
    return eval(subprocess.check_output([sys.executable, '-c', CODE], env=env, text=True))


def test_off_with_the_variable_unset():
    assert _child() == (False, (16, 32), (16, 32))


def test_on_with_the_variable_set():
    assert _child(TTRAP_X3_TRAIN='1')[0] is True
    assert _child(TTRAP_X3_TRAIN='0')[0] is False


def test_the_switch_lives_in_the_package_alone():
    assert 'X3_TRAIN' in vars(ops) and 'X3_TRAIN_CHANNELS' in vars(ops)
    for family in ('_common', 'fp32', 'cl16', 'level16', 'skip', 'x3', 'losses'):
        mod = getattr(ops, family)
        assert 'X3_TRAIN' not in vars(mod) and 'X3_TRAIN_CHANNELS' not in vars(mod), family
    assert set(ops.X3_TRAIN_CHANNELS) <= set(ops.X3_CHANNELS)


def test_the_function_is_registered_nowhere():
    """Its launches are timed one by one inside (like x3_level): neither the event-log nor the loss-scale decorator."""
    assert issubclass(ops.X3LevelTrainFn, torch.autograd.Function)
    assert '_tt_event' not in vars(ops.X3LevelTrainFn) and not vars(ops.X3LevelTrainFn).get('_tt_loss_scaled')


def test_the_route_needs_the_switch_fp32_mode_and_grad(monkeypatch):
    class Conv:
        def __init__(self, shape):
            self.weight = torch.zeros(shape, requires_grad=True)
            self.bias = torch.zeros(shape[0], requires_grad=True)

    class Block:
        def __init__(self, C, d):
            self.conv1, self.conv2, self.dilation = [Conv((C, C, 3, 3))], [Conv((C, C, 1, 1))], d

    class OnGpu:
        """Stands in for a CUDA tensor: x3_training looks at the shape, the dtype and where the tensor lives."""
        is_cuda, dtype, requires_grad = True, torch.float32, False

        def __init__(self, *shape):
            self.shape = shape

        def dim(self):
            return len(self.shape)

        def size(self, i):
            return self.shape[i]

    blocks = [Block(16, d) for d in (1, 2, 3)]
    x = OnGpu(2, 16, 9, 40)
    monkeypatch.setattr(ops, 'PRECISION', 'fp32')
    monkeypatch.setattr(ops, 'X3_TRAIN', False)
    assert not ops.x3_training(x, blocks)
    monkeypatch.setattr(ops, 'X3_TRAIN', True)
    assert ops.x3_training(x, blocks)
    with torch.no_grad():
        assert not ops.x3_training(x, blocks)
    monkeypatch.setattr(ops, 'PRECISION', 'bf16')
    assert not ops.x3_training(x, blocks)
    monkeypatch.setattr(ops, 'PRECISION', 'fp32')
    monkeypatch.setattr(ops, 'WIDE_STORAGE', 'bf16')
    assert not ops.x3_training(x, blocks)
    monkeypatch.setattr(ops, 'WIDE_STORAGE', '')
    assert not ops.x3_training(OnGpu(2, 8, 9, 40), [Block(8, d) for d in (1, 2, 3)])
    assert not ops.x3_training(x, [Block(16, 4)])
    monkeypatch.setattr(ops, 'X3_TRAIN_CHANNELS', (32,))
    assert not ops.x3_training(x, blocks)
    assert not ops.x3_training(torch.zeros(2, 16, 9, 40), blocks)          # a CPU tensor: never
