"""
bench.py's plain run and --dump-outputs: the headline line alone (everything else behind --full), and the outputs of the last timed
step written as float32 .npy files within the size limit -- the same bits from two runs with the same arguments.
"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'steps', 'warmup', 'n_gpus')


def test_write_outputs_keeps_small_sets_whole_and_samples_large_ones(tmp_path, monkeypatch):
    import bench
    small = {'a': torch.arange(6, dtype=torch.float32).reshape(2, 3), 'b': torch.ones(1, dtype=torch.float64), 'c': torch.ones(4, dtype=torch.bfloat16)}
    bench.write_outputs(str(tmp_path / 'small'), small)
    a, b, c = (np.load(str(tmp_path / 'small' / (n + '.npy'))) for n in 'abc')
    assert a.dtype == np.float32 and a.shape == (2, 3) and (a == np.arange(6).reshape(2, 3)).all()
    assert b.dtype == np.float64 and c.dtype == np.float32 and (c == 1).all()

    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 4000)              # 1000 float32 in all, 500 per array
    big = {'x': torch.arange(3000, dtype=torch.float32), 'y': torch.arange(100, dtype=torch.float32)}
    for run in ('one', 'two'):
        bench.write_outputs(str(tmp_path / run), big)
    x1, x2, y = np.load(str(tmp_path / 'one' / 'x.npy')), np.load(str(tmp_path / 'two' / 'x.npy')), np.load(str(tmp_path / 'one' / 'y.npy'))
    assert x1.shape == (500,) and (x1 == x2).all()                          # the same seeded sample every run
    assert (np.diff(x1) > 0).all() and x1.min() >= 0 and x1.max() < 3000     # distinct elements, in index order
    assert (y == np.arange(100)).all()                                      # within its share: whole


def _run(tmp_path, *argv):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(argv), capture_output=True, text=True, timeout=900,
                         env={k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'TTRAP_DIST_BACKEND')})
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_prints_the_headline_and_dumps_the_last_step(tmp_path):
    d = tmp_path / 'train'
    line = _run(tmp_path, '--gpus', '1', '--steps', '3', '--warmup', '1', '--batch', '2', '--dump-outputs', str(d))
    assert all(k in line for k in HEADLINE) and line['steps'] == 3 and line['warmup'] == 1 and line['ms_per_step'] > 0
    assert line['unit'] == 'audio-seconds/s' and line['higher_is_better'] is True and line['dtype'] == 'bf16'
    assert abs(line['value'] - 2 * 3.0 / (line['ms_per_step'] * 1e-3)) <= 1e-6 * line['value']
    assert not any(k in line for k in ('roofline', 'families', 'host', 'cpu_baseline', 'inference_config1'))   # --full only
    files = sorted(os.listdir(str(d)))
    assert files == sorted(['loss_total.npy', 'loss_reconstruction.npy', 'loss_transcription.npy', 'loss_consistency_spectral.npy',
                            'loss_consistency_score.npy', 'flat_param.npy', 'flat_grad.npy'])
    arrays = {f: np.load(str(d / f)) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(os.path.getsize(str(d / f)) for f in files) < 64 * 10 ** 6
    assert abs(float(arrays['loss_total.npy'][0]) - line['final_loss']) <= 1e-6 * abs(line['final_loss'])
    parts = sum(float(arrays[f][0]) for f in files if f.startswith('loss_') and f != 'loss_total.npy')
    assert abs(parts - line['final_loss']) <= 1e-4 * abs(line['final_loss'])
    assert arrays['flat_param.npy'].shape == arrays['flat_grad.npy'].shape and float(np.abs(arrays['flat_grad.npy']).sum()) > 0
    # the same arguments in a fresh process: the same inputs, and the timed path computes the same bits from them
    again = _run(tmp_path, '--gpus', '1', '--steps', '3', '--warmup', '1', '--batch', '2', '--dump-outputs', str(tmp_path / 'train2'))
    assert again['final_loss'] == line['final_loss']
    for f in files:
        assert np.array_equal(np.load(str(tmp_path / 'train2' / f)), arrays[f]), f

    d = tmp_path / 'infer'
    line = _run(tmp_path, '--gpus', '1', '--mode', 'infer', '--steps', '2', '--warmup', '1', '--batch', '2', '--dump-outputs', str(d))
    assert all(k in line for k in HEADLINE) and line['steps'] == 2
    act, rec = np.load(str(d / 'activations.npy')), np.load(str(d / 'reconstruction.npy'))
    assert [list(act.shape), list(rec.shape)] == line['out_shapes'] and act.dtype == rec.dtype == np.float32
    assert np.isfinite(act).all() and np.isfinite(rec).all()
