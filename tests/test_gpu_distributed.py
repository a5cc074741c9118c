"""
N > 1 train-step path on the GPU box: two ranks (gloo backend, so that both can share the single GPU of the test box; the
real launch uses RCCL, one GPU per rank) run FusedAdamW steps with ONE all-reduce of the flat gradient and must end with
identical parameters, equal to a single process that sees the concatenated batch (mean of rank means == global mean).
"""

import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = textwrap.dedent('''
    import os, sys
    sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'timbre-trap_amd'))
    import torch
    from timbre_trap.framework import TimbreTrap, compute_reconstruction_loss
    from timbre_trap.utils import FusedAdamW, GradientSync, init_process_group_from_env
    from timbre_trap.utils.distributed import broadcast_parameters
    rank, world, _ = init_process_group_from_env()
    torch.cuda.set_device(0)
    torch.manual_seed(7 + rank)                      # different initial weights per rank: the broadcast must fix that
    amp = os.environ.get('TT_TEST_AUTOCAST') == '1'   # the bench's configuration: bf16 channels-last path under autocast, mc 2
    skip = os.environ.get('TT_TEST_SKIP') == '1'      # the configs[4] model: fused / riding skip joins, their weights' gradient in the flat buffer
    model = TimbreTrap(sample_rate=22050, n_octaves=9, bins_per_octave=60, latent_size=128 if amp else 32,
                       model_complexity=2 if amp else 1, skip_connections=skip).cuda()
    opt = FusedAdamW(model.parameters(), lr=1e-3, max_norm=10.0)
    broadcast_parameters(opt.flat_param)
    g = torch.Generator().manual_seed(123)
    audio_all = torch.rand(2, 1, 66150, generator=g) * 2 - 1
    audio = audio_all[rank:rank + 1].cuda() if world > 1 else audio_all.cuda()
    sync = GradientSync(world)
    coeffs = model.sliCQ(audio)
    for _ in range(2):
        with torch.autocast(device_type='cuda', dtype=torch.bfloat16, enabled=amp):
            rec = model(audio, False)[0]
            loss = compute_reconstruction_loss(rec, coeffs)
            if os.environ.get('TT_TEST_MODEL_ZERO') == '1':
                model.zero_grad()                # drops every .grad view: autograd then installs fresh tensors ...
            else:
                opt.zero_grad()
            loss.backward()
        if world > 1:
            sync.start(opt)                      # ... which must be back in the flat buffer BEFORE it is averaged; asynchronous all-reduce ...
            coeffs = model.sliCQ(audio)          # ... with the next step's transform issued meanwhile (bench.py's overlap)
            sync.finish()
        else:
            coeffs = model.sliCQ(audio)
        opt.step()
    print('RESULT %%d %%.9e %%.9e' %% (rank, float(opt.flat_param.double().sum()), float(opt.flat_param.double().abs().sum())))
''') % (ROOT, ROOT)


def _run(rank, world, port, amp=False, model_zero=False, skip=False):
    env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
               TTRAP_DIST_BACKEND='gloo', TT_TEST_AUTOCAST='1' if amp else '0', TT_TEST_MODEL_ZERO='1' if model_zero else '0',
               TT_TEST_SKIP='1' if skip else '0')
    return subprocess.Popen([sys.executable, '-c', SCRIPT], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _result(proc):
    out, _ = proc.communicate(timeout=600)
    assert proc.returncode == 0, out[-2000:]
    line = [l for l in out.splitlines() if l.startswith('RESULT')][-1].split()
    return float(line[2]), float(line[3])


@pytest.mark.gpu
@pytest.mark.parametrize('amp,skip', [(False, False), (True, False), (True, True)], ids=['fp32', 'autocast-bf16', 'autocast-bf16-skip-connections'])
def test_two_ranks_match_single_process_global_batch(amp, skip):
    procs = [_run(r, 2, 29541 + 4 * amp + 8 * skip, amp, skip=skip) for r in range(2)]
    res = [_result(p) for p in procs]
    assert res[0] == res[1]                                       # ranks end with bit-identical parameters
    single = _result(_run(0, 1, 29542 + 4 * amp + 8 * skip, amp, skip=skip))
    tol = 1e-4 if amp else 1e-5                                   # bf16 step: the same products summed in another order, then Adam
    assert abs(res[0][0] - single[0]) <= tol * abs(single[1]) and abs(res[0][1] - single[1]) <= tol * abs(single[1])


@pytest.mark.gpu
def test_two_ranks_after_model_zero_grad():
    """``model.zero_grad()`` between steps drops the gradient views of the flat buffer: autograd then deposits this step's
    gradient in fresh tensors, and the collective must average THAT (GradientSync.start(opt) re-attaches first), not the stale
    slot -- otherwise the ranks diverge silently (round-2 advisor finding)."""
    procs = [_run(r, 2, 29561, False, model_zero=True) for r in range(2)]
    res = [_result(p) for p in procs]
    assert res[0] == res[1]
    single = _result(_run(0, 1, 29562, False, model_zero=True))
    assert abs(res[0][0] - single[0]) <= 1e-5 * abs(single[1]) and abs(res[0][1] - single[1]) <= 1e-5 * abs(single[1])
    # and the same trajectory as with opt.zero_grad()
    plain = _result(_run(0, 1, 29563, False, model_zero=False))
    assert abs(single[0] - plain[0]) <= 1e-5 * abs(plain[1])


NCCL_SCRIPT = textwrap.dedent('''
    import os, sys
    sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'timbre-trap_amd'))
    import torch
    from timbre_trap.utils import GradientSync, init_process_group_from_env
    rank, world, local = init_process_group_from_env()           # backend 'nccl' = RCCL, one GPU per rank
    torch.cuda.set_device(local)
    g = torch.arange(614490, dtype=torch.float32, device='cuda') * (rank + 1)
    sync = GradientSync(world)
    sync.start(g)
    busy = torch.ones(1 << 20, device='cuda').cumsum(0)          # compute stream stays busy while RCCL runs on its own stream
    sync.finish()
    want = torch.arange(614490, dtype=torch.float32, device='cuda') * (sum(range(1, world + 1)) / world)
    assert torch.allclose(g, want, rtol=1e-6), float((g - want).abs().max())
    print('NCCL_OK', rank)
''') % (ROOT, ROOT)


@pytest.mark.gpu
def test_rccl_allreduce_smoke_when_two_gpus_present(tmp_path):
    """The 'nccl' (= RCCL over xGMI) branch, one process per GPU through torchrun; skipped on a 1-GPU box."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip('needs >= 2 GPUs (the test box has one): the RCCL branch runs in the driver\'s multi-GPU bench')
    n = min(torch.cuda.device_count(), 8)
    path = str(tmp_path / 'nccl_smoke.py')
    with open(path, 'w') as f:
        f.write(NCCL_SCRIPT)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.pop('TTRAP_DIST_BACKEND', None)
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n), '--master-addr',
                          '127.0.0.1', '--master-port', '29551', path], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.count('NCCL_OK') == n


@pytest.mark.gpu
def test_rccl_single_rank_next_to_the_hip_library():
    """
    RCCL on the 1-GPU box (round-4 verdict item 5): `bench.py` under `torch.distributed.run --nproc-per-node 1` with backend 'nccl' and
    TTRAP_FORCE_DIST=1, which keeps the whole N > 1 path alive at world size 1 -- process group, broadcast of the flat parameters,
    GradientSync's asynchronous all-reduce on RCCL's own stream with the next batch's CQT issued meanwhile, the stream wait, the
    stand-alone all-reduce timing.  Proves that ProcessGroupNCCL initialises beside the ctypes-loaded libttrap_hip.so and torch's
    bundled HIP runtime (three users of one runtime), that the communicator comes up with HSA_ENABLE_IPC_MODE_LEGACY=0, and that
    `work.wait()` orders the optimizer step after the collective: the loss after the same steps must equal the plain one-process run.
    """
    import json
    import socket
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', TTRAP_FORCE_DIST='1')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT', 'TTRAP_DIST_BACKEND'):
        env.pop(k, None)
    with socket.socket() as s_:
        s_.bind(('127.0.0.1', 0))
        port = s_.getsockname()[1]
    argv = ['--gpus', '1', '--steps', '3', '--warmup', '1', '--batch', '2', '--no-cpu-baseline', '--full']
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1', '--master-addr', '127.0.0.1',
                          '--master-port', str(port), os.path.join(ROOT, 'bench.py')] + argv, env=env, capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    assert line['n_gpus'] == 1 and line['config']['parallelism'] == 'dp1'
    assert line['overlap'] is not None and line['overlap']['backend'] == 'nccl', line['overlap']
    assert line['allreduce_ms'] is not None and 0.0 < line['allreduce_ms'] < 50.0
    # RCCL does not block the host: the compute stream's wait after the CQT is a stream wait of (at most) the collective's length
    assert line['overlap']['wait_for_collective_after_cqt_ms'] < 50.0
    plain = _bench(*argv)
    assert plain.returncode == 0, plain.stdout[-2000:] + plain.stderr[-3000:]
    ref = json.loads([l for l in plain.stdout.splitlines() if l.startswith('{')][0])
    assert ref['overlap'] is None and ref['allreduce_ms'] is None
    assert abs(line['final_loss'] - ref['final_loss']) <= 1e-4 * abs(ref['final_loss']), (line['final_loss'], ref['final_loss'])


def _bench(*argv, **env_over):
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT', 'TTRAP_DIST_BACKEND'):
        env.pop(k, None)
    env.update(env_over)
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(argv), env=env, capture_output=True, text=True,
                          timeout=900)


@pytest.mark.gpu
def test_two_host_cores_keep_up_with_the_gpu_step():
    """
    The one-GPU proxy for eight ranks sharing a host (round-5 verdict, weak #12 / next #5; SURVEY.md section 8e: ">= 6.5x hinges on ...
    per-step host syncs"): the bench's 64-clip train step enqueues ~600 launches from Python + autograd threads per ~50 ms of GPU time.
    `bench.py --cores 2` pins the process to two host cores before torch is imported (a 16-core host / 8 ranks); its ms_per_step must stay
    within 5 % of the unrestricted run's, and in both the host must finish enqueueing well before the GPU finishes computing.
    """
    import json
    argv = ['--full', '--timed-only', '--steps', '8', '--warmup', '3']
    runs = {}
    for name, extra in (('all cores', []), ('two cores', ['--cores', '2'])):
        out = _bench(*(extra + argv))
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
        runs[name] = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][0])
    full, capped = runs['all cores'], runs['two cores']
    assert capped['host']['host_cores'] == 2 and full['host']['host_cores'] >= 2
    print('ms_per_step %.2f (all %d cores) / %.2f (2 cores); host enqueue %.2f / %.2f ms per step; host_over_gpu %.2f / %.2f'
          % (full['ms_per_step'], full['host']['host_cores'], capped['ms_per_step'], full['host']['host_enqueue_ms'], capped['host']['host_enqueue_ms'],
             full['host']['host_over_gpu'], capped['host']['host_over_gpu']))
    assert capped['ms_per_step'] <= 1.05 * full['ms_per_step'], (capped['ms_per_step'], full['ms_per_step'])
    assert capped['host']['host_over_gpu'] < 0.9 and full['host']['host_over_gpu'] < 0.9, (capped['host'], full['host'])


@pytest.mark.gpu
def test_bare_bench_gpus2_launches_two_ranks():
    """`python bench.py --gpus 2` with no WORLD_SIZE starts its own two ranks (fresh children through torch.distributed.run) and
    reports n_gpus = 2 -- it used to benchmark ONE GPU silently (round-3 verdict).  gloo so that both ranks can share the box's GPU."""
    import json
    out = _bench('--gpus', '2', '--steps', '2', '--warmup', '1', '--batch', '2', '--no-cpu-baseline', '--full', TTRAP_DIST_BACKEND='gloo')
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    assert line['n_gpus'] == 2 and len(line['per_rank_ms']) == 2 and line['overlap'] is not None
    assert line['config']['global_batch'] == 4 and line['config']['parallelism'] == 'dp2' and line['scaling'] == 'weak'
    assert line['value'] > 0 and line['allreduce_ms'] is not None


@pytest.mark.gpu
def test_bare_bench_more_gpus_than_visible_exits_nonzero():
    """Never a silent fallback to fewer GPUs: asking for more ranks than visible devices (without the gloo override) fails."""
    import torch
    n = torch.cuda.device_count() + 1
    out = _bench('--gpus', str(n), '--steps', '1', '--warmup', '0', '--batch', '1', '--no-cpu-baseline')
    assert out.returncode != 0
    assert not [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert 'refusing' in out.stderr
