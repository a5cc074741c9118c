"""
Random stem mixtures of a training batch on the device (csrc/mix.hip; timbre_trap.utils.StemMixer) against the host route on one
machine: 64 mixtures of 3 s (66150 samples, 1024 frames, 540 bins), 2 to 5 stems each, drawn from 40 synthetic five-minute tracks
uploaded once -- 10 audio-only, 15 + 15 annotated on a 5.8 ms grid with 0-6 random pitches per frame (tools/kb_pitch.py's tracks).

    python tools/kb_mix.py [--iters 30] [--host-iters 2] [--seconds 300] [--items 64] [--tracks 40]

Every result is compared before anything is timed, and a mismatch ends the run: ``batch()`` in float64 and float32 and the two kernels
alone against the yardstick -- per stem the host ``slice_audio`` and this package's list route for the targets
(``resample_multi_pitch`` + ``multi_pitch_to_activations``), the stems added ONE AFTER THE OTHER from zero on the CPU, clamped.  The
timed host route adds with ``torch.sum`` like the reference; how many of its elements differ from the loop (the row tails of 5-stem
groups, tests/test_mix_restatement.py) is reported, not asserted.  One JSON line:
  upload_ms             StemMixer.upload() once per dataset: the audio arena, the annotation arena (not repeated)
  plan_ms               StemMixer.plan(64 indices): the draws and the frame times, host only
  mix_audio_us          tt_mix_audio alone, device events around the launch, tables uploaded beforehand; the plans rotate over 8 batches so
                        that the excerpts read are not the ones the last launch left in the cache
  mix_audio_gbs         its algorithmic bytes (every stem's excerpt read once, the batch written once) over that time
  copy_audio_gbs        a device-to-device copy_ moving the same number of bytes (half read, half written), timed the same way in this
                        process, rotating over 8 buffer pairs
  mix_targets_us / mix_targets_gbs / copy_targets_gbs   the same for tt_mix_targets (float32 out) over the whole batch's stem maps
  mix_targets_f64_us    the same with float64 out
  batch_ms              StemMixer.batch(64 indices), float32 targets, host clock between two device synchronisations (every call
                        draws a new batch)
  batch_f64_ms          the same with float64 targets
  host_ms               the host route for one plan: per stem slice_audio on the CPU and the list route's map brought to the host,
                        torch.sum per group on the CPU, the clamp, the upload of audio and float64 targets, .float() on the device
Medians; *_min / *_max give the spread.  The host figures are this package's host code on the CPU of the same machine, not the
reference's loader.
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'timbre-trap_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from kb_pitch import random_track  # noqa: E402

SAMPLE_RATE, N_SECS, ROTATE = 22050, 3.0, 8


def synthetic_audio(n_tracks, seconds, dev):
    """Uniform noise in [-1, 1], generated on the device from a seed (1 x N each)."""
    gen = torch.Generator(device=dev).manual_seed(0)
    return [torch.rand(1, int(seconds * SAMPLE_RATE), generator=gen, device=dev) * 2 - 1 for _ in range(n_tracks)]


def sequential(rows):
    acc = torch.zeros_like(rows[0])
    for r in rows:
        acc = acc + r
    return acc


def host_route(mixer, plan, host_audio, add, dev):
    """The batch of ``plan`` formed on the host: (audio (B, 1, N) float32, targets (B, F, T) float64) on the device after one upload
    each.  ``add``: how a stack of stems is summed (torch.sum like the reference, or the sequential loop)."""
    from timbre_trap.utils import multi_pitch_to_activations, resample_multi_pitch, slice_audio
    B, N, F, T = len(plan['item_off']) - 1, mixer.n_samples, len(mixer.pitch_bank.midi_freqs), mixer.n_frames
    audio, maps = torch.zeros(B, 1, N), torch.zeros(B, F, T, dtype=torch.float64)
    for b in range(B):
        s0, s1, split = plan['item_off'][b], plan['item_off'][b + 1], plan['item_split'][b]
        cut = [slice_audio(host_audio[plan['stem_track'][s]], N, int(plan['stem_start'][s]), sample_rate=SAMPLE_RATE)[0]
               for s in range(s0, s1)]
        groups = [add(torch.stack(c)) for c in (cut[:split], cut[split:]) if c]
        audio[b] = groups[0] if len(groups) == 1 else groups[0] + groups[1]
        q0, q1 = plan['pitch_off'][b], plan['pitch_off'][b + 1]
        if q1 > q0:
            stems = []
            for q in range(q0, q1):
                src, lists = mixer.pitch_bank.tracks[plan['pitch_track'][q]]
                stems.append(torch.from_numpy(multi_pitch_to_activations(resample_multi_pitch(src, lists, plan['pitch_times'][q]),
                                                                         mixer.pitch_bank.midi_freqs, mixer.n_bins_blur_decay, dev)))
            maps[b] = add(torch.stack(stems)).clamp(0, 1)
    return audio.to(dev), maps.to(dev)


def event_us(fn, iters):
    """Per call: device events around fn(k); microseconds."""
    out = []
    for k in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(k)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def copy_us(n_bytes, iters, dev):
    """copy_ between distinct device buffers, n_bytes moved in all (half read, half written), rotating over ROTATE pairs."""
    n = max(1, n_bytes // 8)
    pairs = [(torch.empty(n, dtype=torch.float32, device=dev).normal_(), torch.empty(n, dtype=torch.float32, device=dev)) for _ in range(ROTATE)]
    for src, dst in pairs:
        dst.copy_(src)
    return event_us(lambda k: pairs[k % ROTATE][1].copy_(pairs[k % ROTATE][0]), iters)


def spread(res, name, values, digits=3):
    res[name] = round(statistics.median(values), digits)
    res[name + '_min'], res[name + '_max'] = round(min(values), digits), round(max(values), digits)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--host-iters', type=int, default=2)
    ap.add_argument('--seconds', type=float, default=300.0)
    ap.add_argument('--items', type=int, default=64)
    ap.add_argument('--tracks', type=int, default=40)
    args = ap.parse_args()
    from timbre_trap import _hip
    from timbre_trap.framework import CQT
    from timbre_trap.utils import StemMixer, StemSource
    if not torch.cuda.is_available():
        raise SystemExit('kb_mix.py measures on the GPU; none found')
    dev = torch.device('cuda:0')
    lib = _hip.lib()
    cqt = CQT(9, 60, SAMPLE_RATE, 3)
    audio = synthetic_audio(args.tracks, args.seconds, dev)
    n_audio = args.tracks // 4
    n_first = n_audio + (args.tracks - n_audio) // 2
    rng = np.random.default_rng(0)
    annotations = [random_track(args.seconds, rng) for _ in range(args.tracks - n_audio)]
    sources = [StemSource(audio[:n_audio], None, seed=1), StemSource(audio[n_audio:n_first], annotations[:n_first - n_audio], seed=2),
               StemSource(audio[n_first:], annotations[n_first - n_audio:], seed=3)]
    mixer = StemMixer(sources, cqt, N_SECS, args.items, seed=0, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mixer.upload()
    torch.cuda.synchronize()
    res = dict(tracks=args.tracks, seconds=args.seconds, items=args.items, samples=mixer.n_samples, frames=mixer.n_frames,
               bins=len(mixer.pitch_bank.midi_freqs), arena_mb=round(mixer.audio_bank.arena.numel() * 4 / 1e6, 1),
               upload_ms=round((time.perf_counter() - t0) * 1e3, 1))
    host_audio = [a.cpu() for a in audio]
    idx = list(range(args.items))
    B, N, F, T = args.items, mixer.n_samples, len(mixer.pitch_bank.midi_freqs), mixer.n_frames
    bank, pbank = mixer.audio_bank, mixer.pitch_bank
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)              # noqa: E731

    # ---- equality first (this pass is also the warm-up of every route) ----------------------------------------------------------------
    state = (mixer.rng.get_state(), [s.rng.get_state() for s in sources])

    def rewind():
        mixer.rng.set_state(state[0])
        for s, st in zip(sources, state[1]):
            s.rng.set_state(st)
    plans = [mixer.plan(idx) for _ in range(ROTATE)]
    p0 = plans[0]
    want_audio, want_maps = host_route(mixer, p0, host_audio, sequential, dev)
    sum_audio, sum_maps = host_route(mixer, p0, host_audio, lambda x: torch.sum(x, dim=0), dev)
    rewind()
    got64 = mixer.batch(idx, dtype=torch.float64)
    rewind()
    got32 = mixer.batch(idx)
    assert torch.equal(got64['audio'], want_audio) and torch.equal(got32['audio'], want_audio), 'audio differs from the sequential host route'
    assert torch.equal(got64['ground_truth'], want_maps), 'float64 targets differ from the sequential host route'
    assert torch.equal(got32['ground_truth'], want_maps.float()), 'float32 targets differ'
    assert np.array_equal(got64['times'][got64['annotated']], p0['pitch_times'][p0['pitch_off'][:-1][got64['annotated']]])
    res.update(stems=int(p0['item_off'][-1]), annotated_stems=int(p0['pitch_off'][-1]), results_equal=True,
               torch_sum_differs_audio=int((sum_audio != want_audio).sum()), torch_sum_differs_targets=int((sum_maps != want_maps).sum()),
               groups_of_5=int(sum(1 for b in range(B) for n in (p0['item_split'][b], p0['item_off'][b + 1] - p0['item_off'][b] - p0['item_split'][b])
                                   if n == 5)))

    # ---- the kernels alone --------------------------------------------------------------------------------------------------------------
    tables = [[up(p[k]) for k in ('stem_track', 'stem_start', 'item_off', 'item_split')] for p in plans]
    y = torch.empty((B, 1, N), dtype=torch.float32, device=dev)
    st = _hip.stream_ptr()

    def launch_audio(k):
        t = tables[k % ROTATE]
        _hip.check(lib.tt_mix_audio(_hip.ptr(bank.arena), _hip.ptr(bank.table_d), len(bank), _hip.ptr(t[0]), _hip.ptr(t[1]), _hip.ptr(t[2]),
                                    _hip.ptr(t[3]), B, N, _hip.ptr(y), st))
    launch_audio(0)
    assert torch.equal(y, want_audio), 'tt_mix_audio alone differs'
    for k in range(ROTATE):
        launch_audio(k)
    audio_bytes = [(int(p['item_off'][-1]) + B) * N * 4 for p in plans]
    us = event_us(launch_audio, args.iters)
    spread(res, 'mix_audio_us', us, 1)
    res['mix_audio_gbs'] = round(statistics.median(audio_bytes[k % ROTATE] / (u * 1e-6) / 1e9 for k, u in enumerate(us)), 1)
    cus = copy_us(int(statistics.median(audio_bytes)), args.iters, dev)
    res['copy_audio_gbs'] = round(statistics.median(audio_bytes) / (statistics.median(cus) * 1e-6) / 1e9, 1)
    spread(res, 'copy_audio_us', cus, 1)

    A = int(p0['pitch_off'][-1])
    maps = torch.empty((A, F, T), dtype=torch.float64, device=dev)
    for a0 in range(0, A, 32):
        maps[a0:a0 + 32] = pbank.targets(p0['pitch_track'][a0:a0 + 32], p0['pitch_times'][a0:a0 + 32], mixer.n_bins_blur_decay, torch.float64)
    off_d = up(p0['pitch_off'])
    target_bytes = {}
    for name, dtype in (('mix_targets', torch.float32), ('mix_targets_f64', torch.float64)):
        out = torch.empty((B, F, T), dtype=dtype, device=dev)
        launch = lambda k: _hip.check(lib.tt_mix_targets(_hip.ptr(maps), _hip.ptr(off_d), B, F, T, int(dtype == torch.float32),  # noqa: E731
                                                         _hip.ptr(out), st))
        launch(0)
        assert torch.equal(out, want_maps.to(dtype)), 'tt_mix_targets alone differs'
        launch(1)
        us = event_us(launch, args.iters)
        spread(res, name + '_us', us, 1)
        target_bytes[name] = A * F * T * 8 + B * F * T * out.element_size()
        res[name + '_gbs'] = round(target_bytes[name] / (statistics.median(us) * 1e-6) / 1e9, 1)
        del out
    del maps
    cus = copy_us(target_bytes['mix_targets'], max(5, args.iters // 3), dev)
    res['copy_targets_gbs'] = round(target_bytes['mix_targets'] / (statistics.median(cus) * 1e-6) / 1e9, 1)
    spread(res, 'copy_targets_us', cus, 1)
    torch.cuda.empty_cache()

    # ---- the front ----------------------------------------------------------------------------------------------------------------------
    def clock(fn, iters):
        ms = []
        for _ in range(iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms
    spread(res, 'plan_ms', clock(lambda: mixer.plan(idx), args.iters))
    spread(res, 'batch_ms', clock(lambda: mixer.batch(idx), args.iters))
    spread(res, 'batch_f64_ms', clock(lambda: mixer.batch(idx, dtype=torch.float64), args.iters))

    def host():
        a, m = host_route(mixer, p0, host_audio, lambda x: torch.sum(x, dim=0), dev)
        return a, m.float()
    spread(res, 'host_ms', clock(host, args.host_iters), 1)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
