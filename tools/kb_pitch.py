"""
Frame-level pitch annotations to batched targets and to the scorer's reference (csrc/pitch.hip) against this package's host route on
one machine, on a synthetic five-minute track: a 5.8 ms annotation grid (51 725 frames), 0-6 random pitches per frame (seed 0,
27.5 Hz - 3.5 kHz), 540 bins (472 below 5 kHz).  Targets are timed for the batch a training step holds -- 64 items of 1024 frames at 341
frames / s, cut at 64 offsets spread over the track -- and for one item; the scorer on the whole track.

    python tools/kb_pitch.py [--iters 20] [--host-iters 3] [--seconds 300] [--items 64]

Every result is compared before anything is timed: the batch against the host route item by item (float64 ``array_equal``, float32
against its ``.float()``), the score dictionaries with ``==``; a mismatch ends the run.  One JSON line:
  bank_build_ms         PitchBank(...) once per dataset: the lists flattened, bins and MIDI numbers for every value in NumPy, six uploads
  targets_ms            bank.targets(ids, times) for the batch, float32 on the device, warm, host clock between two device synchronisations
                        (two uploads, tt_pitch_nearest, tt_pitch_targets, the flags back)
  targets_f64_ms        the same in float64
  targets_one_ms        bank.targets for one item (B = 1), float32
  host_targets_ms       the host route for the batch: per item resample_multi_pitch (list comprehension over the frames) +
                        multi_pitch_to_activations (Python loop over the frames, two uploads, tt_target_activations), the float64 maps left on
                        the device, then stacked and cast with .float()
  host_targets_one_ms   the same for one item
  evaluate_track_ms     MultipitchEvaluator.evaluate_track on the whole track, activations on the device, reference read from the bank
  host_evaluate_ms      evaluate_activations with the track's lists (flattened to CSR in NumPy and uploaded per call)
  targets_equal / scores_equal   as asserted above
Medians; *_min / *_max give the spread.  The host figures are this package's host code on the CPU of the same machine, not the
reference's loops.
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

from kb_mpe import F, FV, synthetic_track  # noqa: E402

EXCERPT, FRAME_RATE, ANNOTATION_STEP = 1024, 341.0, 0.0058


def random_track(seconds, rng):
    times = np.arange(0.0, seconds, ANNOTATION_STEP)
    return times, [27.5 * 2.0 ** rng.uniform(0.0, 7.0, size=int(n)) for n in rng.integers(0, 7, size=len(times))]


def timed(fn, iters):
    out, ms = None, []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--host-iters', type=int, default=3)
    ap.add_argument('--seconds', type=float, default=300.0)
    ap.add_argument('--items', type=int, default=64)
    args = ap.parse_args()
    from timbre_trap.utils import MultipitchEvaluator, PitchBank, multi_pitch_to_activations, resample_multi_pitch
    dev = torch.device('cuda:0')
    midi_freqs = 16.76557586 + np.arange(F) / 5.0
    src, lists = random_track(args.seconds, np.random.default_rng(0))
    n_est = int(args.seconds * FRAME_RATE)
    est_time = np.arange(n_est) / FRAME_RATE
    x = synthetic_track(n_est, dev)
    starts = np.linspace(0, n_est - EXCERPT, args.items).astype(np.int64)
    times = np.stack([est_time[s:s + EXCERPT] for s in starts])
    ids = np.zeros(args.items, dtype=np.int64)
    ev = MultipitchEvaluator()

    def host_item(t):
        return multi_pitch_to_activations(resample_multi_pitch(src, lists, t), midi_freqs, device=dev, return_tensor=True)

    build = lambda: PitchBank([(src, lists)], midi_freqs, device=dev)              # noqa: E731
    bank = build()
    routes = {
        'bank_build': (build, args.host_iters),
        'targets': (lambda: bank.targets(ids, times), args.iters),
        'targets_f64': (lambda: bank.targets(ids, times, dtype=torch.float64), args.iters),
        'targets_one': (lambda: bank.targets(0, times[len(times) // 2]), args.iters),
        'host_targets': (lambda: torch.stack([host_item(t) for t in times]).float(), args.host_iters),
        'host_targets_one': (lambda: host_item(times[len(times) // 2]).float(), args.iters),
        'evaluate_track': (lambda: ev.evaluate_track(est_time, x, midi_freqs, bank, 0, n_valid_bins=FV), args.iters),
        'host_evaluate': (lambda: ev.evaluate_activations(est_time, x, midi_freqs, src, lists, n_valid_bins=FV), args.host_iters),
    }
    # equality first: a difference ends the run before anything is timed (this pass is also the warm-up of every route)
    first = {name: fn() for name, (fn, _) in routes.items()}
    want64 = torch.stack([host_item(t) for t in times])
    assert torch.equal(first['targets_f64'], want64), 'float64 targets differ from the host route'
    assert torch.equal(first['targets'], want64.float()) and torch.equal(first['host_targets'], want64.float()), 'float32 targets differ'
    assert torch.equal(first['targets_one'], first['host_targets_one']), 'single-item targets differ'
    assert first['evaluate_track'] == first['host_evaluate'], 'scores differ'
    ms = {name: timed(fn, iters)[1] for name, (fn, iters) in routes.items()}
    per_frame = np.array([len(f) for f in lists])
    res = dict(seconds=args.seconds, source_frames=len(src), values=int(per_frame.sum()), pitches_per_frame_mean=round(float(per_frame.mean()), 2),
               items=args.items, item_frames=EXCERPT, estimate_frames=n_est, painted=int((want64 == 1).sum()),
               f1=round(first['evaluate_track']['mpe/f1-score'], 6))
    for name, v in ms.items():
        res[name + '_ms'] = round(statistics.median(v), 3)
        res[name + '_ms_min'], res[name + '_ms_max'] = round(min(v), 3), round(max(v), 3)
    res['targets_equal'] = res['scores_equal'] = True                              # asserted above
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
