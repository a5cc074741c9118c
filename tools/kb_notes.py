"""
Note annotations to targets and to the scorer's reference (csrc/notes.hip, tt_target_activations_spans) against this package's host
route on one machine, on a synthetic five-minute track: 6000 random notes (seed 0) over 102 400 frames at 341 frames / s, 540 bins
(472 below 5 kHz).  Targets are timed at the excerpt a training item holds (n_secs = 3: 1024 frames from the middle of the track, all
6000 notes handed in, as NoteDataset.__getitem__ does), the scorer on the whole track.

    python tools/kb_notes.py [--iters 20] [--host-iters 3] [--frames 102400] [--notes 6000]

One JSON line:
  targets_ms            notes_to_activations(..., return_tensor=True) on the excerpt, warm, host clock between two device synchronisations
                        (per-note bins in NumPy, three small uploads, tt_note_spans, tt_target_activations_spans, one flag back)
  targets_download_ms   the same returning an ndarray like the reference: plus the (540, 1024) float64 map to the host
  host_lists_ms         notes_to_multi_pitch (this package's vectorised host function) on the excerpt
  host_targets_ms       host_lists_ms + multi_pitch_to_activations of those lists (Python loop over the frames, then tt_target_activations
                        and the same download)
  evaluate_notes_ms     MultipitchEvaluator.evaluate_notes on the whole track, activations on the device, warm, synchronised
  host_track_lists_ms   notes_to_multi_pitch on the whole track
  host_evaluate_ms      host_track_lists_ms + evaluate_activations with those lists (the ragged reference flattened in NumPy)
  targets_equal / scores_equal   the two routes' maps are array_equal, their score dictionaries ==
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

EXCERPT = 1024


def random_notes(n_notes, seconds, rng):
    """Onsets anywhere on the track, 0.1 - 1.0 s long (at most 24 sounding at once), 27.5 Hz - 3.5 kHz, in no particular order."""
    on = rng.uniform(0.0, seconds, size=n_notes)
    return 27.5 * 2.0 ** rng.uniform(0.0, 7.0, size=n_notes), np.stack([on, on + rng.uniform(0.1, 1.0, size=n_notes)], 1)


def timed(fn, iters, sync):
    out, ms = None, []
    for _ in range(iters):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        if sync:
            torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--host-iters', type=int, default=3)
    ap.add_argument('--frames', type=int, default=102400)
    ap.add_argument('--notes', type=int, default=6000)
    args = ap.parse_args()
    from timbre_trap.utils import MultipitchEvaluator, multi_pitch_to_activations, notes_to_activations, notes_to_multi_pitch
    dev = torch.device('cuda:0')
    midi_freqs = 16.76557586 + np.arange(F) / 5.0
    times = np.arange(args.frames) / 341.0
    pitches, intervals = random_notes(args.notes, times[-1], np.random.default_rng(0))
    start = max(0, (args.frames - EXCERPT) // 2)
    excerpt = times[start:start + EXCERPT]
    x = synthetic_track(args.frames, dev)
    ev = MultipitchEvaluator()

    routes = {
        'targets': (lambda: notes_to_activations(pitches, intervals, excerpt, midi_freqs, device=dev, return_tensor=True), args.iters),
        'targets_download': (lambda: notes_to_activations(pitches, intervals, excerpt, midi_freqs, device=dev), args.iters),
        'host_lists': (lambda: notes_to_multi_pitch(pitches, intervals, excerpt), args.host_iters),
        'host_targets': (lambda: multi_pitch_to_activations(notes_to_multi_pitch(pitches, intervals, excerpt), midi_freqs, device=dev),
                         args.host_iters),
        'evaluate_notes': (lambda: ev.evaluate_notes(times, x, midi_freqs, times, pitches, intervals, n_valid_bins=FV), args.iters),
        'host_track_lists': (lambda: notes_to_multi_pitch(pitches, intervals, times), args.host_iters),
        'host_evaluate': (lambda: ev.evaluate_activations(times, x, midi_freqs, times, notes_to_multi_pitch(pitches, intervals, times),
                                                          n_valid_bins=FV), args.host_iters),
    }
    out, ms = {}, {}
    for name, (fn, iters) in routes.items():
        fn()                                                   # once untimed: lazy kernel loading, allocator growth
        out[name], ms[name] = timed(fn, iters, sync=True)
    per_frame = np.array([len(f) for f in out['host_track_lists']])
    res = dict(frames=args.frames, seconds=round(args.frames / 341.0, 1), notes=args.notes, excerpt_frames=len(excerpt),
               notes_per_frame_mean=round(float(per_frame.mean()), 2), notes_per_frame_max=int(per_frame.max()),
               excerpt_pairs=int(sum(len(f) for f in out['host_lists'])), f1=round(out['evaluate_notes']['mpe/f1-score'], 6))
    for name, v in ms.items():
        res[name + '_ms'] = round(statistics.median(v), 3)
        res[name + '_ms_min'], res[name + '_ms_max'] = round(min(v), 3), round(max(v), 3)
    res['targets_equal'] = bool(np.array_equal(out['targets_download'], out['host_targets']) and
                                np.array_equal(out['targets'].cpu().numpy(), out['host_targets']))
    res['scores_equal'] = out['evaluate_notes'] == out['host_evaluate']
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
