"""
Generates tests/golden/notes.npz by importing the REFERENCE (read-only at /root/reference) in this container and recording what its
``NoteDataset.notes_to_multi_pitch`` and ``PitchDataset.multi_pitch_to_activations`` return for a closed-form note set on the real
540-bin ``midi_freqs`` and the ``CQT.get_times`` grid of 300 frames.  Run once here:

    python tests/golden/make_golden_notes.py

Only inputs and recorded outputs travel; third-party modules the reference imports and this image lacks are stubbed for import only
(``make_golden.install_stubs`` plus empty ``mir_eval`` / ``jams`` / ``mido``).

Two note sets: ``a`` holds every corner case, two pitches outside the bin range among them, so the reference warns; ``b`` is ``a``
without the notes ``in_b`` marks False (the out-of-range ones), so it does not.
"""

import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import install_stubs  # noqa: E402

N_FRAMES = 300


def hz(m):
    return 440.0 * (2.0 ** ((np.asarray(m, dtype=np.float64) - 69.0) / 12.0))


def closed_form_notes(midi_freqs, times):
    """(pitches Hz (L), intervals (L, 2), in_b (L) bool): regular notes all over the grid, then the corner cases one by one."""
    hop = times[1] - times[0]
    p, iv, keep = [], [], []

    def note(pitch, on, off, in_b=True):
        p.append(float(pitch))
        iv.append((float(on), float(off)))
        keep.append(in_b)
    for i in range(40):
        k = (37 * i) % 500 + 10
        start = (53 * i) % 270
        length = 3 + (11 * i) % 40
        frac = (0.0, 0.25, 0.5, 0.75)[i % 4]                               # every fourth onset falls exactly on a frame time
        note(hz(midi_freqs[k] + 0.03 * ((i % 5) - 2)), times[start] + frac * hop, times[start] + (length + 0.4) * hop)
    note(hz(midi_freqs[100]), times[20], times[30])                        # onset on a frame (in), offset on a frame (out)
    note(hz(midi_freqs[102]), np.nextafter(times[40], np.inf), np.nextafter(times[50], -np.inf))      # one ulp inside both
    note(hz(midi_freqs[104]), times[60], times[60])                        # zero length
    note(hz(midi_freqs[106]), times[80], times[70])                        # reversed
    note(hz(midi_freqs[108]), -3.0, -1.0)                                  # wholly before the grid
    note(hz(midi_freqs[110]), times[-1] + 1.0, times[-1] + 2.0)            # wholly after it
    note(hz(midi_freqs[300]), -1.0, times[-1] + 1.0)                       # covers every frame
    note(hz(midi_freqs[200] + 0.01), times[100] + 0.5 * hop, times[130])   # a note and its twin: twice in the lists, once in the map
    note(hz(midi_freqs[200] + 0.01), times[100] + 0.5 * hop, times[130])
    note(hz(midi_freqs[201] - 0.02), times[110], times[140])               # the neighbouring bin: blurs overlap and clip at 1
    note(hz(midi_freqs[112]), np.nan, times[150])                          # a NaN bound either side
    note(hz(midi_freqs[114]), times[140], np.nan)
    note(0.0, times[150], times[170])                                      # the "no pitch" marker, filtered
    note(hz(midi_freqs[-1] + 1.0), times[160], times[165], in_b=False)     # outside the bin range: dropped with a warning
    note(hz(midi_freqs[0] - 0.5), times[200], times[204], in_b=False)
    note(hz(midi_freqs[0] - 0.5), times[210], times[210])                  # outside, but silent: no warning on its account
    note(hz(midi_freqs[0]), times[220], times[230])                        # the edge bins
    note(hz(midi_freqs[-1]), times[225], times[235])
    note(hz(0.5 * (midi_freqs[250] + midi_freqs[251])), times[240], times[260])        # half way between two bins
    return np.array(p), np.array(iv), np.array(keep)


def main():
    install_stubs()
    for name in ('mir_eval', 'jams', 'mido'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, '/root/reference')
    from timbre_trap.datasets import NoteDataset, PitchDataset
    from timbre_trap.framework import CQT
    cqt = CQT(n_octaves=9, bins_per_octave=60, sample_rate=22050, secs_per_block=3)
    midi_freqs = np.asarray(cqt.get_midi_freqs(), dtype=np.float64)
    times = np.asarray(cqt.get_times(N_FRAMES), dtype=np.float64)
    pitches, intervals, in_b = closed_form_notes(midi_freqs, times)
    out = {'midi_freqs': midi_freqs, 'times': times, 'pitches': pitches, 'intervals': intervals, 'in_b': in_b}
    for tag, sel in (('a', np.ones(len(pitches), dtype=bool)), ('b', in_b)):
        mp = NoteDataset.notes_to_multi_pitch(pitches[sel], intervals[sel], times)
        out['mp_%s_values' % tag] = np.concatenate(mp)
        out['mp_%s_counts' % tag] = np.array([len(f) for f in mp], dtype=np.int64)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            out['act_%s_blur' % tag] = PitchDataset.multi_pitch_to_activations(mp, midi_freqs, 2.5)
            out['act_%s_noblur' % tag] = PitchDataset.multi_pitch_to_activations(mp, midi_freqs, 0)
        out['warned_%s' % tag] = np.array(any('Could not fully represent' in str(w.message) for w in caught))
        print(tag, 'notes', int(sel.sum()), 'pairs', len(out['mp_%s_values' % tag]), 'warned', bool(out['warned_%s' % tag]))
    path = os.path.join(HERE, 'notes.npz')
    np.savez_compressed(path, **out)
    print('notes.npz', os.path.getsize(path))


if __name__ == '__main__':
    main()
