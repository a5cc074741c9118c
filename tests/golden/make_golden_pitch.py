"""
Generates tests/golden/pitch.npz by importing the REFERENCE (read-only at /root/reference) in this container and recording what its
``PitchDataset.resample_multi_pitch`` followed by ``PitchDataset.multi_pitch_to_activations`` returns for a closed-form track of 200
irregular source frames read at 300 target times, on the real 540-bin ``midi_freqs``.  Run once here:

    python tests/golden/make_golden_pitch.py

Only inputs and recorded outputs travel; third-party modules the reference imports and this image lacks are stubbed for import only
(``make_golden.install_stubs`` plus empty ``mir_eval`` / ``jams`` / ``mido``).

Two variants: ``a`` holds every corner case, read with ``resample_idcs = [3, -2]``; among them is a pitch outside the bin range in a
source frame that a target reads, so the reference warns.  ``b`` is ``a`` without that pitch (``in_b`` False), read with ``[0, -1]``:
the out-of-range pitch that is left sits in a source frame no target reads, so the reference does not warn.
"""

import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import install_stubs  # noqa: E402

K_SOURCE, N_TARGETS, N_REAL = 200, 300, 260
READ_LOST, UNREAD_LOST = 37, 121              # source frames with an out-of-range pitch: read by a target / read by none
MIDPOINTS = (10, 48, 49, 50, 77, 150)         # source intervals whose exact midpoint is a target (49: the duplicate pair, 48 / 50 around it)
CORNER_FRAMES = (30, 31, 33, 34, 35, 36)      # zeros, one bin twice, neighbouring bins, the edge bins, half way between two bins
IDCS = {'a': [3, -2], 'b': [0, -1]}


def hz(m):
    return 440.0 * (2.0 ** ((np.asarray(m, dtype=np.float64) - 69.0) / 12.0))


def closed_form_track(midi_freqs):
    """(source times (K), list of K arrays in Hz, list of K bool arrays: the value is part of variant b too)."""
    i = np.arange(K_SOURCE)
    src = 0.0058 * i + 0.0011 * ((7 * i) % 5)                               # irregular, increasing: steps between 0.0014 and 0.0102 s
    src[50] = src[49]                                                        # a duplicate source time
    src[UNREAD_LOST - 1], src[UNREAD_LOST + 1] = src[UNREAD_LOST] - 1e-7, src[UNREAD_LOST] + 1e-7      # three frames within 0.2 us
    assert (np.diff(src) >= 0).all()
    mp, keep = [], []
    for k in range(K_SOURCE):
        n = k % 4                                                            # every fourth frame is empty
        bins = [(37 * k + 111 * j) % 500 + 10 for j in range(n)]
        mp.append([float(hz(midi_freqs[b] + 0.03 * ((k + j) % 5 - 2))) for j, b in enumerate(bins)])
        keep.append([True] * n)

    def frame(k, values, in_b=None):
        mp[k], keep[k] = [float(v) for v in values], list(in_b) if in_b is not None else [True] * len(values)
    frame(3, [hz(midi_freqs[60]), hz(midi_freqs[180])])                      # what targets before the span read with idcs [3, -2]
    frame(K_SOURCE - 2, [hz(midi_freqs[90])])                                # ... and targets after it
    frame(0, [hz(midi_freqs[400])])                                          # ... and with [0, -1]
    frame(K_SOURCE - 1, [hz(midi_freqs[420]), hz(midi_freqs[300])])
    frame(30, [0.0, hz(midi_freqs[100]), 0.0])                               # zeros in a list
    frame(31, [0.0])                                                         # nothing but a zero
    frame(33, [hz(midi_freqs[200] + 0.01), hz(midi_freqs[200] - 0.02)])      # two pitches in one bin
    frame(34, [hz(midi_freqs[200]), hz(midi_freqs[201]), hz(midi_freqs[202])])          # neighbouring bins: blurs overlap and clip at 1
    frame(35, [hz(midi_freqs[0]), hz(midi_freqs[-1])])                       # both edge bins
    frame(36, [hz(0.5 * (midi_freqs[250] + midi_freqs[251]))])               # half way between two bins
    frame(READ_LOST, [hz(midi_freqs[150]), hz(midi_freqs[-1] + 1.0)], [True, False])    # outside the bin range, in a frame that is read
    frame(UNREAD_LOST, [hz(midi_freqs[0] - 0.5), hz(midi_freqs[222])])       # outside, in a frame that no target reads
    return src, [np.array(f, dtype=np.float64) for f in mp], [np.array(f, dtype=bool) for f in keep]


def closed_form_targets(src, slicer):
    """300 target times: 260 real ones from before the span to after it, the corner cases written over some of them (so the targets
    are not sorted), then the reference's own ``slice_times`` padding to 300 with -inf in front and +inf behind."""
    real = np.linspace(src[0] - 0.05, src[-1] + 0.05, N_REAL)
    at = 40
    for k in MIDPOINTS:
        mid = src[k] / 2.0 + src[k + 1] / 2.0
        real[at:at + 3] = (mid, np.nextafter(mid, -np.inf), np.nextafter(mid, np.inf))       # the midpoint goes to the earlier frame
        at += 3
    real[70:78] = (src[0], np.nextafter(src[0], -np.inf), src[-1], np.nextafter(src[-1], np.inf), src[49], src[READ_LOST],
                   src[UNREAD_LOST - 1], src[UNREAD_LOST + 1])
    real[78:78 + len(CORNER_FRAMES)] = src[list(CORNER_FRAMES)]             # every corner-case frame is read by at least one target
    times, offset_n = slicer.slice_times(real, n_frames=N_TARGETS, offset_t=-15 * slicer.cqt.hop_length / slicer.sample_rate)
    assert offset_n == -15 and len(times) == N_TARGETS and np.isneginf(times[:15]).all() and np.isposinf(times[-25:]).all()
    return times


def main():
    import scipy.interpolate
    install_stubs()
    for name in ('mir_eval', 'jams', 'mido'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, '/root/reference')
    from timbre_trap.datasets import PitchDataset
    from timbre_trap.framework import CQT
    cqt = CQT(n_octaves=9, bins_per_octave=60, sample_rate=22050, secs_per_block=3)
    midi_freqs = np.asarray(cqt.get_midi_freqs(), dtype=np.float64)
    src, mp, keep = closed_form_track(midi_freqs)

    class Slicer:                                 # the state the reference's two methods read from ``self``
        slice_times = PitchDataset.slice_times
        resample_multi_pitch = PitchDataset.resample_multi_pitch
    slicer = Slicer()
    slicer.cqt, slicer.sample_rate, slicer.n_secs, slicer.rng = cqt, 22050, None, np.random.RandomState(0)
    times = closed_form_targets(src, slicer)
    out = {'midi_freqs': midi_freqs, 'source_times': src, 'times': times, 'values': np.concatenate(mp),
           'counts': np.array([len(f) for f in mp], dtype=np.int64), 'in_b': np.concatenate(keep)}
    for tag in ('a', 'b'):
        lists = mp if tag == 'a' else [f[k] for f, k in zip(mp, keep)]
        slicer.resample_idcs = IDCS[tag]
        original = np.arange(len(src))
        fill = (original[IDCS[tag][0]], original[IDCS[tag][-1]])
        idx = scipy.interpolate.interp1d(x=src, y=original, kind='nearest', bounds_error=False, fill_value=fill,
                                         assume_sorted=True)(times).astype('uint')
        resampled = slicer.resample_multi_pitch(src, lists, times)
        assert all(r is lists[int(i)] for r, i in zip(resampled, idx))
        assert all(k in idx for k in CORNER_FRAMES)
        assert READ_LOST in idx and UNREAD_LOST not in idx and UNREAD_LOST - 1 in idx and UNREAD_LOST + 1 in idx
        out['idcs_%s' % tag] = np.array(IDCS[tag], dtype=np.int64)
        out['idx_%s' % tag] = idx.astype(np.int64)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            out['act_%s_blur' % tag] = PitchDataset.multi_pitch_to_activations(resampled, midi_freqs, 2.5)
            out['act_%s_noblur' % tag] = PitchDataset.multi_pitch_to_activations(resampled, midi_freqs, 0)
        out['warned_%s' % tag] = np.array(any('Could not fully represent' in str(w.message) for w in caught))
        print(tag, 'values', sum(len(f) for f in lists), 'read', len(set(idx.tolist())), 'painted', int(out['act_%s_noblur' % tag].sum()),
              'warned', bool(out['warned_%s' % tag]))
    assert out['warned_a'] and not out['warned_b']
    path = os.path.join(HERE, 'pitch.npz')
    np.savez_compressed(path, **out)
    print('pitch.npz', os.path.getsize(path))


if __name__ == '__main__':
    main()
