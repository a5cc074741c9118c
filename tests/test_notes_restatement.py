"""
CPU-only: the host ``notes_to_multi_pitch`` (timbre_trap/utils/notes.py) against the lists the reference's
``NoteDataset.notes_to_multi_pitch`` returned (tests/golden/notes.npz, recorded by tests/golden/make_golden_notes.py) and against a
restatement of its mask in this file's own words, on the note sets tests/test_gpu_notes.py runs on the device; plus the host-side
pieces of the device routes that need no GPU (the per-note frame ranges, the per-note bins, argument checks, the dataset stand-in).

Everything here is float64 comparisons and integers, so every assertion is ``==`` / ``array_equal``.

``grid`` / ``note_case`` / ``eval_case`` / ``host_lists`` / ``golden_sets`` are shared with tests/test_gpu_notes.py; what they return is
cached and read-only.
"""

import functools
import os

import numpy as np
import pytest

from timbre_trap.utils import metrics, notes
from timbre_trap.utils.metrics import MPE_MAX_REF
from timbre_trap.utils.notes import notes_to_multi_pitch
from timbre_trap.utils.targets import hz_to_midi, midi_to_hz

from test_mpe_restatement import FV, MIDI_FREQS, frozen

HOP = 64.0 / 22050.0                          # seconds per frame of the 3-second CQT grid (get_times: n * hop_length / sample_rate)
N_EDGE = 21                                   # notes edge_notes() returns
CROWD, CROWD_FRAMES = MPE_MAX_REF + 6, (300, 303)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'notes.npz')


# ---- inputs -------------------------------------------------------------------------------------------------------------------

def grid(n_frames):
    return frozen(np.arange(n_frames) * HOP)


def between_two_bins():
    """A frequency whose MIDI number, as hz_to_midi gives it, is exactly the midpoint of two bins as the target code forms it --
    or, should no such double exist near a midpoint, the nearest one (the two sides still see the same number)."""
    mids = (MIDI_FREQS[1:] + MIDI_FREQS[:-1]) / 2.0
    for k in range(100, 400):
        h = midi_to_hz(mids[k])
        for cand in (h, np.nextafter(h, 0.0), np.nextafter(h, np.inf)):
            if hz_to_midi(cand) == mids[k]:
                return float(cand), True
    return float(midi_to_hz(mids[250])), False


def edge_notes(times, evaluable):
    """The corner cases of the issue, on any grid (indices are clipped to it).  ``evaluable``: every pitch inside [20, 5000] Hz and
    non-zero, as the scorer demands of a note that sounds; otherwise pitch 0 and pitches just outside both ends of the bin range are
    among them and sound."""
    n = len(times)
    at = lambda i: times[min(i, n - 1)]                                       # noqa: E731
    first, last = times[0], times[-1]
    tie, _ = between_two_bins()
    zero, below, above = ((midi_to_hz(MIDI_FREQS[120]), midi_to_hz(MIDI_FREQS[0]), midi_to_hz(MIDI_FREQS[FV - 1])) if evaluable else
                          (0.0, midi_to_hz(MIDI_FREQS[0] - 1e-6), midi_to_hz(MIDI_FREQS[-1] + 1e-6)))
    rows = [
        (midi_to_hz(MIDI_FREQS[100]), at(20), at(30)),                        # onset on a frame time (in), offset on one (out)
        (midi_to_hz(MIDI_FREQS[102]), np.nextafter(at(40), np.inf), np.nextafter(at(50), -np.inf)),     # one ulp inside both
        (midi_to_hz(MIDI_FREQS[104]), at(60), at(60)),                        # zero length
        (midi_to_hz(MIDI_FREQS[106]), at(80), at(70)),                        # reversed
        (midi_to_hz(MIDI_FREQS[108]), first - 3.0, first - 1.0),              # wholly before the grid
        (midi_to_hz(MIDI_FREQS[110]), last + 1.0, last + 2.0),                # wholly after it
        (midi_to_hz(MIDI_FREQS[300]), first - 1.0, last + 1.0),               # covers every frame
        (midi_to_hz(MIDI_FREQS[200] + 0.01), at(100) + 0.5 * HOP, at(130)),   # a note and its twin
        (midi_to_hz(MIDI_FREQS[200] + 0.01), at(100) + 0.5 * HOP, at(130)),
        (midi_to_hz(MIDI_FREQS[201] - 0.02), at(110), at(140)),               # the neighbouring bin
        (midi_to_hz(MIDI_FREQS[112]), np.nan, at(150)),                       # a NaN bound, either side and both
        (midi_to_hz(MIDI_FREQS[114]), at(140), np.nan),
        (midi_to_hz(MIDI_FREQS[116]), np.nan, np.nan),
        (zero, at(150), at(170)),                                             # pitch 0: the "no pitch" marker
        (above, at(160), at(165)),                                            # just above the last bin
        (below, at(200), at(204)),                                            # just below the first
        (midi_to_hz(MIDI_FREQS[-1] + 3.0), at(210), at(210)),                 # far outside (> 5 kHz) but silent: nobody may mind
        (midi_to_hz(MIDI_FREQS[0]), at(220), at(230)),                        # the edge bins of the range in use
        (midi_to_hz(MIDI_FREQS[FV - 1]), at(225), at(235)),
        (tie, at(240), at(260)),                                              # half way between two bins
        (midi_to_hz(MIDI_FREQS[150]), first, np.inf),                         # an infinite offset
    ]
    assert len(rows) == N_EDGE
    return [r[0] for r in rows], [(r[1], r[2]) for r in rows]


@functools.lru_cache(maxsize=None)
def note_case(n_frames, n_notes, evaluable=False, crowd=False, seed=0):
    """times (n_frames), pitches Hz (n_notes), intervals (n_notes, 2): the edge notes first (when n_notes leaves room for them), then
    random short notes in no particular order -- about seven sounding per frame -- every fifth with its onset exactly on a frame time;
    ``crowd``: the last CROWD notes all sound over frames CROWD_FRAMES, more than the matching kernel holds."""
    times = grid(n_frames)
    rng = np.random.default_rng([seed, n_frames, n_notes, int(evaluable)])
    p, iv = edge_notes(times, evaluable) if n_notes >= N_EDGE else ([], [])
    m = n_notes - len(p)
    on = rng.uniform(times[0] - 0.05, times[-1] + 0.05, size=m)
    on[::5] = times[rng.integers(0, n_frames, size=len(on[::5]))]
    dur = rng.uniform(-0.005, 0.05, size=m)
    pitch = midi_to_hz(MIDI_FREQS[rng.integers(0, FV, size=m)] + rng.normal(0.0, 0.05, size=m))
    pitch = np.clip(pitch, metrics.MIN_FREQ, metrics.MAX_FREQ)
    if m and n_notes < N_EDGE:
        on[0], dur[0] = times[0], 1.5 * HOP                                   # a lone note is one that sounds
    pitches = np.concatenate([np.array(p, dtype=np.float64), pitch])
    intervals = np.concatenate([np.array(iv, dtype=np.float64).reshape(-1, 2), np.stack([on, on + dur], 1)])
    if crowd:
        a, b = CROWD_FRAMES
        intervals[-CROWD:] = (times[a], times[b])
        pitches[-CROWD:] = midi_to_hz(MIDI_FREQS[np.arange(CROWD) * 5 + 40] + 0.01)
    return dict(key=('notes', n_frames, n_notes, evaluable, crowd, seed), times=times, pitches=frozen(pitches), intervals=frozen(intervals))


@functools.lru_cache(maxsize=None)
def host_lists(case_key):
    """The host yardstick on one case, once (read-only arrays)."""
    case = note_case(*case_key[1:])
    return tuple(frozen(f) for f in notes_to_multi_pitch(case['pitches'], case['intervals'], case['times']))


def lists_of(case):
    return host_lists(case['key'])


@functools.lru_cache(maxsize=None)
def golden_sets():
    """tests/golden/notes.npz as {'a' | 'b': dict(pitches, intervals, lists, act_blur, act_noblur, warned)}, times, midi_freqs."""
    g = np.load(GOLDEN)
    sets = {}
    for tag, sel in (('a', np.ones(len(g['pitches']), dtype=bool)), ('b', g['in_b'])):
        lists = np.split(g['mp_%s_values' % tag], np.cumsum(g['mp_%s_counts' % tag])[:-1])
        sets[tag] = dict(pitches=frozen(g['pitches'][sel]), intervals=frozen(g['intervals'][sel]), lists=tuple(frozen(f) for f in lists),
                         act_blur=frozen(g['act_%s_blur' % tag]), act_noblur=frozen(g['act_%s_noblur' % tag]),
                         warned=bool(g['warned_%s' % tag]))
    return sets, frozen(g['times']), frozen(g['midi_freqs'])


def same_lists(got, want):
    return len(got) == len(want) and all(g.dtype == np.float64 and np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want))


def mask_lists(pitches, intervals, times):
    """The reference's condition, stated as one (note, frame) mask: a row per note, read down a column in note order."""
    sounding = (times[None, :] >= intervals[:, :1]) & (times[None, :] < intervals[:, 1:])
    return [pitches[sounding[:, t]] for t in range(len(times))]


SIZES = ((549, 531), (1, 531), (549, 1), (1, 1), (300, 0))        # the GPU test takes its sizes from the tile constants instead


# ---- tests --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('tag', ('a', 'b'))
def test_host_function_gives_the_reference_lists(tag):
    sets, times, _ = golden_sets()
    s = sets[tag]
    assert len(s['lists']) == len(times) == 300 and sum(len(f) for f in s['lists']) > 1000
    assert same_lists(notes_to_multi_pitch(s['pitches'], s['intervals'], times), s['lists'])
    assert sets['a']['warned'] and not sets['b']['warned']
    # integer MIDI-like input and float32 intervals are read as float64, like the reference's comparisons promote them
    got = notes_to_multi_pitch(s['pitches'], s['intervals'].astype(np.float32), times)
    assert same_lists(got, mask_lists(s['pitches'], s['intervals'].astype(np.float32).astype(np.float64), times))


@pytest.mark.parametrize('n_frames,n_notes', SIZES)
@pytest.mark.parametrize('evaluable', (False, True))
def test_host_function_is_the_mask(n_frames, n_notes, evaluable):
    case = note_case(n_frames, n_notes, evaluable)
    want = mask_lists(case['pitches'], case['intervals'], case['times'])
    got = lists_of(case)
    assert same_lists(got, want)
    if n_notes >= N_EDGE and n_frames > 260:
        assert len(got[20]) >= 2 and len(got[104]) >= 3 and not any(len(f) == 0 for f in got)     # the long note sounds everywhere
        twin = case['pitches'][7]
        assert (got[110] == twin).sum() == 2                                       # the duplicate appears twice
        assert case['pitches'][0] in got[20] and case['pitches'][0] in got[29] and case['pitches'][0] not in got[30]
        assert case['pitches'][1] not in got[40] and case['pitches'][1] in got[41] and case['pitches'][1] not in got[50]
    if n_notes == 1:
        assert len(got[0]) == 1
    if n_notes == 0:
        assert all(f.size == 0 for f in got) and len(got) == n_frames


def test_unsorted_times_take_the_mask_route():
    case = note_case(549, 531)
    perm = np.random.default_rng(3).permutation(549)
    times = case['times'][perm]
    assert not notes._is_sorted(times) and notes._is_sorted(case['times'])
    got = notes_to_multi_pitch(case['pitches'], case['intervals'], times)
    assert same_lists(got, mask_lists(case['pitches'], case['intervals'], times))
    assert same_lists(got, [lists_of(case)[i] for i in perm])
    with_nan = np.array(case['times'])
    with_nan[17] = np.nan                                                          # a NaN time is "not sorted": no frame of it sounds
    assert not notes._is_sorted(with_nan)
    got = notes_to_multi_pitch(case['pitches'], case['intervals'], with_nan)
    assert same_lists(got, mask_lists(case['pitches'], case['intervals'], with_nan)) and got[17].size == 0
    repeated = np.sort(np.concatenate([case['times'][:50], case['times'][:50]]))   # equal neighbours are sorted
    assert notes._is_sorted(repeated)
    assert same_lists(notes_to_multi_pitch(case['pitches'], case['intervals'], repeated), mask_lists(case['pitches'], case['intervals'], repeated))


def test_spans_are_the_mask_rows():
    """What tt_note_spans is tested against: per note the mask row is the range [lo, hi), empty iff hi <= lo."""
    for evaluable in (False, True):
        case = note_case(549, 531, evaluable)
        lo, hi = notes._host_spans(case['intervals'], case['times'])
        sounding = (case['times'][None, :] >= case['intervals'][:, :1]) & (case['times'][None, :] < case['intervals'][:, 1:])
        for i in range(len(lo)):
            assert np.array_equal(np.flatnonzero(sounding[i]), np.arange(lo[i], max(hi[i], lo[i])))
        assert (hi[[2, 3, 4, 5, 10, 11, 12]] <= lo[[2, 3, 4, 5, 10, 11, 12]]).all()
        assert (lo[6], hi[6]) == (0, 549) and (lo[0], hi[0]) == (20, 30) and (lo[1], hi[1]) == (41, 50) and hi[20] == 549


def test_note_bins_are_the_target_code_per_frame():
    """_note_bins over L pitches against the expressions of multi_pitch_to_activations over one frame holding all of them."""
    case = note_case(549, 531)
    p = case['pitches']
    bins, lost = notes._note_bins(p, MIDI_FREQS)
    mids = (MIDI_FREQS[1:] + MIDI_FREQS[:-1]) / 2.0
    m = hz_to_midi(p[p != 0])
    inside = np.logical_and(m >= MIDI_FREQS.min(), m <= MIDI_FREQS.max())
    assert np.array_equal(bins[bins >= 0], np.searchsorted(mids, m[inside], side='left'))
    assert lost.sum() == len(m) - inside.sum() == 3 and (bins[lost] == -1).all()     # below, above, and the silent far-outside one
    assert bins[13] == -1 and not lost[13]                                          # pitch 0 is dropped without a warning
    tie, exact = between_two_bins()
    assert exact, 'no double whose MIDI number is exactly a bin midpoint'
    k = bins[19]
    assert hz_to_midi(tie) == mids[k] and MIDI_FREQS[k] < hz_to_midi(tie) < MIDI_FREQS[k + 1]          # the tie goes to the lower bin


def test_crowd_case_exceeds_the_matcher():
    case = note_case(549, 531, True, True)
    n = np.array([len(f) for f in lists_of(case)])
    a, b = CROWD_FRAMES
    assert (n[a:b] >= CROWD).all() and (n > MPE_MAX_REF).sum() == b - a
    assert np.array([len(f) for f in lists_of(note_case(549, 531, True))]).max() <= MPE_MAX_REF
    flat = np.concatenate(lists_of(case))
    assert flat.min() >= metrics.MIN_FREQ and flat.max() <= metrics.MAX_FREQ       # what sounds is in the scorer's range


def test_device_routes_refuse_what_they_cannot_take():
    from timbre_trap.utils import notes_csr_device, notes_to_activations
    case = note_case(549, 531)
    with pytest.raises(RuntimeError):                                              # no CPU fallback
        notes_to_activations(case['pitches'], case['intervals'], case['times'], MIDI_FREQS, device='cpu')
    with pytest.raises(RuntimeError):
        notes_csr_device(case['pitches'], case['intervals'], case['times'], device='cpu')
    for fn in (lambda p, iv: notes_to_multi_pitch(p, iv, case['times']),
               lambda p, iv: notes_to_activations(p, iv, case['times'], MIDI_FREQS, device='cpu'),
               lambda p, iv: notes_csr_device(p, iv, case['times'], device='cpu')):
        with pytest.raises(ValueError):                                            # one interval per pitch
            fn(case['pitches'][:-1], case['intervals'])


def test_dataset_stand_in_has_the_static_method():
    from timbre_trap import datasets
    if datasets.REFERENCE_DATASETS is None:
        assert issubclass(datasets.NoteDataset, datasets.PitchDataset)
        sets, times, _ = golden_sets()
        s = sets['b']
        assert same_lists(datasets.NoteDataset.notes_to_multi_pitch(s['pitches'], s['intervals'], times), s['lists'])
    assert hasattr(datasets.NoteDataset, 'notes_to_multi_pitch')
