"""
``timbre_trap.datasets``.  File parsing, downloads and the dataset classes are outside the accelerated path (DESIGN.md
section 6): when a reference checkout is on ``sys.path`` after this package, its dataset modules are used as they are -- this
package's ``__path__`` is extended with the reference directory, so ``timbre_trap.datasets.MixedMultiPitch`` etc. resolve
there and the base classes below are the reference's.  Without a reference checkout only the path-adjacent pieces exist
(SURVEY.md section 8f, rows f3 / f4): the target and note helpers as static methods and the slicing arithmetic.
"""

from pkgutil import extend_path

__path__ = extend_path(__path__, __name__)

from ..utils.audio import prepare_audio
from ..utils.notes import notes_to_activations, notes_to_multi_pitch
from ..utils.pitch import pitch_to_activations
from ..utils.slicing import ExcerptSlicer
from ..utils.targets import activations_to_multi_pitch, multi_pitch_to_activations

REFERENCE_DATASETS = None
try:
    from .BaseDataset import BaseDataset, ComboDataset, StemMixingDataset
    from .AudioDataset import AudioDataset
    from .PitchDataset import PitchDataset
    from .MPEDataset import MPEDataset
    from .NoteDataset import NoteDataset
    from .AMTDataset import AMTDataset
    REFERENCE_DATASETS = BaseDataset.__module__
except Exception as _e:                          # no reference on the path, or one of its third-party imports is missing
    REFERENCE_DATASETS = None
    _reason = repr(_e)

    class PitchDataset(ExcerptSlicer):
        """
        Stand-in with the reference's static target helpers (``PitchDataset.multi_pitch_to_activations`` /
        ``activations_to_multi_pitch``, device kernels) and slicing methods (``slice_times``, ``resample_multi_pitch``);
        construct it with the CQT object and excerpt length instead of a dataset directory.  The static ``pitch_to_activations``
        is the two lines of ``__getitem__`` that turn a track's annotations into an item's targets (``PitchDataset.py:182-185``)
        on the device; ``utils.PitchBank`` does the same for whole batches from annotations uploaded once.
        """

        multi_pitch_to_activations = staticmethod(multi_pitch_to_activations)
        pitch_to_activations = staticmethod(pitch_to_activations)
        activations_to_multi_pitch = staticmethod(activations_to_multi_pitch)

    class NoteDataset(PitchDataset):
        """
        Stand-in with the reference's static ``notes_to_multi_pitch(pitches, intervals, times)`` (``NoteDataset.py:93-123``; the
        vectorised host function, same lists) and, as the static ``notes_to_activations``, the two lines of ``__getitem__`` that turn
        a track's notes into its targets (``NoteDataset.py:81-84``) on the device.
        """

        notes_to_multi_pitch = staticmethod(notes_to_multi_pitch)
        notes_to_activations = staticmethod(notes_to_activations)

    class AudioDataset(ExcerptSlicer):
        """
        Stand-in with the reference's ``slice_audio`` arithmetic and, as the static ``prepare_audio(waveform, fs, sample_rate)``,
        the mono mix, sample-rate conversion and inf-norm of ``get_audio`` (``AudioDataset.py:70-77``) on the device.
        """

        prepare_audio = staticmethod(prepare_audio)

    # the mixing wrapper's stand-in: the same draws, whole batches formed on the device (utils/mixing.py)
    from ..utils.mixing import AudioBank, StemMixer, StemSource
