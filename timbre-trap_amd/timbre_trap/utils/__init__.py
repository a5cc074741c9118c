"""
``timbre_trap.utils``: the path-adjacent helpers of the reference package, implemented here (HIP kernels where the work is
device work), plus -- when a reference checkout is on ``sys.path`` after this package -- the reference's own host-only modules
this package does not replace (``data``: constants / download helpers, ``visualization``), re-exported under the reference's
names so that ``from timbre_trap.utils import *`` yields the same namespace as in the reference.

``audio`` has no module of the same name in the reference: it holds what ``AudioDataset.get_audio`` asks of torchaudio and torch
between a decoded file and the CQT (mono mix, sample-rate conversion, inf-norm) as device kernels -- ``resample``,
``prepare_audio`` -- with the float64 host yardstick ``resample_host`` and the tap design ``sinc_resample_kernel``.
"""

from pkgutil import extend_path

__path__ = extend_path(__path__, __name__)

from .optim import FusedAdamW
from .distributed import DataParallel, GradientSync, init_process_group_from_env, allreduce_gradients
from .experiments import (CosineWarmup, seed_everything, gradient_statistics, sum_gradient_norms, average_gradient_norms,
                          get_max_gradient, get_max_gradient_norm)
from .processing import to_array, debug_nans, filter_non_peaks, threshold, peaks_above
from .targets import multi_pitch_to_activations, activations_to_multi_pitch, hz_to_midi, midi_to_hz
from .slicing import slice_audio, slice_times, resample_multi_pitch, nearest_indices, ExcerptSlicer
from .metrics import (MultipitchEvaluator, multipitch_metrics, multipitch_metrics_device, multipitch_counts_device,
                      multipitch_metrics_device_notes, multipitch_counts_device_notes,
                      multipitch_metrics_device_track, multipitch_counts_device_track,
                      signal_distortion_ratio, signal_distortion_ratio_device, SignalDistortionRatio,
                      note_counts, note_metrics, note_counts_device, note_metrics_device, NoteCounts, DeviceNoteCounts)
from .notes import notes_to_multi_pitch, notes_csr_device, notes_to_activations, note_tiles
from .events import NoteEvents, note_events, events_to_notes, write_midi
from .contours import (NoteContours, note_contours, refined_pitches, refine_multi_pitch, activations_to_multi_pitch_refined,
                       contours_to_bends, write_midi_bends)
from .embedding import TSNEResult, TSNEState, tsne_joint_probabilities, tsne, latent_codes, plot_latents_device
from .pitch import PitchBank, pitch_to_activations, pitch_tiles
from .mixing import AudioBank, StemSource, StemMixer, mix_tiles, mix_targets
from .audio import sinc_resample_kernel, resample_host, resample, mix_resample, prepare_audio
from .trainloop import (make_schedulers, checkpoints_for, StepLogger, TrainingState, save_checkpoint, print_and_log,
                        log_gradient_norms, TRAIN_TAGS)

# reference-only host modules (found through the extended __path__; absent or missing a third-party dependency -> skipped)
REFERENCE_MODULES = {}
for _name in ('data', 'visualization'):
    try:
        _mod = __import__(__name__ + '.' + _name, fromlist=['*'])
    except Exception as _e:                      # ImportError, or a dependency of the reference module failing to import
        REFERENCE_MODULES[_name] = repr(_e)
        continue
    REFERENCE_MODULES[_name] = _mod.__file__
    for _k in getattr(_mod, '__all__', ()):
        globals()[_k] = getattr(_mod, _k)
del _name
