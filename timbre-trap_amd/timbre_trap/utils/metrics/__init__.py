"""
Scoring next to the hot path: what reference ``experiments/evaluate.py:113-127`` computes per track
from the outputs of the path, and a note-level score beside it.  One module per score family:

  multipitch   the host yardstick: frame-level multi-pitch precision / recall / accuracy / errors (NumPy only, float64)
  mpe          the same scores, bit for bit, from activations that stay on the device (csrc/mpe.hip)
  sdr          the reconstruction SDR: host yardstick, device kernels (csrc/sdr.hip) and the ``SignalDistortionRatio`` module
  notescore    note-level precision / recall / F-measure: host rule and the same integers on the device (csrc/notescore.hip)
  evaluator    ``MultipitchEvaluator``, the reference's result tracker over all of them

The packages the reference delegates to (``mir_eval``, ``torchmetrics``) are absent from this image; each module says what it restates
and how the restatement is pinned.  Every host function is the float64 yardstick its device counterpart is tested against.
"""

from .multipitch import (MAX_FREQ, MIN_FREQ, _max_matching, _nearest_frame_index, _scores_from_sums, frequencies_to_midi, match_count,
                         midi_to_chroma, multipitch_metrics, resample_multipitch)
from .mpe import (MPE_MAX_EST, MPE_MAX_REF, _mpe_activations, _mpe_bin_tables, mpe_compact, multipitch_counts_device,
                  multipitch_counts_device_notes, multipitch_counts_device_track, multipitch_metrics_device, multipitch_metrics_device_notes,
                  multipitch_metrics_device_track)
from .sdr import (SDR_CHUNK, SDR_MAX_FILTER, SignalDistortionRatio, sdr_correlations, signal_distortion_ratio,
                  signal_distortion_ratio_device)
from .notescore import (NOTESCORE_MAX, NOTESCORE_ROUNDS, DeviceNoteCounts, NoteCounts, _kuhn, note_counts, note_counts_device, note_metrics,
                        note_metrics_device)
from .evaluator import MultipitchEvaluator

__all__ = ['resample_multipitch', 'frequencies_to_midi', 'match_count', 'multipitch_metrics', 'MultipitchEvaluator',
           'multipitch_counts_device', 'multipitch_metrics_device', 'multipitch_counts_device_notes',
           'multipitch_metrics_device_notes', 'multipitch_counts_device_track', 'multipitch_metrics_device_track', 'mpe_compact', 'MPE_MAX_EST', 'MPE_MAX_REF',
           'signal_distortion_ratio', 'signal_distortion_ratio_device', 'SignalDistortionRatio', 'SDR_CHUNK', 'SDR_MAX_FILTER',
           'note_counts', 'note_metrics', 'note_counts_device', 'note_metrics_device', 'NoteCounts', 'DeviceNoteCounts', 'NOTESCORE_MAX',
           'NOTESCORE_ROUNDS']
