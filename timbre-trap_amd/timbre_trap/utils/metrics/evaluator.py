"""``MultipitchEvaluator``: the reference's result tracker (``timbre_trap/utils/experiments.py:277-396``) over the scores of this package
-- frame lists on the host, activations on the device against three forms of reference, note events on the device."""

import sys
from copy import deepcopy

import numpy as np
import torch

from ..events import NoteEvents
from .mpe import multipitch_metrics_device, multipitch_metrics_device_notes, multipitch_metrics_device_track
from .multipitch import multipitch_metrics
from .notescore import note_metrics_device


class MultipitchEvaluator(object):
    """
    Result tracker with the reference's interface (``timbre_trap/utils/experiments.py:277-396``): ``evaluate`` returns the
    scores of ``multipitch_metrics`` under lower-case keys prefixed ``mpe/`` plus ``mpe/f1-score = 2 P R / (P + R + eps)``; ``append_results`` /
    ``average_results`` accumulate per-track dictionaries and give rounded means and standard deviations.
    """

    def __init__(self, tolerance=0.5):
        self.tolerance = tolerance
        self.results = None
        self.reset_results()

    def reset_results(self):
        self.results = {}

    def append_results(self, results):
        for key in results.keys():
            if key in self.results.keys():
                self.results[key] = np.append(self.results[key], results[key])
            else:
                self.results[key] = np.array([results[key]])

    def average_results(self):
        mean, std_dev = deepcopy(self.results), deepcopy(self.results)
        for key in self.results.keys():
            mean[key] = round(np.mean(mean[key]), 5)
            std_dev[key] = round(np.std(std_dev[key]), 5)
        return mean, std_dev

    @staticmethod
    def _tagged(scores):
        results = {k.lower(): v for k, v in scores.items()}
        pr, rc = results['precision'], results['recall']
        results['f1-score'] = 2 * pr * rc / (pr + rc + sys.float_info.epsilon)
        return {'mpe/' + k: v for k, v in results.items()}

    def evaluate(self, times_est, multi_pitch_est, times_ref, multi_pitch_ref):
        return self._tagged(multipitch_metrics(times_ref, multi_pitch_ref, times_est, multi_pitch_est, window=self.tolerance))

    def evaluate_activations(self, times_est, activations, midi_freqs, times_ref, multi_pitch_ref, n_valid_bins=0):
        """
        ``evaluate`` for activations that are still on the device -- the (F, T) or (1, F, T) tensor ``model.to_activations``
        returned -- instead of frame lists: the same ``mpe/...`` dictionary as ``evaluate(times_est,
        activations_to_multi_pitch(masked activations, midi_freqs, peaks_only=True), times_ref, multi_pitch_ref)``, bit for bit,
        without downloading the map (reference ``experiments/evaluate.py:100-116``).  ``n_valid_bins`` > 0 zeroes the rows from
        that bin upwards first (``evaluate.py:107-112``).
        """
        return self._tagged(multipitch_metrics_device(times_ref, multi_pitch_ref, times_est, activations, midi_freqs,
                                                      window=self.tolerance, n_valid_bins=n_valid_bins))

    def evaluate_notes(self, times_est, activations, midi_freqs, times_ref, pitches_hz, intervals, n_valid_bins=0):
        """
        ``evaluate_activations`` for a reference given as notes -- ``pitches_hz`` (L), ``intervals`` (L, 2) -- instead of frame lists:
        the dictionary of ``evaluate_activations(..., times_ref, notes_to_multi_pitch(pitches_hz, intervals, times_ref))``, bit for
        bit, with the reference lists built on the device too (reference ``experiments/evaluate.py:67-75,100-116`` on a ``NoteDataset``).
        """
        return self._tagged(multipitch_metrics_device_notes(times_ref, pitches_hz, intervals, times_est, activations, midi_freqs,
                                                            window=self.tolerance, n_valid_bins=n_valid_bins))

    def evaluate_track(self, times_est, activations, midi_freqs, bank, track_id, n_valid_bins=0):
        """
        ``evaluate_activations`` for a reference kept on the device in a ``utils.pitch.PitchBank``: the dictionary of
        ``evaluate_activations(..., *bank.tracks[track_id])``, bit for bit, without flattening and uploading the track's lists again
        (reference ``experiments/evaluate.py:76-78,100-116`` on an ``MPEDataset``).
        """
        return self._tagged(multipitch_metrics_device_track(bank, track_id, times_est, activations, midi_freqs, window=self.tolerance,
                                                            n_valid_bins=n_valid_bins))

    def evaluate_events(self, events, hop_seconds, pitches, intervals, item=0, **tolerances):
        """
        Note-level scores of the notes of batch item ``item`` of ``events`` (a ``NoteEvents`` on the device) against one track's
        annotation -- ``pitches`` (L) in MIDI numbers, ``intervals`` (L, 2) in seconds, as ``NoteDataset.get_ground_truth`` returns them
        with pitches converted to MIDI: the six scores of ``note_metrics_device`` under lower-case keys prefixed ``note/``, ready for
        ``append_results``.  ``hop_seconds``: as for ``events_to_notes``.  The pitch tolerance defaults to the evaluator's.
        """
        tolerances.setdefault('pitch_tolerance', self.tolerance)
        sel = events.item == int(item)
        est = NoteEvents(*(f[sel] for f in events))
        est = est._replace(item=torch.zeros_like(est.item))
        scores = note_metrics_device(est, [(pitches, intervals)], hop_seconds, **tolerances)[0]
        return {'note/' + k.lower(): v for k, v in scores.items()}
