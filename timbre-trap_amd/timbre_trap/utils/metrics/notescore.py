"""
The note-level score: precision / recall / F-measure of estimated against reference notes, with and without the offset criterion, in
the manner of ``mir_eval.transcription``, which the reference never calls and which is absent here too.  ``note_counts`` /
``note_metrics`` restate the published algorithm on the host: PARITY UNPINNED against the package, pinned by known answers and by an
independent maximum-matching routine (tests/test_notescore_restatement.py).
``note_counts_device`` / ``note_metrics_device`` give the same counts, integer for integer, for estimated notes that stay on the device
(csrc/notescore.hip: onset windows by binary search, connected components by label propagation, one matching per component).
"""

from collections import namedtuple

import numpy as np
import torch

from ... import _hip
from ..events import NoteEvents

NoteCounts = namedtuple('NoteCounts', ('n_ref', 'n_est', 'tp', 'tp_no_offset'))
NoteCounts.__doc__ = """The integers the note-level scores are formed from (``tp`` is None without the offset criterion)."""
DeviceNoteCounts = namedtuple('DeviceNoteCounts', ('n_ref', 'n_est', 'tp', 'tp_no_offset', 'n_fallback'))
DeviceNoteCounts.__doc__ = """``NoteCounts`` per batch item as int64 device tensors [B], and how many items were counted on the host."""

_NOTE_WINDOW_SLACK = 1e-4     # rnd(d) <= tol implies d <= tol + 0.5e-4: candidates are looked for this far beyond the onset tolerance


def _note_arrays(pitches, intervals, what):
    p = np.asarray(pitches, dtype=np.float64).ravel()
    iv = np.asarray(intervals, dtype=np.float64).reshape(-1, 2)
    if len(p) != len(iv):
        raise ValueError('%s pitches (%d) and intervals (%d) must hold one entry per note' % (what, len(p), len(iv)))
    return p, iv


def _note_pairs(ref_p, ref_iv, est_p, est_iv, onset_tolerance, pitch_tolerance, offset_ratio, offset_min_tolerance):
    """THE RULE.  -> (i, k, offset_ok): the onset pairs (reference i, estimate k), ascending in i, and which of them are offset pairs
    too (None without ``offset_ratio``).  Only pairs inside the widened onset window are looked at; no other can pass."""
    order = np.argsort(est_iv[:, 0], kind='stable')                       # NaN onsets last
    est_on = est_iv[order, 0]
    lo = np.searchsorted(est_on, ref_iv[:, 0] - (onset_tolerance + _NOTE_WINDOW_SLACK), side='left')
    hi = np.maximum(np.searchsorted(est_on, ref_iv[:, 0] + (onset_tolerance + _NOTE_WINDOW_SLACK), side='right'), lo)
    n = hi - lo
    i = np.repeat(np.arange(len(ref_p)), n)
    k = order[np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n) + np.repeat(lo, n)]
    with np.errstate(invalid='ignore'):                                   # inf - inf: a NaN, and a NaN makes every compare false
        onset_ok = (np.around(np.abs(ref_iv[i, 0] - est_iv[k, 0]), 4) <= onset_tolerance) & (np.abs(ref_p[i] - est_p[k]) <= pitch_tolerance)
        i, k = i[onset_ok], k[onset_ok]
        if offset_ratio is None:
            return i, k, None
        tolerance = np.maximum(offset_ratio * (ref_iv[i, 1] - ref_iv[i, 0]), offset_min_tolerance)
        return i, k, np.around(np.abs(ref_iv[i, 1] - est_iv[k, 1]), 4) <= tolerance


def _kuhn(n_ref, n_est, i, k):
    """Size of a maximum matching of the bipartite graph with edges (i[.], k[.]), ``i`` ascending: Kuhn's augmenting paths as in
    ``multipitch._max_matching``, with an explicit stack (a chain of notes may be thousands long)."""
    if len(i) == 0:
        return 0
    start = np.searchsorted(i, np.arange(n_ref + 1)).tolist()
    adj = k.tolist()
    match = [-1] * n_est
    count = 0
    for root in range(n_ref):
        if start[root] == start[root + 1]:
            continue
        seen = set()
        stack, chosen, pos = [root], [], {root: start[root]}
        while stack:
            r = stack[-1]
            at = pos[r]
            while at < start[r + 1] and adj[at] in seen:
                at += 1
            if at == start[r + 1]:                                        # r has no untried estimate left: back to its caller
                stack.pop()
                if chosen:
                    chosen.pop()
                continue
            e = adj[at]
            pos[r] = at + 1
            seen.add(e)
            chosen.append(e)
            if match[e] < 0:                                              # a free estimate: flip the path
                for rr, ee in zip(stack, chosen):
                    match[ee] = rr
                count += 1
                break
            stack.append(match[e])
            pos[match[e]] = start[match[e]]
    return count


def note_counts(ref_pitches, ref_intervals, est_pitches, est_intervals, onset_tolerance=0.05, pitch_tolerance=0.5, offset_ratio=0.2,
                offset_min_tolerance=0.05):
    """
    The integers behind ``note_metrics``: ``NoteCounts(n_ref, n_est, tp, tp_no_offset)``; ``tp`` is None when ``offset_ratio`` is None.
    """
    ref_p, ref_iv = _note_arrays(ref_pitches, ref_intervals, 'reference')
    est_p, est_iv = _note_arrays(est_pitches, est_intervals, 'estimated')
    n_ref, n_est = len(ref_p), len(est_p)
    if n_ref == 0 or n_est == 0:
        return NoteCounts(n_ref, n_est, None if offset_ratio is None else 0, 0)
    i, k, offset_ok = _note_pairs(ref_p, ref_iv, est_p, est_iv, onset_tolerance, pitch_tolerance, offset_ratio, offset_min_tolerance)
    tp = None if offset_ratio is None else _kuhn(n_ref, n_est, i[offset_ok], k[offset_ok])
    return NoteCounts(n_ref, n_est, tp, _kuhn(n_ref, n_est, i, k))


def _note_prf(tp, n_ref, n_est):
    """Precision, recall and F-measure from the integer counts, in float64."""
    tp, n_ref, n_est = np.float64(tp), np.float64(n_ref), np.float64(n_est)
    precision = tp / n_est if n_est > 0 else 0.0
    recall = tp / n_ref if n_ref > 0 else 0.0
    f_measure = 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
    return float(precision), float(recall), float(f_measure)


def _note_scores(counts):
    out = {}
    for suffix, tp in (('', counts.tp), ('_no_offset', counts.tp_no_offset)):
        if tp is not None:
            for key, v in zip(('Precision', 'Recall', 'F-measure'), _note_prf(tp, counts.n_ref, counts.n_est)):
                out[key + suffix] = v
    return out


def note_metrics(ref_pitches, ref_intervals, est_pitches, est_intervals, onset_tolerance=0.05, pitch_tolerance=0.5, offset_ratio=0.2,
                 offset_min_tolerance=0.05):
    """
    Note-level precision, recall and F-measure of estimated against reference notes, modelled on
    ``mir_eval.transcription.match_notes`` / ``precision_recall_f1_overlap`` AS RECALLED -- the package is not installed and there is
    no network, so PARITY IS UNPINNED against it; this function is the yardstick everything else in the package is compared with.

    Notes are (pitch, onset, offset) in float64: ``*_pitches`` (L) in MIDI numbers, ``*_intervals`` (L, 2) in seconds.  With
    ``rnd(x) = np.around(x, 4) = rint(x * 1e4) / 1e4``, reference note i and estimated note k are an ONSET PAIR when both

        rnd(|on_i - on_k|) <= onset_tolerance        and        |p_i - p_k| <= pitch_tolerance   (semitones)

    and additionally an OFFSET PAIR when ``rnd(|off_i - off_k|) <= max(offset_ratio * (off_i - on_i), offset_min_tolerance)``.  All
    compares are float64, and a NaN anywhere makes the compare false: such a note never matches but still counts.  ``tp_no_offset`` is
    the size of a maximum matching of the onset pairs, ``tp`` of the pairs that are both; precision = tp / n_est, recall = tp / n_ref
    (0 for a zero denominator), F-measure = 2 P R / (P + R) (0 when both are 0).

    Two deliberate differences from mir_eval.  Pitch is compared in MIDI numbers, not as 1200 |log2(f_i / f_k)| cents of Hz values: the
    device can then reproduce the verdict bit for bit, and the two forms differ only for pitches exactly at the tolerance.  The average
    overlap ratio is left out: it depends on WHICH maximum matching is chosen, and that is not unique.

    Returns ``Precision``, ``Recall``, ``F-measure`` and the same three with the suffix ``_no_offset``; ``offset_ratio=None`` returns
    only the latter.
    """
    return _note_scores(note_counts(ref_pitches, ref_intervals, est_pitches, est_intervals, onset_tolerance, pitch_tolerance, offset_ratio,
                                    offset_min_tolerance))


# ---- on the device (csrc/notescore.hip) ----------------------------------------------------------------------------------------

NOTESCORE_MAX = 64        # references / estimates per connected component the matching kernel holds (= tt_notescore_max(), checked on first use)
NOTESCORE_ROUNDS = 32     # label-propagation rounds before an item that has not settled goes to the host


def _note_device_four(notes, what):
    if not (isinstance(notes, (tuple, list)) and len(notes) == 4 and all(isinstance(t, torch.Tensor) for t in notes)):
        raise RuntimeError('%s notes for scoring on the device are a NoteEvents or four GPU tensors (item int32, pitch, onset, offset '
                           'float64); the host function note_metrics takes arrays' % what)
    _hip.require_cuda(*notes)
    item, pitch, onset, offset = notes
    if item.dtype != torch.int32 or any(t.dtype != torch.float64 for t in (pitch, onset, offset)):
        raise ValueError('%s notes must be (item int32, pitch float64, onset float64, offset float64)' % what)
    if any(t.dim() != 1 or t.shape != item.shape or t.device != item.device for t in (item, pitch, onset, offset)):
        raise ValueError('%s notes must be four 1-d tensors of one length on one device' % what)
    return tuple(t.detach().contiguous() for t in notes)


def _note_event_times(events, hop_seconds):
    """Onset / offset seconds of a ``NoteEvents`` on the device, in the arithmetic of ``events_to_notes``."""
    if hop_seconds is None:
        raise ValueError('hop_seconds is required to place NoteEvents in time')
    _hip.require_cuda(events.item, events.onset, events.end, events.pitch)
    if isinstance(hop_seconds, (tuple, list)):
        hop_length, sample_rate = hop_seconds
        integral = isinstance(hop_length, (int, np.integer))
        hop_int, hop_mul, denom = (int(hop_length), 1.0, float(sample_rate)) if integral else (1, float(hop_length), float(sample_rate))
    else:
        hop_int, hop_mul, denom = 1, float(hop_seconds), 1.0
    n, dev = events.onset.numel(), events.onset.device
    onset = torch.empty(n, dtype=torch.float64, device=dev)
    offset = torch.empty_like(onset)
    on_f, end_f = events.onset.to(torch.int32).contiguous(), events.end.to(torch.int32).contiguous()
    if n:
        with torch.cuda.device(dev):
            _hip.check(_hip.lib().tt_notescore_times(_hip.ptr(on_f), _hip.ptr(end_f), n, hop_int, hop_mul, denom, _hip.ptr(onset),
                                                     _hip.ptr(offset), _hip.stream_ptr()), 'tt_notescore_times')
    return onset, offset


def _note_sorted(notes, n_items):
    """Notes ordered by (item, onset) -- torch's stable sort, NaN onsets last -- and the bounds of every item's run (int64 [B + 1])."""
    item, pitch, onset, offset = notes
    by_onset = torch.argsort(onset, stable=True)
    perm = by_onset[torch.argsort(item[by_onset], stable=True)]
    item = item[perm].contiguous()
    seg = torch.searchsorted(item, torch.arange(n_items + 1, dtype=torch.int32, device=item.device)).to(torch.int64)
    return (item, pitch[perm].contiguous(), onset[perm].contiguous(), offset[perm].contiguous()), seg


def _note_counts_device(est, ref, hop_seconds, n_items, onset_tolerance, pitch_tolerance, offset_ratio, offset_min_tolerance):
    """-> (DeviceNoteCounts, the same four counts as an int64 ndarray [B, 4])."""
    if isinstance(est, NoteEvents):
        est = (est.item, est.pitch) + _note_event_times(est, hop_seconds)
    est = _note_device_four(est, 'estimated')
    dev = est[0].device
    if isinstance(ref, (tuple, list)) and len(ref) == 4 and all(isinstance(t, torch.Tensor) for t in ref):
        ref = _note_device_four(ref, 'reference')
        if ref[0].device != dev:
            raise RuntimeError('estimated notes are on %s, reference notes on %s' % (dev, ref[0].device))
        if n_items is None:                                               # one value comes back
            n_items = int(torch.cat([ref[0].max().reshape(1) if ref[0].numel() else ref[0].new_zeros(1),
                                     est[0].max().reshape(1) if est[0].numel() else est[0].new_zeros(1)]).max()) + 1
    else:
        pairs = [_note_arrays(p, iv, 'reference') for p, iv in ref]
        if n_items is None:
            n_items = len(pairs)
        if len(pairs) > n_items:
            raise ValueError('%d reference note lists for %d items' % (len(pairs), n_items))
        sizes = [len(p) for p, _ in pairs]
        flat = np.empty((3, sum(sizes)))                                  # the one upload: pitch, onset, offset rows
        if sum(sizes):
            flat[0] = np.concatenate([p for p, _ in pairs])
            flat[1:] = np.concatenate([iv for _, iv in pairs]).T
        up = torch.from_numpy(flat).to(dev)
        item = torch.from_numpy(np.repeat(np.arange(len(pairs), dtype=np.int32), sizes)).to(dev)
        ref = (item, up[0], up[1], up[2])
    n_items = int(n_items)
    if n_items < 1:
        raise ValueError('n_items must be at least 1 (got %d)' % n_items)
    lib = _hip.lib()
    if lib.tt_notescore_max() != NOTESCORE_MAX:
        raise RuntimeError('libttrap_hip.so was built with a component capacity of %d, metrics.NOTESCORE_MAX says %d'
                           % (lib.tt_notescore_max(), NOTESCORE_MAX))
    ratio = 0.0 if offset_ratio is None else float(offset_ratio)
    (r_item, r_p, r_on, r_off), r_seg = _note_sorted(ref, n_items)
    (e_item, e_p, e_on, e_off), e_seg = _note_sorted(est, n_items)
    R, E, B = r_item.numel(), e_item.numel(), n_items
    if R + E >= 2 ** 31:
        raise ValueError('more than 2^31 notes')
    if R == 0 or E == 0:
        sums = torch.zeros(B, 5, dtype=torch.int64, device=dev)
        sums[:, 0], sums[:, 1] = r_seg[1:] - r_seg[:-1], e_seg[1:] - e_seg[:-1]
        host = sums.cpu().numpy()
    else:
        N = R + E
        lo, hi = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
        label, other = torch.arange(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
        changed = torch.zeros(NOTESCORE_ROUNDS, dtype=torch.int32, device=dev)
        item_mark = torch.zeros(B, dtype=torch.int32, device=dev)
        tp, tp_no = torch.empty(R, dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.int32, device=dev)
        sums = torch.empty(B, 5, dtype=torch.int64, device=dev)
        p = _hip.ptr
        with torch.cuda.device(dev):
            st = _hip.stream_ptr()
            _hip.check(lib.tt_notescore_ranges(p(r_item), p(r_on), R, p(e_item), p(e_on), E, p(r_seg), p(e_seg), B, float(onset_tolerance),
                                               p(lo), p(hi), st), 'tt_notescore_ranges')
            settled = False
            for rnd in range(NOTESCORE_ROUNDS):
                _hip.check(lib.tt_notescore_labels(p(r_item), p(r_p), p(r_on), R, p(e_item), p(e_p), p(e_on), E, p(lo), p(hi),
                                                   float(onset_tolerance), float(pitch_tolerance), p(label), p(other), p(changed[rnd:]),
                                                   p(item_mark), B, rnd + 1, st), 'tt_notescore_labels')
                label, other = other, label
                if not int(changed[rnd]):                                 # the one flag read per round
                    settled = True
                    break
            # an item whose labels still moved in the last round allowed is counted on the host
            item_flag = torch.zeros(B, dtype=torch.int32, device=dev) if settled else (item_mark == NOTESCORE_ROUNDS).to(torch.int32)
            r_lab, r_perm = torch.sort(label[:R], stable=True)
            e_lab, e_perm = torch.sort(label[R:], stable=True)
            r_perm, e_perm = r_perm.to(torch.int32), e_perm.to(torch.int32)
            _hip.check(lib.tt_notescore_match(p(label), p(r_lab), p(r_perm), p(e_lab), p(e_perm), p(r_item), p(r_p), p(r_on), p(r_off), R,
                                              p(e_p), p(e_on), p(e_off), E, float(onset_tolerance), float(pitch_tolerance), ratio,
                                              float(offset_min_tolerance), p(tp), p(tp_no), p(item_flag), B, st), 'tt_notescore_match')
            _hip.check(lib.tt_notescore_sums(p(tp), p(tp_no), R, E, p(r_seg), p(e_seg), p(item_flag), B, p(sums), st), 'tt_notescore_sums')
        host = sums.cpu().numpy()                                         # the one copy back: five integers per item
    flagged = np.flatnonzero(host[:, 4])
    if len(flagged):
        # over the kernel's capacity, or labels that did not settle: these items alone are counted by the host function from their own notes
        rs, es = r_seg.cpu().numpy(), e_seg.cpu().numpy()
        for b in flagged:
            r, e = slice(rs[b], rs[b + 1]), slice(es[b], es[b + 1])
            got = note_counts(r_p[r].cpu().numpy(), torch.stack([r_on[r], r_off[r]], 1).cpu().numpy(), e_p[e].cpu().numpy(),
                              torch.stack([e_on[e], e_off[e]], 1).cpu().numpy(), onset_tolerance, pitch_tolerance, offset_ratio,
                              offset_min_tolerance)
            host[b, 2], host[b, 3] = got.tp or 0, got.tp_no_offset
        sums = torch.from_numpy(host).to(dev)
    counts = DeviceNoteCounts(sums[:, 0], sums[:, 1], None if offset_ratio is None else sums[:, 2], sums[:, 3], len(flagged))
    return counts, host[:, :4]


def note_counts_device(est, ref, hop_seconds=None, n_items=None, onset_tolerance=0.05, pitch_tolerance=0.5, offset_ratio=0.2,
                       offset_min_tolerance=0.05):
    """
    ``note_counts`` per batch item for estimated notes that are on the device: ``DeviceNoteCounts`` of int64 device tensors [B]
    ``n_ref``, ``n_est``, ``tp`` (None when ``offset_ratio`` is None), ``tp_no_offset`` -- equal to the host function's integers -- and
    ``n_fallback``, the number of items that were counted by the host function instead.

    ``est``: a ``NoteEvents`` (then ``hop_seconds`` is required: seconds per frame or ``(hop_length, sample_rate)``, and the times are
    formed on the device in the arithmetic of ``events_to_notes``), or four device tensors ``(item int32, pitch float64 MIDI, onset
    float64 s, offset float64 s)`` in any order of notes.  ``ref``: a list over items of host ``(pitches, intervals)`` with pitches in
    MIDI numbers (uploaded once), or the same four device tensors (then ``n_items`` saves reading the largest item back).  Notes of an
    item outside [0, B) are ignored.  CPU tensors for ``est`` raise ``RuntimeError``: there is no CPU fallback.

    On the device: both lists sorted by (item, onset); per note the slice of the other list inside the onset window (binary search);
    connected components of the onset pairs by minimum-label propagation, one flag read per round; one wavefront per component for the
    two maximum matchings; integer sums per item; ONE copy of five integers per item back.  An item with a component of more than
    ``NOTESCORE_MAX`` references or estimates, or whose labels have not settled after ``NOTESCORE_ROUNDS`` rounds, is downloaded and
    counted by ``note_counts``.
    """
    return _note_counts_device(est, ref, hop_seconds, n_items, onset_tolerance, pitch_tolerance, offset_ratio, offset_min_tolerance)[0]


def note_metrics_device(est, ref, hop_seconds=None, n_items=None, onset_tolerance=0.05, pitch_tolerance=0.5, offset_ratio=0.2,
                        offset_min_tolerance=0.05):
    """The dictionary of ``note_metrics`` for every batch item (a list of B dicts), from ``note_counts_device``'s integers: the same
    float64 values, bit for bit."""
    host = _note_counts_device(est, ref, hop_seconds, n_items, onset_tolerance, pitch_tolerance, offset_ratio, offset_min_tolerance)[1]
    return [_note_scores(NoteCounts(int(n_ref), int(n_est), None if offset_ratio is None else int(tp), int(tp_no)))
            for n_ref, n_est, tp, tp_no in host]
