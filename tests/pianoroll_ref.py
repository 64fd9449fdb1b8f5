"""The piano roll and frame count rule (include/mt3_hip.h, "piano rolls and frame counts") in its plainest form: a Python
loop over the notes with slice adds in float64, boolean arrays for the counts.  The yardstick of tests/test_gpu_pianoroll.py;
itself pinned by the hand-computed literals of tests/test_pianoroll_ref.py.  Not the product: nothing in mt3_amd/ imports it."""
import numpy as np

PITCHES = 128
MIN_NOTE_SECONDS = 0.05


def pianoroll(ns, fps, is_drum):
    """mt3/metrics_utils.py:149-171 with pretty_midi's get_piano_roll written out: float64 [128, F]"""
    spans = []
    for n in ns.notes:
        start, end = float(n.start_time), float(n.end_time)
        if is_drum or end - start < MIN_NOTE_SECONDS:
            end = start + MIN_NOTE_SECONDS               # on a copy: ns keeps its times
        spans.append((start, end, n))
    if not spans:
        return np.zeros((PITCHES, 0), np.float64)
    roll = np.zeros((PITCHES, int(fps * max(end for _, end, _ in spans))), np.float64)
    for start, end, n in spans:
        if n.is_drum and not is_drum:
            continue                                     # a drum instrument renders as zeros; it did count for the width
        roll[n.pitch, int(start * fps):int(end * fps)] += n.velocity
    return roll


def frame_counts(ref_roll, est_roll, velocity_threshold):
    """(TP, FP, FN) of mt3/metrics_utils.py:174-196 before sklearn's ratios"""
    width = max(ref_roll.shape[1], est_roll.shape[1])
    ref = np.pad(ref_roll, [(0, 0), (0, width - ref_roll.shape[1])], mode="constant")
    est = np.pad(est_roll, [(0, 0), (0, width - est_roll.shape[1])], mode="constant")
    ref_on, est_on = ref > velocity_threshold, est > 0
    return int((ref_on & est_on).sum()), int((~ref_on & est_on).sum()), int((ref_on & ~est_on).sum())


def precision_recall_f1(tp, fp, fn):
    """sklearn's precision_recall_fscore_support for the positive class: 0.0 where a denominator is 0"""
    p = tp / (tp + fp) if tp + fp else 0.0
    r = tp / (tp + fn) if tp + fn else 0.0
    return p, r, (2 * p * r / (p + r) if p + r else 0.0)


def frame_metrics(ref_roll, est_roll, velocity_threshold):
    return precision_recall_f1(*frame_counts(ref_roll, est_roll, velocity_threshold))
