"""Maximum note matching for a whole job on the device (mt3_op_match_notes; the rule: include/mt3_hip.h, "note matching").

The device side of `metrics.match_notes`: every (reference notes, estimated notes, rule) problem of a job -- some tens per
(reference, estimate) pair, thousands per evaluation -- goes through ONE upload of the packed notes, ONE op call and ONE
copy of 4 bytes per problem back to the host.  The matchings themselves stay on the device unless asked for.  There is no
host fallback.
"""
from __future__ import annotations

import dataclasses
from typing import List, Optional, Sequence

import numpy as np

from . import _lib, note_arrays

RULE_DTYPE = np.dtype([("onset_tolerance", "<f8"), ("pitch_tolerance", "<f8"), ("offset_ratio", "<f8"),
                       ("offset_min_tolerance", "<f8"), ("strict", "<i4"), ("reserved", "<i4")])       # mt3_match_rule
PROBLEM_DTYPE = np.dtype([("ref0", "<i8"), ("est0", "<i8"), ("state0", "<i8"), ("n_ref", "<i4"), ("n_est", "<i4"),
                          ("rule", "<i4"), ("reserved", "<i4")])                                      # mt3_match_problem
REF_WORDS, EST_WORDS = 6, 2             # mt3_note_match_state_words: 6 n_ref + 2 n_est


@dataclasses.dataclass
class Problem:
    """One matching: the arguments of `metrics.match_notes`.  intervals [n, 2] (onset, offset) in seconds, pitches [n] in
    the unit the cents rule is to act on.  Problems that are handed the SAME array objects share their notes on the
    device (the onset-only, onset + offset and sweep problems of one track)."""
    ref_intervals: np.ndarray
    ref_pitches: np.ndarray
    est_intervals: np.ndarray
    est_pitches: np.ndarray
    onset_tolerance: float = 0.05
    pitch_tolerance: float = 50.0
    offset_ratio: Optional[float] = 0.2
    offset_min_tolerance: float = 0.05
    strict: bool = False

    def rule(self):
        return (float(self.onset_tolerance), float(self.pitch_tolerance),
                _lib.NOTE_MATCH_NO_OFFSET if self.offset_ratio is None else float(self.offset_ratio),
                float(self.offset_min_tolerance), 1 if self.strict else 0)


@dataclasses.dataclass
class Packed:
    """the host side of one op call"""
    notes: np.ndarray                   # float64 [3, n_notes]: onset | offset | log2(pitch)
    problems: np.ndarray                # PROBLEM_DTYPE [n_problems]
    rules: np.ndarray                   # RULE_DTYPE [n_rules]
    est_order: List[np.ndarray]         # per problem: position in the onset-sorted estimates -> the caller's index
    workspace_words: int


def pack(problems: Sequence[Problem]) -> Packed:
    """notes packed once per distinct (intervals, pitches) pair of array objects, estimates sorted stably by onset"""
    sides, order_of, chunks, at = {}, {}, [], 0

    def side(intervals, pitches, is_est):
        nonlocal at
        key = (id(intervals), id(pitches), is_est)
        if key in sides:
            return sides[key]
        iv = np.asarray(intervals, np.float64).reshape(-1, 2)
        pt = np.asarray(pitches, np.float64).reshape(-1)
        if len(iv) != len(pt):
            raise ValueError("%d intervals, %d pitches" % (len(iv), len(pt)))
        if not np.isfinite(iv).all():
            raise ValueError("note times must be finite")
        order = np.argsort(iv[:, 0], kind="stable") if is_est else np.arange(len(iv))
        with np.errstate(divide="ignore", invalid="ignore"):
            chunks.append(np.stack([iv[order, 0], iv[order, 1], np.log2(pt[order])]))
        sides[key] = (at, len(iv))
        order_of[key] = order
        at += len(iv)
        return sides[key]

    rules, table, est_order, words = {}, np.zeros(len(problems), PROBLEM_DTYPE), [], 0
    keep = []                           # the keys are ids: the arrays must outlive the packing
    for k, p in enumerate(problems):
        keep.append((p.ref_intervals, p.ref_pitches, p.est_intervals, p.est_pitches))
        r0, n_ref = side(p.ref_intervals, p.ref_pitches, False)
        e0, n_est = side(p.est_intervals, p.est_pitches, True)
        est_order.append(order_of[(id(p.est_intervals), id(p.est_pitches), True)])
        rule = p.rule()
        if not all(np.isfinite(v) and v >= 0 for v in rule[:2] + rule[3:4]) or \
                not (rule[2] == _lib.NOTE_MATCH_NO_OFFSET or (np.isfinite(rule[2]) and rule[2] >= 0)):
            raise ValueError("problem %d: tolerances must be finite and not negative, got %r" % (k, rule))
        table[k] = (r0, e0, words, n_ref, n_est, rules.setdefault(rule, len(rules)), 0)
        words += REF_WORDS * n_ref + EST_WORDS * n_est
    if len(rules) > _lib.NOTE_MATCH_MAX_RULES:
        raise ValueError("%d distinct rules in one job; the op takes %d" % (len(rules), _lib.NOTE_MATCH_MAX_RULES))
    rule_table = np.zeros(len(rules), RULE_DTYPE)
    for rule, i in rules.items():
        rule_table[i] = rule + (0,)
    notes = np.ascontiguousarray(np.concatenate(chunks, axis=1)) if chunks else np.zeros((3, 0), np.float64)
    return Packed(notes, table, rule_table, est_order, words)


def warm_words(packed: Packed, warm_start: Sequence) -> np.ndarray:
    """the workspace image that carries `warm_start`: per problem an int array [n_ref] of the caller's estimate indices
    (-1: free), or None.  Indices are translated to positions in the sorted estimates; a value outside the problem's
    estimates is passed on as it is, for the kernel to refuse."""
    image = np.full(packed.workspace_words, -1, np.int32)
    for k, (q, warm) in enumerate(zip(packed.problems, warm_start)):
        if warm is None:
            continue
        warm = np.asarray(warm, np.int64).reshape(-1)
        if len(warm) != q["n_ref"]:
            raise ValueError("problem %d: %d warm-start entries for %d reference notes" % (k, len(warm), q["n_ref"]))
        inverse = np.empty(q["n_est"], np.int64)
        inverse[packed.est_order[k]] = np.arange(q["n_est"])
        inside = (warm >= 0) & (warm < q["n_est"])
        sorted_pos = np.clip(warm, -2 ** 31, 2 ** 31 - 1)
        sorted_pos[inside] = inverse[warm[inside]]
        image[q["state0"]: q["state0"] + q["n_ref"]] = sorted_pos
    return image


class Matching:
    """What `match` returns.  counts: int64 numpy [n_problems].  mates[k]: int32 CUDA tensor [n_ref_k], a view of the
    workspace: the position, in problem k's onset-sorted estimates, of the estimate matched to reference note i, or -1.
    pairs(k) copies one matching back and translates it to the caller's indices."""

    def __init__(self, counts, workspace, packed: Packed):
        self.counts, self.workspace, self._packed = counts, workspace, packed
        self.mates = [workspace[int(q["state0"]): int(q["state0"]) + int(q["n_ref"])] for q in packed.problems]

    def pairs(self, k: int) -> np.ndarray:
        """int64 [matched, 2]: (reference index, estimate index) in the order the caller's arrays have"""
        return pairs_of(self.mates[k].cpu().numpy(), self._packed.est_order[k])

    def all_pairs(self) -> list:
        """pairs(k) of every problem, from one copy of the workspace"""
        host = self.workspace.cpu().numpy()
        return [pairs_of(host[int(q["state0"]): int(q["state0"]) + int(q["n_ref"])], self._packed.est_order[k])
                for k, q in enumerate(self._packed.problems)]


def pairs_of(mate_ref: np.ndarray, est_order: np.ndarray) -> np.ndarray:
    ref = np.nonzero(mate_ref >= 0)[0]
    return np.stack([ref, est_order[mate_ref[ref]]], axis=1).astype(np.int64).reshape(-1, 2)


def match(problems: Sequence[Problem], warm_start: Optional[Sequence] = None, packed: Optional[Packed] = None) -> Matching:
    """The maximum matchings of `problems`: one upload, one mt3_op_match_notes call, one copy of the counts.
    warm_start: per problem None or an int array [n_ref] of estimate indices (-1: free) to start from; entries that are
    not edges, out of range or claim an estimate twice are dropped by the kernel.  RuntimeError if the kernel reports
    that a problem passed its phase bound (count -1), which its termination argument excludes."""
    import torch
    packed = pack(problems) if packed is None else packed
    n = len(packed.problems)
    if warm_start is not None:
        workspace = note_arrays.to_device(warm_words(packed, warm_start))
    else:
        workspace = torch.empty(packed.workspace_words, device="cuda", dtype=torch.int32)
    if n == 0:
        return Matching(np.zeros(0, np.int64), workspace, packed)
    n_notes = packed.notes.shape[1]
    notes, ptr = note_arrays.upload(packed.notes, n_notes, ("<f8",) * 3)        # the one upload
    counts = torch.empty(n, device="cuda", dtype=torch.int32)
    _lib.check(_lib.load().mt3_op_match_notes(*ptr, n_notes, n, packed.problems.ctypes.data, len(packed.rules),
                                              packed.rules.ctypes.data, workspace.data_ptr() if workspace.numel() else None,
                                              packed.workspace_words, 1 if warm_start is not None else 0,
                                              counts.data_ptr(), torch.cuda.current_stream().cuda_stream))
    host = counts.cpu().numpy().astype(np.int64)         # the one copy back: 4 n bytes
    if (host < 0).any():
        raise RuntimeError("mt3_op_match_notes: problem %d passed its phase bound" % int(np.nonzero(host < 0)[0][0]))
    return Matching(host, workspace, packed)
