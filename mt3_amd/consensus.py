"""Consensus notes: several transcriptions of one recording (voters) -> the notes a quorum of them agrees on, and for every
note the number of voters that have it (mt3_op_note_consensus; the rule: include/mt3_hip.h, "note consensus").

  consensus(groups, ...)             the consensus of every file of a job on the device: one upload of the packed notes,
                                     one op call, one copy back
  consensus_reference(groups, ...)   the rule in numpy: the yardstick of the kernel, bit for bit

The voters of `InferenceModel.sample(audio, num_samples=n)` are the case it was built for (self-consistency: a note most
samples contain is kept, a note one sample made up is dropped, and the vote count is a confidence that costs no second
model pass); the engines of several precisions, greedy against k-beam, or two checkpoints are voters just as well.
There is no host fallback: `consensus` needs the library and a device.

THE RULE.  key = is_drum << 14 | program << 7 | pitch (programs=False: the program field is 0, so instruments do not
split a vote).  A file's notes, from all its voters together, are sorted by (key, onset, offset, velocity, voter).  Note i
of the sorted file starts a cluster when it is the first, or key[i] != key[i-1], or onset[i] - onset[i-1] > tolerance
(float64); clusters are runs [a, b) of m members = the connected components of "same key and onsets within tolerance".
votes = the distinct voters among the members; the cluster is kept when votes >= min_votes (default V // 2 + 1 of the
file's V voters).  The emitted note takes the onset of member a + (m - 1) // 2, the offset of rank (m - 1) // 2 under
(offset, position) and the velocity of rank (m - 1) // 2 under (velocity, position): lower medians, member values only, so
nothing rounds and end >= start.  Limit: repeated notes of one key closer than `tolerance` chain into one cluster;
members > votes shows it.
"""
from __future__ import annotations

import dataclasses
from typing import List, Optional, Sequence

import numpy as np

from . import _lib, note_arrays, note_sequences

MAX_VOTERS = _lib.CONSENSUS_MAX_VOTERS
DEFAULT_TOLERANCE = 0.05                # seconds: the onset tolerance of the note scores
LAYOUT = ("<f8", "<f8", "<i4", "<i4", "<i4")          # onset | offset | key | velocity | voter: what _pack lays out
OUT_LAYOUT = ("<f8", "<f8", "<i4", "<i4", "<i4", "<i4", "<i4")       # the consensus columns, votes, members, note_votes
FILE_DTYPE = np.dtype([("first", "<i8"), ("n_notes", "<i4"), ("n_voters", "<i4"), ("min_votes", "<i4"),
                       ("reserved", "<i4")])                                                   # mt3_consensus_file


@dataclasses.dataclass
class Consensus:
    """One file's result.  notes: the consensus NoteSequence, its notes in (start, is_drum, program, pitch) order,
    total_time the largest end (0.0 without notes).  votes / members: int64 [len(notes.notes)], the distinct voters and
    the member notes of each note's cluster.  note_votes[v]: int64, for every note of voter v in the voter's own order,
    the votes of its cluster (kept or not).  min_votes: the quorum that was used."""
    notes: note_sequences.NoteSequence
    votes: np.ndarray
    members: np.ndarray
    note_votes: List[np.ndarray]
    n_voters: int
    min_votes: int


@dataclasses.dataclass
class Packed:
    """the host side of one op call"""
    columns: np.ndarray                 # uint8: the LAYOUT columns back to back, each file's notes sorted
    n_notes: int
    files: np.ndarray                   # FILE_DTYPE [n_files]
    order: List[np.ndarray]             # per file: position in the sorted file -> index in the file's concatenated voters
    lengths: List[List[int]]            # per file: the notes of each voter
    tolerance: float

    def column(self, k: int) -> np.ndarray:
        at = note_arrays.column_offsets([np.dtype(dt).itemsize for dt in LAYOUT], self.n_notes)[k]
        return self.columns[at: at + self.n_notes * np.dtype(LAYOUT[k]).itemsize].view(LAYOUT[k])


def _quorums(min_votes, voters: Sequence[int]) -> List[int]:
    if min_votes is None:
        quorums = [v // 2 + 1 for v in voters]
    elif isinstance(min_votes, (int, np.integer)) and not isinstance(min_votes, bool):
        quorums = [int(min_votes)] * len(voters)
    else:
        quorums = list(min_votes) if hasattr(min_votes, "__len__") else None
        if quorums is None or len(quorums) != len(voters) or \
                any(isinstance(q, bool) or not isinstance(q, (int, np.integer)) for q in quorums):
            raise ValueError("min_votes must be None, an int or one int per file (%d), got %r" % (len(voters), min_votes))
        quorums = [int(q) for q in quorums]
    for f, (q, v) in enumerate(zip(quorums, voters)):
        if not 1 <= q <= v:
            raise ValueError("file %d: min_votes must be 1 .. %d (its voters), got %d" % (f, v, q))
    return quorums


def pack(groups, tolerance: float = DEFAULT_TOLERANCE, min_votes=None, programs: bool = True) -> Packed:
    """every check of `consensus`, the keys, and each file's notes sorted by (key, onset, offset, velocity, voter)"""
    if isinstance(tolerance, bool) or not isinstance(tolerance, (int, float, np.integer, np.floating)) or \
            not (np.isfinite(tolerance) and tolerance >= 0):
        raise ValueError("tolerance must be finite and not negative, got %r" % (tolerance,))
    groups = [list(g) for g in groups]
    for f, g in enumerate(groups):
        if not 1 <= len(g) <= MAX_VOTERS:
            raise ValueError("file %d: %d voters; a file has 1 .. %d" % (f, len(g), MAX_VOTERS))
    quorums = _quorums(min_votes, [len(g) for g in groups])
    cols = [[] for _ in LAYOUT]
    order, lengths = [], []
    for f, g in enumerate(groups):
        parts = [note_arrays.fields(v, program=True) for v in g]
        for v, (start, end, pitch, velocity, _, program) in enumerate(parts):
            prefix = "file %d, voter %d: " % (f, v)
            note_arrays.check_range(prefix + "pitches are 0 .. 127", pitch)
            note_arrays.check_range(prefix + "programs are 0 .. 127", program)
            note_arrays.check_range(prefix + "velocities are 0 .. 127", velocity)
            note_arrays.check_times(start, end, prefix=prefix)
            if (end < start).any():
                raise ValueError(prefix + "a note ends before it starts")
        lengths.append([len(p[0]) for p in parts])
        start, end, pitch, velocity, drum, program = (np.concatenate([p[k] for p in parts]) for k in range(6))
        voter = np.repeat(np.arange(len(parts)), lengths[-1])
        key = ((drum != 0).astype(np.int64) << 14) | ((program if programs else 0 * program) << 7) | pitch
        by = np.lexsort((voter, velocity, end, start, key))            # the last key is the primary one
        order.append(by)
        for c, a in zip(cols, (start, end, key, velocity, voter)):
            c.append(a[by])
    first = note_arrays.offsets([len(o) for o in order])
    files = np.zeros(len(groups), FILE_DTYPE)
    files["first"], files["n_notes"] = first[:-1], np.diff(first)
    files["n_voters"], files["min_votes"] = [len(g) for g in groups], quorums
    return Packed(note_arrays.pack(cols, LAYOUT), int(first[-1]), files, order, lengths, float(tolerance))


def _results(packed: Packed, onset, offset, key, velocity, votes, members, note_votes, counts) -> List[Consensus]:
    """the op's columns (job-wide; a file's kept notes from its `first` on) -> one Consensus per file"""
    out = []
    for f, n in zip(packed.files, counts):
        a = int(f["first"])
        on, off, k = onset[a: a + n], offset[a: a + n], key[a: a + n].astype(np.int64)
        drum, program, pitch = k >> 14, (k >> 7) & 127, k & 127
        by = np.lexsort((pitch, program, drum, on))
        notes = [note_sequences.Note(start_time=float(on[i]), end_time=float(off[i]), pitch=int(pitch[i]),
                                     velocity=int(velocity[a + i]), program=int(program[i]), is_drum=bool(drum[i]))
                 for i in by]
        mine = np.empty(int(f["n_notes"]), np.int64)
        mine[packed.order[len(out)]] = note_votes[a: a + int(f["n_notes"])]
        ends = np.cumsum(packed.lengths[len(out)])
        out.append(Consensus(note_sequences.NoteSequence(notes=notes, total_time=float(off.max()) if n else 0.0),
                             votes[a: a + n][by].astype(np.int64), members[a: a + n][by].astype(np.int64),
                             [mine[e - c: e] for e, c in zip(ends, packed.lengths[len(out)])], int(f["n_voters"]),
                             int(f["min_votes"])))
    return out


def reference_columns(packed: Packed):
    """THE RULE over the packed job, in numpy alone, in the op's output form: (onset, offset, key, velocity, votes,
    members, note_votes, counts); a file's kept notes lie compacted from its `first` on, the rest is zeros"""
    onset, offset, key, velocity, voter = (packed.column(k) for k in range(5))
    n, files = packed.n_notes, packed.files
    counts = np.zeros(len(files), np.int64)
    out = [np.zeros(n, dt) for dt in OUT_LAYOUT]
    if n == 0:
        return tuple(out) + (counts,)
    head = np.ones(n, bool)
    head[1:] = (key[1:] != key[:-1]) | (onset[1:] - onset[:-1] > packed.tolerance)
    head[files["first"][files["n_notes"] > 0]] = True
    cluster = np.cumsum(head) - 1                                      # per note
    a = np.nonzero(head)[0]                                            # per cluster from here on
    m = np.diff(np.append(a, n))
    k = a + (m - 1) // 2
    votes = np.bincount(np.unique(cluster * MAX_VOTERS + voter) // MAX_VOTERS, minlength=len(a))
    file_of = np.repeat(np.arange(len(files)), files["n_notes"])[a]
    kept = votes >= files["min_votes"][file_of]
    by_offset = np.lexsort((offset, cluster))                          # stable: (cluster, offset, position)
    by_velocity = np.lexsort((velocity, cluster))
    columns = (onset[k], offset[by_offset][k], key[a], velocity[by_velocity][k], votes, m)
    counts = np.bincount(file_of[kept], minlength=len(files))
    # the kept clusters of file f, in order, go to first[f], first[f] + 1, ...
    place = files["first"][file_of[kept]] + np.arange(int(kept.sum())) - (np.cumsum(counts) - counts)[file_of[kept]]
    for o, c in zip(out, columns):
        o[place] = c[kept]
    out[6][:] = votes[cluster]
    return tuple(out) + (counts,)


def consensus_reference(groups, tolerance: float = DEFAULT_TOLERANCE, min_votes=None, programs: bool = True):
    """`consensus` in numpy alone: the same arguments, checks and results, bit for bit"""
    packed = pack(groups, tolerance, min_votes, programs)
    return _results(packed, *reference_columns(packed))


def run(packed: Packed):
    """one upload, one mt3_op_note_consensus call, one copy back -> the op's columns as `reference_columns` gives them
    (entries past a file's count are whatever the buffer held)"""
    import torch
    n, n_files = packed.n_notes, len(packed.files)
    sizes = [np.dtype(dt).itemsize for dt in OUT_LAYOUT]
    at = note_arrays.column_offsets(sizes, n) + [n * sum(sizes)]          # the counts come last
    out = torch.empty(at[-1] + 4 * n_files, device="cuda", dtype=torch.uint8)
    scratch = torch.empty(_lib.CONSENSUS_SCRATCH_WORDS_PER_NOTE * n, device="cuda", dtype=torch.int32)
    notes, ptr = note_arrays.upload(packed.columns, n, LAYOUT)            # the one upload
    stream = torch.cuda.current_stream()
    _lib.check(_lib.load().mt3_op_note_consensus(
        *ptr, n, packed.files.ctypes.data, n_files, packed.tolerance, *[out.data_ptr() + a if n else None for a in at[:7]],
        out.data_ptr() + at[7], scratch.data_ptr() if n else None, scratch.numel(), stream.cuda_stream))
    scratch.record_stream(stream)
    host = out.cpu().numpy()                                              # the one copy back
    columns = [host[a: a + n * size].view(dt) for a, size, dt in zip(at, sizes, OUT_LAYOUT)]
    return tuple(columns) + (host[at[7]:].view("<i4").astype(np.int64),)


def consensus(groups, tolerance: float = DEFAULT_TOLERANCE, min_votes=None, programs: bool = True) -> List[Consensus]:
    """The consensus of every file of a job.  groups[f]: the transcriptions of file f, 1 .. 64 voters, each a NoteSequence
    or a metrics_utils.NOTE_DTYPE record array (a voter may have no notes; the order of a voter's notes and of the voters
    does not change the notes, votes or members).  tolerance: seconds between neighbouring onsets of one cluster.
    min_votes: None (a strict majority, V // 2 + 1, of each file's V voters), an int for all files or one int per file,
    each 1 .. V.  programs=False: instruments do not split a vote, and every consensus note has program 0.
    -> one `Consensus` per file.  One upload, one op call, one copy back.  ValueError, before anything is uploaded: a file
    with no voters or more than 64; a pitch, program or velocity outside 0 .. 127; a time that is not finite; a note that
    ends before it starts; a bad min_votes or tolerance.  An empty job gives an empty list."""
    packed = pack(groups, tolerance, min_votes, programs)
    if not len(packed.files):
        return []
    return _results(packed, *run(packed))
