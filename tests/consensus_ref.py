"""The consensus rule (include/mt3_hip.h, "note consensus") once more, by brute force and sharing no code with
mt3_amd/consensus.py: clusters as connected components over ALL same-key pairs with |onset_i - onset_j| <= tolerance
(union-find), medians by sorting Python lists, votes with sets.  Also the hand-written cases and the random jobs that
the CPU and the GPU tests both run."""
import numpy as np

from mt3_amd import note_sequences


def ns(notes):
    """[(start, end, pitch[, velocity[, program[, is_drum]]])] -> NoteSequence"""
    out = note_sequences.NoteSequence()
    for n in notes:
        start, end, pitch = n[:3]
        velocity, program, drum = (list(n[3:]) + [100, 0, False][len(n) - 3:])[:3]
        out.notes.append(note_sequences.Note(float(start), float(end), int(pitch), int(velocity), int(program), bool(drum)))
        out.total_time = max(out.total_time, float(end))
    return out


def brute_force(groups, tolerance=0.05, min_votes=None, programs=True):
    """-> per file: (notes, note_votes): notes = [(start, end, pitch, velocity, program, is_drum, votes, members)] in
    (start, is_drum, program, pitch) order; note_votes[v] = [votes of the cluster of voter v's note i]"""
    out = []
    for f, voters in enumerate(groups):
        V = len(voters)
        quorum = V // 2 + 1 if min_votes is None else (min_votes if isinstance(min_votes, int) else min_votes[f])
        notes = [(v, i, n) for v, seq in enumerate(voters) for i, n in enumerate(seq.notes)]
        keys = [(bool(n.is_drum), n.program if programs else 0, n.pitch) for _, _, n in notes]
        parent = list(range(len(notes)))

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for a in range(len(notes)):
            for b in range(a):
                if keys[a] == keys[b] and abs(notes[a][2].start_time - notes[b][2].start_time) <= tolerance:
                    parent[find(a)] = find(b)
        clusters = {}
        for a in range(len(notes)):
            clusters.setdefault(find(a), []).append(a)
        emitted, note_votes = [], [[None] * len(seq.notes) for seq in voters]
        for members in clusters.values():
            votes = len(set(notes[a][0] for a in members))
            for a in members:
                note_votes[notes[a][0]][notes[a][1]] = votes
            if votes < quorum:
                continue
            k = (len(members) - 1) // 2
            drum, program, pitch = keys[members[0]]
            emitted.append((sorted(notes[a][2].start_time for a in members)[k],
                            sorted(notes[a][2].end_time for a in members)[k], pitch,
                            sorted(notes[a][2].velocity for a in members)[k], program, drum, votes, len(members)))
        emitted.sort(key=lambda e: (e[0], e[5], e[4], e[2]))
        out.append((emitted, note_votes))
    return out


def as_brute(results):
    """a list of consensus.Consensus in brute_force's form"""
    return [([(n.start_time, n.end_time, n.pitch, n.velocity, n.program, bool(n.is_drum), int(v), int(m))
              for n, v, m in zip(r.notes.notes, r.votes, r.members)], [list(map(int, nv)) for nv in r.note_votes])
            for r in results]


def assert_same(got, want):
    """two lists of consensus.Consensus are the same to the bit: integer columns equal, times equal as uint64"""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.n_voters == w.n_voters and g.min_votes == w.min_votes
        assert len(g.notes.notes) == len(w.notes.notes)
        for name in ("pitch", "velocity", "program", "is_drum"):
            assert np.array_equal([getattr(n, name) for n in g.notes.notes], [getattr(n, name) for n in w.notes.notes]), name
        for name in ("start_time", "end_time"):
            a = np.array([getattr(n, name) for n in g.notes.notes], np.float64).view(np.uint64)
            b = np.array([getattr(n, name) for n in w.notes.notes], np.float64).view(np.uint64)
            assert np.array_equal(a, b), name
        assert np.float64(g.notes.total_time).view(np.uint64) == np.float64(w.notes.total_time).view(np.uint64)
        assert np.array_equal(g.votes, w.votes) and np.array_equal(g.members, w.members)
        assert len(g.note_votes) == len(w.note_votes)
        for a, b in zip(g.note_votes, w.note_votes):
            assert np.array_equal(a, b)


G = 1.0 / 64            # a grid on which sums and differences are exact

_three = [ns([(0.50, 1.00, 60, 90), (1.00, 1.50, 62, 80), (2.00, 2.20, 64, 70)]),
          ns([(0.51, 1.10, 60, 70), (1.02, 1.40, 62, 100)]),
          ns([(0.49, 0.90, 60, 80), (3.00, 3.50, 65, 60)])]

# name -> (groups, keywords)
CASES = {
    # onsets 3/64 apart with tolerance 3/64: equality is exact and must NOT split; 4/64 apart must
    "tie_at_tolerance": ([[ns([(10 * G, 30 * G, 60)]), ns([(13 * G, 31 * G, 60)]), ns([(16 * G, 29 * G, 60), (20 * G, 40 * G, 60)])]],
                         dict(tolerance=3 * G, min_votes=1)),
    "duplicates_of_one_voter": ([[ns([(1.0, 2.0, 60, 80), (1.0, 2.0, 60, 80), (1.0, 2.0, 60, 80)]), ns([(1.01, 2.1, 60, 90)]),
                                  ns([])]], dict()),
    "same_onset_other_key": ([[ns([(1.0, 2.0, 60, 80, 0), (1.0, 2.0, 61, 80, 0), (1.0, 2.0, 60, 80, 5), (1.0, 2.0, 60, 80, 0, True)]),
                               ns([(1.0, 2.0, 60, 80, 5), (1.0, 2.0, 60, 70, 0, True), (1.0, 2.5, 60, 80, 0)])]],
                             dict(min_votes=1)),
    "programs_false": ([[ns([(1.0, 2.0, 60, 80, 0), (1.0, 2.0, 61, 80, 0), (1.0, 2.0, 60, 80, 5), (1.0, 2.0, 60, 80, 0, True)]),
                         ns([(1.0, 2.0, 60, 80, 7), (1.0, 2.0, 60, 70, 3, True), (1.0, 2.5, 61, 80, 9)])]],
                       dict(programs=False)),
    "one_voter": ([[ns([(0.0, 0.5, 60), (0.02, 0.6, 60), (1.0, 1.5, 61)])]], dict()),
    "min_votes_1": ([_three], dict(min_votes=1)),
    "min_votes_majority": ([_three], dict()),
    "min_votes_all": ([_three], dict(min_votes=3)),
    "a_voter_without_notes": ([[ns([]), ns([(0.5, 1.0, 60)]), ns([(0.52, 1.1, 60)]), ns([])]], dict(min_votes=2)),
    # five notes 0.04 s apart chain into one cluster of 5 members and 2 votes: the documented limit
    "chain": ([[ns([(1.00, 1.03, 60), (1.08, 1.11, 60), (1.16, 1.19, 60)]), ns([(1.04, 1.07, 60), (1.12, 1.15, 60)])]], dict()),
    "per_file_min_votes": ([_three, _three[:2], [ns([])]], dict(min_votes=[3, 1, 1])),
}


def random_job(seed, files=4, grid=True, max_voters=5, notes=12, pitches=3):
    """a small job dense in ties: few pitches, short times (on a 1/64 grid: ties everywhere), some programs and drums"""
    rng = np.random.RandomState(seed)
    groups = []
    for _ in range(files):
        voters = []
        for _ in range(rng.randint(1, max_voters + 1)):
            seq = []
            for _ in range(rng.randint(0, notes + 1)):
                start = rng.randint(0, 64) * G if grid else float(rng.uniform(0, 1.0))
                length = rng.randint(0, 16) * G if grid else float(rng.uniform(0, 0.3))
                seq.append((start, start + length, 60 + rng.randint(pitches), rng.randint(1, 128), rng.randint(2),
                            bool(rng.randint(4) == 0)))
            voters.append(ns(seq))
        groups.append(voters)
    return groups


def shuffled(groups, seed):
    """the same job, every voter's notes and every file's voters in another order -> (groups, per file: the voter order,
    per file and NEW voter: the permutation of its notes)"""
    rng = np.random.RandomState(seed)
    out, voter_order, note_order = [], [], []
    for voters in groups:
        order = rng.permutation(len(voters))
        perms = [rng.permutation(len(voters[v].notes)) for v in order]
        out.append([note_sequences.NoteSequence(notes=[voters[v].notes[i] for i in p], total_time=voters[v].total_time)
                    for v, p in zip(order, perms)])
        voter_order.append(order)
        note_order.append(perms)
    return out, voter_order, note_order
