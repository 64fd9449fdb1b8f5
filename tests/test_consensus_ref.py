"""`consensus.consensus_reference` (the numpy statement of the consensus rule, the yardstick of the GPU tests) against the
brute force of tests/consensus_ref.py: all-pairs connected components, medians from sorted lists, votes from sets."""
import numpy as np
import pytest

from mt3_amd import consensus, metrics_utils
from tests import consensus_ref as ref


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_hand_written_cases(name):
    groups, kw = ref.CASES[name]
    got = ref.as_brute(consensus.consensus_reference(groups, **kw))
    assert got == ref.brute_force(groups, **kw)


def test_what_the_hand_written_cases_are_about():
    run = lambda name: consensus.consensus_reference(*ref.CASES[name][:1], **ref.CASES[name][1])[0]     # noqa: E731
    tie = run("tie_at_tolerance")                  # 10, 13, 16 in one cluster (gaps of exactly the tolerance); 20 alone
    assert [n.start_time for n in tie.notes.notes] == [13 * ref.G, 20 * ref.G]
    assert list(tie.votes) == [3, 1] and list(tie.members) == [3, 1]
    dup = run("duplicates_of_one_voter")           # three copies from one voter are one vote; 2 of 3 voters: kept
    assert list(dup.votes) == [2] and list(dup.members) == [4] and dup.n_voters == 3
    assert [list(v) for v in dup.note_votes] == [[2, 2, 2], [2], []]
    assert len(run("same_onset_other_key").notes.notes) == 4        # pitch, program and drum flag each split
    flat = run("programs_false")                   # programs no longer split: pitch 60, pitch 61 and the drum, 2 votes each
    assert [(n.pitch, n.program, n.is_drum) for n in flat.notes.notes] == [(60, 0, False), (61, 0, False), (60, 0, True)]
    assert list(flat.votes) == [2, 2, 2] and list(flat.members) == [3, 2, 2]
    one = run("one_voter")
    assert list(one.votes) == [1, 1] and list(one.members) == [2, 1] and one.min_votes == 1
    assert [len(run(n).notes.notes) for n in ("min_votes_1", "min_votes_majority", "min_votes_all")] == [4, 2, 1]
    empty = run("a_voter_without_notes")
    assert list(empty.votes) == [2] and [len(v) for v in empty.note_votes] == [0, 1, 1, 0]
    chain = run("chain")
    assert list(chain.votes) == [2] and list(chain.members) == [5]
    assert chain.notes.notes[0].start_time == 1.08 and chain.notes.notes[0].end_time == 1.11
    per_file = consensus.consensus_reference(*ref.CASES["per_file_min_votes"][:1], **ref.CASES["per_file_min_votes"][1])
    assert [len(r.notes.notes) for r in per_file] == [1, 3, 0] and [r.min_votes for r in per_file] == [3, 1, 1]
    assert per_file[2].notes.total_time == 0.0 and [len(v) for v in per_file[2].note_votes] == [0]


@pytest.mark.parametrize("grid", [True, False])
def test_random_jobs(grid):
    for seed in range(40):
        groups = ref.random_job(seed, grid=grid)
        for kw in (dict(), dict(min_votes=1), dict(programs=False), dict(tolerance=3 * ref.G), dict(tolerance=0.0)):
            got = consensus.consensus_reference(groups, **kw)
            assert ref.as_brute(got) == ref.brute_force(groups, **kw), (seed, kw)
            for r in got:
                assert all(n.end_time >= n.start_time for n in r.notes.notes)
                assert all(r.min_votes <= v <= r.n_voters for v in r.votes) and all(r.members >= r.votes)
                key = [(n.start_time, n.is_drum, n.program, n.pitch) for n in r.notes.notes]
                assert key == sorted(key)


def test_the_order_of_notes_and_voters_does_not_matter():
    for seed in range(20):
        groups = ref.random_job(100 + seed)
        other, voter_order, note_order = ref.shuffled(groups, seed)
        a, b = consensus.consensus_reference(groups), consensus.consensus_reference(other)
        for ra, rb, order, perms in zip(a, b, voter_order, note_order):
            assert ra.notes == rb.notes and np.array_equal(ra.votes, rb.votes) and np.array_equal(ra.members, rb.members)
            for new, (old, p) in enumerate(zip(order, perms)):                # nothing but note_votes' permutation
                assert np.array_equal(rb.note_votes[new], ra.note_votes[old][p])


def test_record_arrays_are_voters_too():
    groups = ref.random_job(7, files=2)
    records = [[np.array([(n.start_time, n.end_time, n.pitch, n.velocity, n.program, n.is_drum, 0, 0) for n in v.notes],
                         metrics_utils.NOTE_DTYPE) for v in g] for g in groups]
    ref.assert_same(consensus.consensus_reference(records), consensus.consensus_reference(groups))


def test_an_empty_job():
    assert consensus.consensus_reference([]) == [] and consensus.consensus([]) == []


def test_value_errors_come_before_anything_is_uploaded():
    ok = ref.ns([(0.0, 1.0, 60)])
    bad = [
        (dict(groups=[[]]), "voters"),
        (dict(groups=[[ok] * 65]), "voters"),
        (dict(groups=[[ref.ns([(0.0, 1.0, 128)])]]), "pitches are 0 .. 127"),
        (dict(groups=[[ok, ref.ns([(0.0, 1.0, 60, 100, 128)])]]), "programs are 0 .. 127"),
        (dict(groups=[[ref.ns([(float("nan"), 1.0, 60)])]]), "finite"),
        (dict(groups=[[ref.ns([(0.0, float("inf"), 60)])]]), "finite"),
        (dict(groups=[[ref.ns([(1.0, 0.5, 60)])]]), "ends before it starts"),
        (dict(groups=[[ok, ok]], min_votes=0), "min_votes"),
        (dict(groups=[[ok, ok]], min_votes=3), "min_votes"),
        (dict(groups=[[ok, ok]], min_votes=[1, 1]), "min_votes"),
        (dict(groups=[[ok, ok]], min_votes=1.5), "min_votes"),
        (dict(groups=[[ok, ok]], min_votes=True), "min_votes"),
        (dict(groups=[[ok]], tolerance=-0.01), "tolerance"),
        (dict(groups=[[ok]], tolerance=float("nan")), "tolerance"),
        (dict(groups=[[ok]], tolerance=float("inf")), "tolerance"),
    ]
    for kw, what in bad:
        for fn in (consensus.consensus, consensus.consensus_reference):       # the device is never reached
            with pytest.raises(ValueError, match=what):
                fn(**kw)
