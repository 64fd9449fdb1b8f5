"""mt3_op_prepare_notes on the device against the host rules, event by event (note_sequences.apply_sustain_control_changes,
trim_overlapping_notes): the survivors, their original positions, their ends as uint64 bit patterns and total_time, in both
modes, on every input.  No end is computed on either side, so every comparison is ==."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import metrics_utils, note_prep, note_sequences  # noqa: E402
from tests import note_prep_ref as ref  # noqa: E402

MODES = {"sustain": note_prep.SUSTAIN, "trim": note_prep.TRIM}


def _device(job, mode):
    """one mode over the job through the module's own path: per file (src, end, total_time)"""
    out = note_prep.apply([note_prep.columns(ns, f) for f, ns in enumerate(job)], MODES[mode])
    return [(c.src, c.end, c.total_time) for c in out]


def _assert_same(job, mode, got=None):
    got = _device(job, mode) if got is None else got
    assert len(got) == len(job)
    for f, (ns, (src, end, total)) in enumerate(zip(job, got)):
        want_src, want_end, want_total = ref.host_rule(ns, mode)
        assert src.tolist() == want_src.tolist(), (mode, f, len(ns.notes))
        bad = np.nonzero(end.view(np.uint64) != want_end.view(np.uint64))[0]
        assert bad.size == 0, (mode, f, bad[:8].tolist(), end[bad[:8]].tolist(), want_end[bad[:8]].tolist())
        assert np.float64(total).view(np.uint64) == np.float64(want_total).view(np.uint64), (mode, f, total, want_total)
    return got


@pytest.mark.parametrize("mode", sorted(MODES))
def test_hand_written_cases(mode):
    names = sorted(ref.HAND)
    got = _assert_same([ref.HAND[name][0] for name in names], mode)
    if mode == "sustain":                                     # and the literals themselves
        for name, (src, end, total) in zip(names, got):
            _, ends, want_total = ref.HAND[name]
            assert src.tolist() == [i for i, e in enumerate(ends) if e is not None], name
            assert end.tolist() == [e for e in ends if e is not None] and total == want_total, name


@pytest.mark.parametrize("mode", sorted(MODES))
def test_one_ragged_job(mode):
    job = ref.ragged_job()
    sizes = [len(ns.notes) for ns in job]
    assert {0, 1, 255, 256, 257, 600}.issubset(sizes) and max(sizes) > 4 * 256
    pedals = [sum(c.control_number == 64 for c in ns.control_changes) for ns in job]
    assert {0, 1, 700}.issubset(pedals)
    got = _assert_same(job, mode)
    run = sizes.index(600)
    if mode == "sustain":
        assert got[run][1][0] == 591.0                        # cut by a successor two tile boundaries away
    else:
        assert any(len(src) == 0 and len(ns.notes) > 0 for ns, (src, _, _) in zip(job, got))      # every note deleted


@pytest.mark.parametrize("mode", sorted(MODES))
def test_65_files_one_more_than_a_launch_holds(mode):
    rng = np.random.default_rng(65)
    job = [ref.random_sequence(rng, int(rng.integers(0, 40)), int(rng.integers(0, 30)), span=20) for _ in range(65)]
    job[64] = ref.HAND["note_seq_repeated_notes"][0]
    got = _assert_same(job, mode)
    if mode == "sustain":
        assert got[64][1].tolist() == [1.25, 2.0, 4.0, 3.50, 4.50]


@pytest.mark.parametrize("mode", sorted(MODES))
def test_random_jobs_dense_in_ties_and_twice_the_same_bits(mode):
    rng = np.random.default_rng(7)
    job = [ref.random_sequence(rng) for _ in range(300)]
    job += [ref.random_sequence(rng, int(rng.integers(200, 700)), int(rng.integers(0, 600)), span=30) for _ in range(6)]
    first = _assert_same(job, mode)
    again = _device(job, mode)
    for (a_src, a_end, a_total), (b_src, b_end, b_total) in zip(first, again):
        assert np.array_equal(a_src, b_src) and np.array_equal(a_end.view(np.uint64), b_end.view(np.uint64))
        assert a_total == b_total


def test_prepare_returns_sequences_or_record_arrays():
    job = [ref.HAND[name][0] for name in ("together_under_the_pedal", "note_seq_repeated_notes", "no_notes")]
    job.append(ref.seq([(60, 100, 0.0, 2.0, 0, 5), (60, 90, 1.0, 2.2, 0, 5), (38, 80, 0.5, 0.5, 9, 0, True)],
                       [(0.0, 127), (2.5, 0)]))
    out = note_prep.prepare(job)
    for ns, got in zip(job, out):
        assert got == note_sequences.sustain_reference(ns)
        assert all(a is not b for a in got.notes for b in ns.notes)           # copies: the caller's notes are untouched
    assert job[0].notes[0].end_time == 1.5 and len(job[0].control_changes) == 2
    both = note_prep.prepare(job, sustain=True, trim=True)
    for ns, got in zip(job, both):
        want = note_sequences.trim_overlapping_notes(note_sequences.sustain_reference(ns))
        assert got == want
    # under the pedal note 0 of the last file is cut at 1.0 and note 1 is held to 2.5; the zero-length drum is trimmed away
    assert [(n.start_time, n.end_time) for n in both[3].notes] == [(0.0, 1.0), (1.0, 2.5)]
    only_trim = note_prep.prepare(job, sustain=False, trim=True)
    for ns, got in zip(job, only_trim):
        want = note_sequences.trim_overlapping_notes(ns)
        assert got.notes == want.notes and got.total_time == want.total_time and got.control_changes == []
    assert note_prep.prepare(job, sustain=False) == [
        note_sequences.NoteSequence(ns.notes, ns.total_time, ns.ticks_per_quarter) for ns in job]
    arrays = note_prep.prepare(job, as_arrays=True)
    for got, rec in zip(out, arrays):
        assert rec.dtype == metrics_utils.NOTE_DTYPE and len(rec) == len(got.notes)
        assert [(n.start_time, n.end_time, n.pitch, n.velocity, n.program, int(n.is_drum), n.instrument) for n in got.notes] \
            == [tuple(r)[:7] for r in rec.tolist()]
    assert note_prep.prepare([]) == []
