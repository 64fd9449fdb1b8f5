"""The target tokenizer's rule on the host (mt3_notes_tokenize; include/mt3_hip.h, mt3t_*) against the recipe stated in the
host mirror's own functions (`tokenize.target_rows_reference`: encode_and_index_events, segment_targets,
remove_redundant_state_changes -- themselves pinned to the reference by tests/test_encoding.py).  Every comparison is ==.
No GPU."""
import numpy as np
import pytest

from mt3_amd import metrics_utils, note_sequences, tokenize, vocabularies
from tests import tokenize_cases

TIES, NOTES = note_sequences.NoteEncodingWithTiesSpec, note_sequences.NoteEncodingSpec
GRANULARITIES = ("full", "midi_class", "flat")


@pytest.fixture(scope="module")
def codecs():
    return {TIES.name: vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1)),
            NOTES.name: vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=127))}


@pytest.fixture(scope="module")
def files():
    return tokenize_cases.hand_made() + tokenize_cases.random_files() + tokenize_cases.spread_files()


def _equal(host, reference_rows, reference_cut, row0, name):
    for s, (want, cut) in enumerate(zip(reference_rows, reference_cut)):
        got = host.ids[row0 + s]
        n = int(host.lengths[row0 + s])
        assert n == len(want) and int(host.truncated[row0 + s]) == cut, (name, s, n, len(want))
        assert np.array_equal(got[:n], want), (name, s, got[:n].tolist(), want.tolist())
        assert not got[n:].any(), (name, s)


@pytest.mark.parametrize("spec", [TIES, NOTES], ids=lambda s: s.name)
@pytest.mark.parametrize("granularity", GRANULARITIES)
def test_host_rule_equals_the_recipe_row_for_row(codecs, files, spec, granularity):
    codec = codecs[spec.name]
    host = tokenize.target_rows_host([ns for _, ns, _ in files], [f for _, _, f in files], codec, spec, granularity,
                                     segment_frames=256)
    for i, (name, ns, frames) in enumerate(files):
        rows, cut = tokenize.target_rows_reference(ns, frames, codec, spec, granularity, segment_frames=256)
        row0, n_rows = host.rows_of_file[i, 0]
        assert n_rows == len(rows), name
        _equal(host, rows, cut, row0, name)


@pytest.mark.parametrize("stride", [8, 2, 37])
def test_the_cut_row_for_row(codecs, files, stride):
    codec = codecs[TIES.name]
    host = tokenize.target_rows_host([ns for _, ns, _ in files], [f for _, _, f in files], codec, TIES, stride=stride)
    cut_rows = 0
    for i, (name, ns, frames) in enumerate(files):
        rows, cut = tokenize.target_rows_reference(ns, frames, codec, TIES, stride=stride)
        _equal(host, rows, cut, host.rows_of_file[i, 0, 0], name)
        cut_rows += sum(cut)
    assert cut_rows > 0


def test_expected_rows_of_the_hand_made_cases(codecs, files):
    """what the cases are there for, read off the rows themselves"""
    codec = codecs[TIES.name]
    by_name = {name: (i, ns, frames) for i, (name, ns, frames) in enumerate(files)}
    host = tokenize.target_rows_host([ns for _, ns, _ in files], [f for _, _, f in files], codec, TIES)
    E = lambda t, v: codec.encode_event(vocabularies.event_codec.Event(t, v)) + 3            # noqa: E731
    tie, eos = E("tie", 0), 1

    def rows_of(name):
        first, n = host.rows_of_file[by_name[name][0], 0]
        return [host.ids[r, : host.lengths[r]].tolist() for r in range(first, first + n)]

    assert rows_of("empty file of 3 segments") == [[tie, eos]] * 3
    assert len(rows_of("one segment")) == 1
    held = [E("program", 0), E("pitch", 60), tie]
    across = rows_of("one note across 3 segment starts")
    assert [r[:3] for r in across[1:]] == [held] * 3 and across[0][0] == tie
    # steps 12 and 38: 12.5 and 37.5 round half to even
    assert rows_of("half to even")[0] == [tie, E("shift", 12), E("program", 0), E("velocity", 1), E("pitch", 60),
                                          E("shift", 30), E("velocity", 0), E("pitch", 60),
                                          E("shift", 38), E("velocity", 1), E("pitch", 62),
                                          E("shift", 50), E("velocity", 0), E("pitch", 62), eos]
    # an event on step_lo = 204 has no shift id and belongs to the later segment; the one a step later has shift 1
    on_lo = rows_of("event exactly on step_lo")
    assert on_lo[0] == [tie, eos]
    assert on_lo[1][:7] == [tie, E("program", 0), E("velocity", 1), E("pitch", 60), E("shift", 1), E("pitch", 62), E("shift", 46)]
    # two times on one step: one shift id
    assert rows_of("two times on one step")[0][:7] == [tie, E("shift", 50), E("program", 0), E("velocity", 1), E("pitch", 60),
                                                       E("pitch", 62), E("shift", 100)]
    # the frozen state: the silent segments after the file's last event still declare the note that event ended
    frozen = rows_of("offset, then two silent segments")
    assert frozen[1] == frozen[2] == [E("program", 0), E("pitch", 64), tie, eos]
    # notes after the last frame belong to the last segment
    late = rows_of("notes after the last frame")
    assert len(late) == 2 and E("pitch", 64) in late[1] and E("pitch", 62) in late[1]
    # the seam: the first event's program id is dropped when the tie section ended on it, written when it did not
    same = rows_of("three programs held, seam on the last program")[1]
    other = rows_of("three programs held, seam on another program")[1]
    assert same[:10] == [E("program", 0), E("pitch", 60), E("program", 33), E("pitch", 50), E("program", 40), E("pitch", 70),
                         E("pitch", 72), tie, E("shift", 6), E("velocity", 1)]
    assert other[:9] == [E("program", 0), E("pitch", 60), E("program", 33), E("pitch", 50), E("program", 41), E("pitch", 70),
                         tie, E("shift", 6), E("program", 33)]
    storm_first, storm_n = host.rows_of_file[by_name["chord storm"][0], 0]
    assert host.truncated[storm_first] == 1 and host.lengths[storm_first] == 1024 and eos not in host.ids[storm_first]
    assert len(by_name["chord storm"][1].notes) * 2 > 256              # more than one workgroup tile of events in the segment
    drums = rows_of("drum and pitched note on one pitch number")
    assert E("drum", 40) in drums[0] and E("pitch", 40) in drums[0] and drums[1][:3] == [E("program", 0), E("pitch", 40), tie]


@pytest.mark.parametrize("spec", [TIES, NOTES], ids=lambda s: s.name)
def test_note_of_and_is_onset(codecs, files, spec):
    codec = codecs[spec.name]
    host = tokenize.target_rows_host([ns for _, ns, _ in files], [f for _, _, f in files], codec, spec, segment_frames=256)
    v_lo, v_hi = (x + 3 for x in codec.event_type_range("velocity"))
    p_lo = codec.event_type_range("pitch")[0] + 3
    d_lo = codec.event_type_range("drum")[0] + 3
    tie = codec.event_type_range("tie")[0] + 3
    seen = 0
    for i, (name, ns, _) in enumerate(files):
        first, n = host.rows_of_file[i, 0]
        linked = set()
        for r in range(first, first + n):
            velocity, in_ties = None, spec is TIES
            for pos in range(host.lengths[r]):
                tok, note = int(host.ids[r, pos]), int(host.note_of[r, pos])
                if v_lo <= tok <= v_hi:
                    velocity = tok - v_lo
                if tok == tie:
                    in_ties = False
                is_note_id = not in_ties and (p_lo <= tok < p_lo + 128 or (spec is TIES and d_lo <= tok < d_lo + 128))
                assert (note >= 0) == is_note_id, (name, r, pos)
                if note >= 0:
                    drum = spec is TIES and tok >= d_lo
                    assert ns.notes[note].pitch == tok - (d_lo if drum else p_lo), (name, r, pos)
                    assert int(host.is_onset[r, pos]) == (1 if velocity else 0), (name, r, pos)
                    linked.add((note, int(host.is_onset[r, pos])))
                    seen += 1
                else:
                    assert host.is_onset[r, pos] == 0
            assert (host.note_of[r, host.lengths[r]:] == -1).all() and not host.is_onset[r, host.lengths[r]:].any()
        if not host.truncated[first: first + n].any():
            assert {k for k, on in linked if on} == {k for k, x in enumerate(ns.notes) if x.velocity > 0}, name
    assert seen > 1000


def test_round_trip_through_the_note_decoder(codecs):
    codec = codecs[TIES.name]
    vocab = vocabularies.vocabulary_from_codec(codec)
    for name, ns, frames in tokenize_cases.random_files() + tokenize_cases.spread_files(seeds=range(3)):
        host = tokenize.target_rows_host([ns], [frames], codec, TIES)
        assert not host.truncated.any()
        starts = [tokenize.segment_steps(frames, codec, 256)[s, 0] / codec.steps_per_second for s in range(len(host.ids))]
        tokens = vocab.decode_tf(host.ids)
        rec, invalid, dropped, _ = metrics_utils.decode_token_rows(codec, TIES, tokens, np.asarray(starts, np.float64),
                                                                   lengths=host.lengths - 1)
        assert invalid == 0 and dropped == 0, name
        step = lambda t: int(round(t * 100))                             # noqa: E731
        want = sorted((step(n.start_time), n.pitch, bool(n.is_drum), 0 if n.is_drum else n.program)      # a drum id names no program
                      for n in ns.notes)
        got = sorted((step(a), p, bool(d), g) for a, b, p, v, g, d, i, _ in rec.tolist())
        assert got == want, name


def test_shifts_are_separately_shifted_files(codecs):
    codec = codecs[TIES.name]
    _, ns, frames = tokenize_cases.spread_files(seeds=[3])[0]
    shifts = [-0.05, 0, 0.05]
    a = tokenize.target_rows_host([ns], [frames], codec, TIES, shifts=shifts)
    b = tokenize.target_rows_host([tokenize_cases.shifted(ns, s) for s in shifts], [frames] * 3, codec, TIES)
    assert a.rows_of_file.shape == (1, 3, 2) and b.rows_of_file.shape == (3, 1, 2)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x).reshape(-1), np.asarray(y).reshape(-1))
    assert not np.array_equal(a.ids[: len(a.ids) // 3], a.ids[len(a.ids) // 3: 2 * len(a.ids) // 3])


def test_pack_order_and_refusals(codecs):
    codec = codecs[TIES.name]
    _, ns, _ = tokenize_cases.spread_files(seeds=[1])[0]
    packed = tokenize.pack([ns], codec, TIES)
    times, values = note_sequences.note_sequence_to_onsets_and_offsets_and_programs(ns)
    order = np.argsort(np.asarray(times), kind="stable")
    assert packed.events[0].tolist() == [round(times[i] * 100) for i in order]
    assert packed.events[1].tolist() == [values[i].pitch for i in order]
    assert packed.events[2].tolist() == [values[i].program for i in order]
    assert packed.events[3].tolist() == [vocabularies.velocity_to_bin(values[i].velocity, 1) for i in order]
    assert packed.events[4].tolist() == [int(values[i].is_drum) for i in order]
    assert all(ns.notes[k].pitch == p for k, p in zip(packed.events[5], packed.events[1]))
    with pytest.raises(ValueError):
        tokenize.target_rows_host([ns], [100], codec, note_sequences.NoteOnsetEncodingSpec)
    with pytest.raises(ValueError):
        tokenize.target_rows_host([ns], [100], codec, TIES, granularity="coarse")
    with pytest.raises(ValueError):
        tokenize.target_rows_host([ns], [100, 100], codec, TIES)
    with pytest.raises(ValueError):
        tokenize.target_rows_host([ns], [100], codec, TIES, stride=1)
