"""The scripted seam cases of the target tokenizer (tests/tokenize_seams.py) on the host.  Every case's witness is asserted
against the tables; mt3_notes_tokenize is held to the plain Python restatement of the rule's text (include/mt3_hip.h,
"target tokenizer", items 1-5), which can express custom program maps and raw event columns; the cases that are
NoteSequences under a stock codec are held to the recipe as well.  Every comparison is ==.  No GPU."""
import numpy as np
import pytest

from mt3_amd import tokenize
from tests import tokenize_seams as seams

CASES = seams.all_cases()
NAMES = ("ids", "lengths", "truncated", "note_of", "is_onset")


def first_difference(name, got, want):
    """None, or 'case: array row r position i: got x, want y' for the first entry that differs"""
    for key in NAMES:
        g, w = np.asarray(got[key]).reshape(len(want[key]), -1), np.asarray(want[key]).reshape(len(want[key]), -1)
        bad = np.argwhere(g != w)
        if len(bad):
            r, i = bad[0]
            return "%s: %s row %d position %d: got %d, want %d" % (name, key, r, i, g[r, i], w[r, i])
    return None


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_witness_holds(case):
    assert case.claims, "a case without its witness is not a case"
    assert case.events.shape[1] <= 1500 * len(case.files)
    for kind, row, subject, stated in case.claims:
        assert seams.observe(case, kind, row, subject) == stated, (case.name, kind, row, subject)
        if kind == "held" and list(case.rule.program_map) == list(range(128)):     # and the restated row says the same
            section, program, pairs = seams.observe(case, "tie section", row, None), None, set()
            for what, value in section:
                program = value if what == "program" else program
                pairs |= {(program, value)} if what == "pitch" else set()
            assert (subject in pairs) == stated, (case.name, row, subject)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_host_rule_equals_the_restatement(case):
    for stride in case.strides:
        want = seams.expected(case, stride, seams.restated)
        assert first_difference("%s, stride %d" % (case.name, stride), seams.expected(case, stride, seams.host_row), want) is None


@pytest.mark.parametrize("case", [c for c in CASES if c.recipe], ids=lambda c: c.name)
def test_host_rule_equals_the_recipe(case):
    r = case.recipe
    for stride in case.strides:
        host = seams.expected(case, stride, seams.host_row)
        for f, (ns, frames) in enumerate(zip(r["sequences"], r["frames"])):
            rows, cut = tokenize.target_rows_reference(ns, frames, r["codec"], seams.TIES, r["granularity"], stride,
                                                       segment_frames=r["segment_frames"])
            mine = seams.rows_of(case, f)
            assert len(mine) == len(rows)
            for row, want, was_cut in zip(mine, rows, cut):
                n = int(host["lengths"][row])
                assert (n, int(host["truncated"][row])) == (len(want), was_cut), (case.name, stride, row)
                assert host["ids"][row, :n].tolist() == want.tolist(), (case.name, stride, row)
                assert not host["ids"][row, n:].any()


def test_the_witnesses_cover_what_the_cases_are_for():
    """the seams the cases exist for, counted over all witnesses: lanes 255 and 0 on both kinds of tile, every kind of id
    under the cut, tie rows that do not open, several shift ids"""
    claims = [(c, k, row, s, v) for c in CASES for k, row, s, v in c.claims]
    for kind in ("advance", "events"):
        lanes = {v for _, k, _, _, v in claims if k == kind and v is not None}
        assert {lane for _, lane in lanes} >= {0, 255} and {tile for tile, _ in lanes} >= {0, 1}, kind
    assert {v[0] for _, k, _, _, v in claims if k == "cut"} == {"tie program", "tie pitch", "tie", "shift", "program", "velocity",
                                                               "pitch", "eos", "pad"}
    assert max(len(v) for _, k, _, _, v in claims if k == "shift ids") == 30
    origins = {seams._ranges(c, row)[1] % 256 for c, k, row, _, _ in claims if k == "advance"}
    assert origins >= {0, 37}
    assert any(k == "written" and not v for _, k, _, _, v in claims)


def test_the_cut_around_the_end_of_the_row():
    """from the rule: with `base` ids before the EOS, a stride of base + 1 is the last that keeps the EOS (in its last
    position), base + 2 pads, base and below end without EOS and are truncated"""
    case, base = seams.cut_case()
    assert set(range(2, 21)) | {base - 1, base, base + 1, base + 2} <= set(case.strides)
    for stride, (length, truncated) in ((base + 2, (base + 1, 0)), (base + 1, (base + 1, 0)), (base, (base, 1)),
                                        (base - 1, (base - 1, 1))):
        host = seams.expected(case, stride, seams.host_row)
        for row in (1, 3):
            ids = host["ids"][row].tolist()
            assert (int(host["lengths"][row]), int(host["truncated"][row])) == (length, truncated), (stride, row)
            assert (1 in ids) == (not truncated) and (truncated or ids[base] == 1)
            assert ids[base + 1:] == [0] * (stride - base - 1)
    whole = seams.expected(case, base + 2, seams.host_row)["ids"][1]
    for stride in case.strides:                                       # every cut is a prefix of the uncut row
        host = seams.expected(case, stride, seams.host_row)
        n = min(stride, base + 2)
        assert host["ids"][1, :n].tolist() == whole[:n].tolist() and host["ids"][3].tolist() == host["ids"][1].tolist()


def test_the_tables_job_is_what_it_says():
    case = next(c for c in CASES if c.name.startswith("tables"))
    host = seams.expected(case, 32, seams.host_row)
    tie = case.rule.tie_id
    for row in (7, 8, 14):                                            # the n_rows = 0 file, and a row outside its file's range
        assert (host["ids"][row] == seams.SENTINEL).all() and host["lengths"][row] == seams.SENTINEL
    for row in (9, 10, 11, 12, 13):                                   # the empty file, and the one whose events are out of range
        assert host["ids"][row, :3].tolist() == [tie, 1, 0] and host["lengths"][row] == 2
    assert host["ids"][2].tolist() == host["ids"][3].tolist()         # one step_lo twice
    assert tie in host["ids"][5] and host["note_of"][5].max() == -1   # step_hi <= step_lo: a tie section and no event
    r = case.rule                                                     # masked and clamped: pitch 200 -> 72, program -3 -> 125, 500 -> 127
    assert host["ids"][0, :8].tolist() == [tie, r.program_first, r.velocity_first + 5, r.pitch_first + 60, r.shift_first + 1,
                                           r.velocity_first + 90, r.pitch_first + 72, r.shift_first + 2]
    assert host["ids"][0, 8:11].tolist() == [r.program_first + 125, r.velocity_first + 127, r.pitch_first + 62]
    both = seams.split(case)
    assert len(both) == 5 and all(len(j.files) == 1 for j in both)
    assert [seams.rows_of(j, 0) for j in both] == [seams.rows_of(case, f) for f in range(5)]
