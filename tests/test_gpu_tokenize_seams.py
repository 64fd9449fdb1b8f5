"""mt3_op_tokenize_notes on the scripted seam cases (tests/tokenize_seams.py: advance tiles split between a pair's writers,
stale last-writer keys, the tie section's scans, the program carry across event tiles, several shift ids, the cut at every
kind of position, tables the planner never builds) against mt3_notes_tokenize, which tests/test_tokenize_seams_ref.py
holds to a restatement of the rule's text.  The outputs lie between sentinel rows and every row that no file writes keeps
its sentinel; each event column is a buffer of its own that ends with the column.  Every comparison is ==."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib  # noqa: E402
from tests import tokenize_seams as seams  # noqa: E402
from tests.test_tokenize_seams_ref import NAMES, first_difference  # noqa: E402

CASES = seams.all_cases()
DTYPES = dict(ids=torch.int32, lengths=torch.int32, truncated=torch.int32, note_of=torch.int32, is_onset=torch.uint8)


def fresh(case, stride):
    """the five outputs, sentinels everywhere, with one row more at either end than the job has"""
    n = len(case.rows) + 2
    return {k: torch.full((n, stride) if k in ("ids", "note_of", "is_onset") else (n,),
                          seams.SENTINEL & 255 if k == "is_onset" else seams.SENTINEL, dtype=DTYPES[k], device="cuda")
            for k in NAMES}


def launch(case, stride, out):
    """one call as mt3_amd.tokenize.run makes it, writing from row 1 of `out`"""
    n_ev = case.events.shape[1]
    columns = [torch.from_numpy(np.ascontiguousarray(case.events[k])).cuda() for k in range(6)] if n_ev else []
    assert all(c.numel() == n_ev for c in columns)
    files = torch.from_numpy(case.files.view(np.uint8).copy()).cuda()
    rows = torch.from_numpy(case.rows.view(np.uint8).copy()).cuda()
    ptr = {k: out[k].data_ptr() + out[k][0].numel() * out[k].element_size() for k in NAMES}
    _lib.check(_lib.load().mt3_op_tokenize_notes(
        C.byref(case.rule), *([c.data_ptr() for c in columns] or [None] * 6), n_ev, files.data_ptr(), len(case.files),
        rows.data_ptr(), len(case.rows), stride, ptr["ids"], ptr["lengths"], ptr["truncated"], ptr["note_of"], ptr["is_onset"],
        torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in NAMES}


def same(name, got, want):
    """the job's rows equal `want`, unwritten rows keeping their sentinels, and the row before and the row after intact"""
    bad = first_difference(name, {k: v[1:-1] for k, v in got.items()}, want)
    assert bad is None, bad
    for k in NAMES:
        guard = seams.SENTINEL & 255 if k == "is_onset" else seams.SENTINEL
        assert (got[k][0] == guard).all() and (got[k][-1] == guard).all(), "%s: %s written outside the job's rows" % (name, k)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_kernel_equals_the_host_rule(case):
    assert len(case.rows) >= 1 and case.events.shape[1] <= 1500 * len(case.files)
    for stride in case.strides:
        want = seams.expected(case, stride, seams.host_row)
        got = launch(case, stride, fresh(case, stride))
        same("%s, stride %d" % (case.name, stride), got, want)
        again = launch(case, stride, fresh(case, stride))
        assert all(got[k].tobytes() == again[k].tobytes() for k in NAMES), (case.name, stride)
        if len(case.files) > 1:                                       # a launch per file into the same arrays: the same rows
            out = fresh(case, stride)
            for job in seams.split(case):
                apart = launch(job, stride, out)
            same("%s, stride %d, a launch per file" % (case.name, stride), apart, want)


def test_the_sentinels_would_show_a_stray_write():
    """the comparison above covers the unwritten rows: they are in `want` as sentinels, and `same` refuses a changed one"""
    case = next(c for c in CASES if c.name.startswith("tables"))
    want = seams.expected(case, 32, seams.host_row)
    for row in (7, 8, 14):
        assert (want["ids"][row] == seams.SENTINEL).all() and (want["is_onset"][row] == seams.SENTINEL & 255).all()
        assert want["lengths"][row] == seams.SENTINEL and want["truncated"][row] == seams.SENTINEL
    assert any(len(c.files) > 1 for c in CASES if c.name.startswith("advance"))
    got = {k: np.concatenate([v[7:8], v, v[7:8]]) for k, v in want.items()}    # row 7, unwritten, stands in for the guard rows
    same("intact", got, want)
    got["note_of"][1 + 8, 3] = -1
    with pytest.raises(AssertionError, match="note_of row 8 position 3"):
        same("a stray write", got, want)
    got["note_of"][1 + 8, 3] = seams.SENTINEL
    got["is_onset"][-1, 0] = 0
    with pytest.raises(AssertionError, match="outside the job's rows"):
        same("a stray write", got, want)
