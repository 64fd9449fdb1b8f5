"""mt3_op_tie_prompts alone (mt3_amd/csrc/ties.hip) against mt3_amd/ties.py: prompts, counts and held tables, exactly.

Row lengths 1, 7, 256, 1024 (one tile of the workgroup) and 1030 (the loop over tiles, the state carried across); 1, 3
and 65 rows; the toy descriptor (3 programs x 40 pitches: a ragged second word) and the (128, 128) one.  The scripted rows
hold every way the parallel form can go wrong; each batch of 65 rows is filled up with random rows, more than 200 per descriptor in all."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib, ties  # noqa: E402
from tests import note_grammar_ref as nr  # noqa: E402
from tests import note_grammar_script as ns  # noqa: E402

GRAMMARS = {"toy": ns.toy_notes(), "128x128": ns.toy_notes(128, 128)}
STRIDES = (1, 7, 256, 1024, 1030)


def _struct(n):
    s = _lib.NoteGrammar()
    for f in nr.FIELDS:
        setattr(s.g if hasattr(s.g, f) else s, f, getattr(n, f))
    return s


def _run(n, rows, cap, drop, held=True):
    lib = _lib.load()
    ids = torch.from_numpy(np.ascontiguousarray(rows, np.int32)).cuda()
    R = ids.shape[0]
    prompts = torch.full((R, 2 * cap + 1), -7, device="cuda", dtype=torch.int32)
    counts = torch.full((R,), -7, device="cuda", dtype=torch.int32)
    table = torch.full((R, nr.table_words(n)), -7, device="cuda", dtype=torch.int32) if held else None
    s = _struct(n)
    _lib.check(lib.mt3_op_tie_prompts(C.byref(s), ids.data_ptr(), R, ids.shape[1], cap, 1 if drop else 0,
                                      prompts.data_ptr(), counts.data_ptr(), table.data_ptr() if held else None,
                                      torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return prompts.cpu().numpy(), counts.cpu().numpy(), table.cpu().numpy().view(np.uint32) if held else None


def _check(n, rows, cap, drop, helds=None):
    prompts, counts, table = _run(n, rows, cap, drop)
    for i, row in enumerate(rows):
        held = helds[i] if helds is not None else ties.held_after(n, row)
        want, count = ties.tie_section(n, held, cap, drop)
        assert np.array_equal(table[i], held), (i, list(row[:40]))
        assert counts[i] == count, (i, list(row[:40]))
        assert np.array_equal(prompts[i], want), (i, list(row[:40]), list(prompts[i]), list(want))
    return counts


def _pad(rows, stride):
    out = np.zeros((len(rows), stride), np.int32)
    for i, r in enumerate(rows):
        r = np.asarray(r, np.int32)[:stride]
        out[i, : len(r)] = r
    return out


def _scripted(n, stride):
    """rows of `stride` ids (longer scripts are cut to it)"""
    P, Q, V0, V1, T, S = n.pitch_first, n.program_first, n.velocity_first, n.velocity_first + 1, n.tie_id, n.shift_first
    lastp, lastq = n.pitch_count - 1, n.program_count - 1
    rows = [
        # the same pair set and cleared several times: the last writer decides (cleared, then set)
        [T, Q + 1, V1, P + 5, V0, P + 5, V1, P + 5, V0, P + 5, 1],
        [T, Q + 1, V1, P + 5, V0, P + 5, V1, P + 5, V0, P + 5, V1, P + 5, S + 2, 1],
        # a program token between an onset and its note-off: the note-off goes to the OTHER program
        [T, Q, V1, P + 9, Q + 1, V0, P + 9, 1],
        [Q, P + 9, T, V1, Q + 1, P + 9, Q, V0, P + 9, 1],
        # velocity toggles with no pitch after them
        [T, V1, P + 3, V0, V1, V0, V1, 1],
        [T, V1, P + 3, V0, V1, V0, 1],
        # pitches in the last word of a row and in the last program
        [Q + lastq, P + lastp, P + lastp - 1, P + 32 % n.pitch_count, T, Q, V1, P + lastp, 1],
        # no tie: everything is a declaration, velocity 0 included
        [Q + 1, P + 1, V0, P + 2, Q, P + 1, V0, P + 1],
        [1, Q, P + 4, T],                                   # EOS at position 0
        [T, V1, P + 4, 0, P + 6, V0, P + 4, 1],             # a 0 before the end
        [P + 4, T, V1, P + 4, P + 4, 1],                    # an onset of an already held pitch
        [T, 1],                                             # nothing held
        [T, T, V0, P + 2, V1, P + 2, T, V0, P + 2],         # a second tie_id changes nothing
    ]
    if stride >= 1030:
        # the end, the first tie, the last program and the last velocity in DIFFERENT tiles: a declaration in tile 0, the
        # tie_id and the program in tile 0, the velocity 0 at the last position of tile 0, the note-offs in tile 1
        long = [S] * 1030
        long[0:3] = [Q + 1, P + 7, P + 8]
        long[5] = T
        long[1000:1003] = [V1, P + 9, Q + lastq]
        long[1023] = V0
        long[1024:1028] = [P + 9, Q + 1, P + 7, V1]
        long[1028] = P + lastp
        rows.append(long)
        late = [S] * 1030                                   # the tie_id itself in tile 1: tile 1's first pitches declare
        late[0:2] = [V0, P + 1]
        late[1024:1029] = [P + 2, T, P + 1, Q + 1, P + 1]
        rows.append(late)
    return _pad(rows, stride)


def _random_rows(n, rng, count, stride):
    top = n.drum_first + n.drum_count + 4
    out = np.zeros((count, stride), np.int32)
    for i in range(count):
        length = int(rng.integers(1, stride + 1))
        kind = rng.choice(5, size=length, p=[0.45, 0.15, 0.25, 0.1, 0.05])
        few = rng.integers(0, 2, size=length).astype(bool)
        pitch = np.where(few, rng.choice([0, 5, 31, 32 % n.pitch_count, n.pitch_count - 1], size=length),
                         rng.integers(0, n.pitch_count, size=length))
        prog = np.where(few, rng.choice([0, 1, n.program_count - 1], size=length), rng.integers(0, n.program_count, size=length))
        row = np.select([kind == 0, kind == 1, kind == 2, kind == 3],
                        [n.pitch_first + pitch, n.program_first + prog, n.velocity_first + rng.integers(0, 2, size=length),
                         n.shift_first + rng.integers(0, n.shift_count, size=length)], rng.integers(2, top, size=length))
        row[row == n.tie_id] = n.shift_first
        if i % 6:
            row[int(rng.integers(0, length))] = n.tie_id
        if i % 9 == 0:
            row[int(rng.integers(0, length))] = int(rng.integers(0, 2))
        out[i, :length] = row
    return out


@pytest.mark.parametrize("name", sorted(GRAMMARS))
@pytest.mark.parametrize("stride", STRIDES)
def test_kernel_equals_the_serial_replay(name, stride):
    n = GRAMMARS[name]
    rng = np.random.default_rng(100 + stride)
    scripted = _scripted(n, stride)
    batch = np.concatenate([scripted, _random_rows(n, rng, 65 - len(scripted), stride)])      # >= 40 random rows per stride
    assert len(batch) - len(scripted) >= 40
    for rows in (batch, batch[:3], batch[7:8]):
        helds = [ties.held_after(n, row) for row in rows]
        for drop in (False, True):
            for cap in (0, 2, 64):
                _check(n, rows, cap, drop, helds)


@pytest.mark.parametrize("name", sorted(GRAMMARS))
def test_exactly_cap_one_more_and_none(name):
    n = GRAMMARS[name]
    P, Q, T = n.pitch_first, n.program_first, n.tie_id
    pairs = [(0, 1), (0, 2), (1, 2), (n.program_count - 1, 0), (n.program_count - 1, n.pitch_count - 1)]
    row = [t for q, p in pairs for t in (Q + q, P + p)] + [T, 1]
    rows = _pad([row, [T, 1], row[:4] + [T]], 16)
    for drop in (False, True):
        for cap in (len(pairs), len(pairs) - 1, 0, 1):    # exactly cap, cap + 1 held, cap = 0
            counts = _check(n, rows, cap, drop)
            assert list(counts) == [len(pairs), 0, 2]
    prompts, counts, _ = _run(n, rows, 4, True, held=False)          # d_held == NULL
    assert list(counts) == [5, 0, 2] and prompts[1, 0] == T and not prompts[1, 1:].any()


def test_transformer_tie_prompts_wrapper():
    from mt3_amd import network
    n = GRAMMARS["128x128"]
    rows = torch.from_numpy(_random_rows(n, np.random.default_rng(1), 5, 64)).cuda()
    eng = network.Transformer.__new__(network.Transformer)          # tie_prompts needs the library, not an engine
    eng._lib, eng._h = _lib.load(), None
    prompts, counts, held = eng.tie_prompts(rows, _struct(n), cap=8, drop_redundant_programs=False, return_held=True)
    for i, row in enumerate(rows.cpu().numpy()):
        want, count = ties.tie_prompt(n, row, 8, False)
        assert np.array_equal(prompts[i].cpu().numpy(), want) and int(counts[i]) == count
        assert np.array_equal(held[i].cpu().numpy().view(np.uint32), ties.held_after(n, row))
    with pytest.raises(ValueError):
        eng.tie_prompts(rows.cpu(), _struct(n))
