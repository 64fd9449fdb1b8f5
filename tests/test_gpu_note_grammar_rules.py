"""The NOTES instantiations of the token-rule kernels on scripted logits: mt3_op_token_steps_notes / mt3_op_beam_search_notes
on every case of tests/note_grammar_script.py against tests/note_grammar_ref.py.  Every free decision of every case is
separated by ten times the f32 score bound (beam_script.GAP), so ids, all k decodes, done flags, the packed grammar state,
the `note` int and the WHOLE table of sounding notes of every slot after every step must equal the reference exactly (a
wrong parent permutation or a missed fork shows in the tables); scores are held to beam_script.SCORE_TOL.  With a NULL
descriptor the drivers are the _grammar ones, bit for bit.  No case is skipped or filtered.

Shapes: three elements / rows, 12 to 16 steps; k in {1, 2, 8}; V = 70 (a ragged last mask word), 2048 (the register path's
edge), 2100 (the loop path, token kernel only); 3 programs x 40 pitches (a row of two words, the second ragged) and one
case at 128 x 128; with and without d_ss; max_len; a mask intersecting the rule; a prompt that forces disallowed tokens.
What the scripts reach is asserted here on the reference (and on the CPU in tests/test_note_grammar_ref.py)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib  # noqa: E402
from tests import beam_script as bs  # noqa: E402
from tests import grammar_ref as gr  # noqa: E402
from tests import grammar_script as gs  # noqa: E402
from tests import note_grammar_ref as nr  # noqa: E402
from tests import note_grammar_script as ns  # noqa: E402
from tests import sampling_script as ss  # noqa: E402

STRIDE = 4
_CASE = object()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _tables(prompts, masks, V):
    keep, rows, index = {}, [], []
    for p in prompts or []:
        if not p:
            index.append(-1)
            continue
        rows.append(list(p) + [0] * (STRIDE - len(p)))
        index.append(len(rows) - 1)
    if rows:
        keep["prompts"], keep["row_prompt"] = _dev(np.array(rows, np.int32)), _dev(np.array(index, np.int32))
    n_masks = 0
    if masks is not None:
        words, mi = gs.mask_words(masks, V)
        keep["masks"], keep["row_mask"], n_masks = _dev(words), _dev(mi), len(words)
    args = (_p(keep.get("masks")), n_masks, _p(keep.get("row_mask")), _p(keep.get("prompts")), STRIDE,
            _p(keep.get("row_prompt")))
    return keep, args


def _struct(n):
    return _lib.NoteGrammar(_lib.TokenGrammar(*[getattr(n, f) for f in gr.FIELDS]),
                            *[getattr(n, f) for f in nr.FIELDS[len(gr.FIELDS):]])


def _want_states(n, states):
    """reference states (Python ints) of one step -> (gram int32 [slots], note int32 [slots], held uint32 [slots][words])"""
    gram = np.array([nr.split(s)[0] for s in states], np.uint32).view(np.int32)
    note = np.array([nr.split(s)[1] for s in states], np.uint32).view(np.int32)
    return gram, note, np.stack([nr.held_words(n, s) for s in states])


def _beam(case, driver="notes", masks=_CASE, rc_only=False):
    k, n, T, V, E = case.k, case.elems * case.k, case.num_steps, case.V, case.elems
    W = nr.table_words(case.n)
    logits, scale = _dev(case.logits), (_dev(case.ss) if case.ss is not None else None)
    ids = torch.full((E, T), -7, dtype=torch.int32, device="cuda")
    all_ids = torch.full((E, k, T), -7, dtype=torch.int32, device="cuda")
    scores = torch.full((E, k), float("nan"), device="cuda")
    trace, live = np.full((T, 4, n), -9, np.int32), np.full((T, n), np.nan, np.float32)
    state, note, held = np.full((T, n), -9, np.int32), np.full((T, n), -9, np.int32), np.full((T, n, W), 0xDEAD, np.uint32)
    forks, ran = C.c_int32(-1), C.c_int32(-1)
    keep, tables = _tables(case.prompts, case.masks if masks is _CASE else masks, V)
    st = _struct(case.n)
    torch.cuda.synchronize()
    lib = _lib.load()
    head = (_p(logits), _p(scale), case.n_ss, case.dim, E, k, V, T, case.max_len, None, None, 0, _p(ids), _p(all_ids),
            _p(scores), None, trace.ctypes.data, live.ctypes.data, C.byref(forks), C.byref(ran), None)
    out = (state.ctypes.data, note.ctypes.data, held.ctypes.data)
    if rc_only:
        return lib.mt3_op_beam_search_notes(*head, *tables, C.byref(st), *out)
    if driver == "grammar":                             # the event grammar alone, through the _grammar driver
        _lib.check(lib.mt3_op_beam_search_grammar(*head, *tables, None, state.ctypes.data))
    else:
        _lib.check(lib.mt3_op_beam_search_notes(*head, *tables, C.byref(st) if driver == "notes" else None, *out))
    torch.cuda.synchronize()
    return dict(ids=ids.cpu().numpy(), all_ids=all_ids.cpu().numpy(), scores=scores.cpu().numpy(), trace=trace, live=live,
                forks=forks.value, ran=ran.value, state=state, note=note, held=held)


@pytest.mark.parametrize("case", ns.beam_cases(), ids=lambda c: c.name)
def test_notes_beam_search(case):
    got, ref = _beam(case), case.ref
    k, E = case.k, case.elems
    assert got["ran"] == ref.steps_run
    assert np.array_equal(got["all_ids"], ref.decodes), case.name
    assert np.array_equal(got["ids"], ref.decodes[:, -1])
    err = np.abs(got["scores"].astype(np.float64) - ref.scores)
    bound = bs.SCORE_TOL[0] + bs.SCORE_TOL[1] * np.abs(ref.scores)
    print("SCORE_ERR %s max_abs %.3e max_over_bound %.3f" % (case.name, err.max(), (err / bound).max()))
    assert (err <= bound).all(), (case.name, err.max())
    for t in range(ref.steps_run):
        gram, note, held = _want_states(case.n, ref.states[t])
        assert np.array_equal(got["state"][t], gram), (case.name, t)
        assert np.array_equal(got["note"][t], note), (case.name, t, got["note"][t], note)
        assert np.array_equal(got["held"][t], held), (case.name, t, np.argwhere(got["held"][t] != held)[:4])
        done = got["trace"][t, 2].reshape(E, k)
        assert np.array_equal(done, np.repeat(ref.retired[t].astype(np.int32)[:, None], k, 1)), (case.name, t)
    assert (got["note"][ref.steps_run:] == -9).all()
    plen = [0 if not p else len(p) for p in case.prompts]
    for b in range(E):                                   # every decode is note-consistent
        for d in got["all_ids"][b]:
            assert nr.accepts(case.n, d, plen[b]), (case.name, b, nr.first_rejected(case.n, d, plen[b]))
    null = _beam(case, driver="null")                    # NULL descriptor: the _grammar driver with a NULL grammar
    plain = _beam(case, driver="grammar")
    for key in ("ids", "all_ids", "trace", "forks", "ran"):
        assert np.array_equal(null[key], plain[key]), (case.name, key)
    assert np.array_equal(null["scores"].view(np.int32), plain["scores"].view(np.int32))
    assert np.array_equal(null["live"].view(np.int32), plain["live"].view(np.int32))
    assert (null["note"] == -9).all() and (null["held"] == 0xDEAD).all()
    assert not np.array_equal(null["all_ids"], got["all_ids"])          # the rule bit


def test_a_fork_copies_a_table_that_differs():
    """the k-beam scripts reach forks whose parent holds another table than the slot did (the reference says so; the kernel
    equalled the reference table for table in test_notes_beam_search)"""
    hits = {c.name: ns.fork_with_other_table(c) for c in ns.beam_cases() if c.k > 1}
    assert sum(hits.values()) >= 10 and sum(1 for v in hits.values() if v) >= 4, hits


def _token(case, mode, driver="notes", masks=_CASE, rc_only=False, sampling=None, streams=None, logits=None, scale="case",
           B=None, T=None, prompts=_CASE, max_len=None):
    B, T, V = B or case.elems, T or case.num_steps, case.V
    W = nr.table_words(case.n)
    logits = _dev(case.logits if logits is None else logits)
    scale = (_dev(case.ss) if case.ss is not None else None) if isinstance(scale, str) else scale
    ids = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    done, state = np.full((T, B), -9, np.int32), np.full((T, B), -9, np.int32)
    note, held = np.full((T, B), -9, np.int32), np.full((T, B, W), 0xDEAD, np.uint32)
    keep, tables = _tables(case.prompts if prompts is _CASE else prompts, case.masks if masks is _CASE else masks, V)
    st = _struct(case.n)
    sp = sampling.struct() if sampling is not None else None
    streams = np.ascontiguousarray(streams, dtype=np.uint64) if streams is not None else None
    torch.cuda.synchronize()
    lib = _lib.load()
    n_ss, dim = (case.n_ss, case.dim) if scale is not None else (0, 0)
    head = (_p(logits), _p(scale), n_ss, dim, B, V, T, mode, case.max_len if max_len is None else max_len, _p(ids),
            done.ctypes.data, None)
    samp = (C.byref(sp) if sp is not None else None, streams.ctypes.data if streams is not None else None)
    if rc_only:
        return lib.mt3_op_token_steps_notes(*head, *tables, C.byref(st), state.ctypes.data, *samp, note.ctypes.data,
                                            held.ctypes.data)
    if driver == "grammar":
        _lib.check(lib.mt3_op_token_steps_sampled(*head, *tables, None, state.ctypes.data, *samp))
    else:
        _lib.check(lib.mt3_op_token_steps_notes(*head, *tables, C.byref(st) if driver == "notes" else None,
                                                state.ctypes.data, *samp, note.ctypes.data, held.ctypes.data))
    torch.cuda.synchronize()
    return dict(ids=ids.cpu().numpy(), done=done, state=state, note=note, held=held, left=logits.cpu().numpy())


@pytest.mark.parametrize("mode", (0, 1), ids=("greedy", "beam1"))
@pytest.mark.parametrize("case", ns.token_cases(), ids=lambda c: c.name)
def test_notes_token_steps(case, mode):
    got = _token(case, mode)
    T = case.num_steps
    if mode == 0:
        scaled = np.stack([case.scaled(t) for t in range(T)])
        want_ids, want_done, states = nr.greedy(scaled, case.prompts, case.n, case.masks, case.max_len)
        assert np.array_equal(got["ids"], want_ids) and np.array_equal(got["done"], want_done), case.name
        steps = T
    else:
        ref = case.ref
        assert np.array_equal(got["ids"], ref.decodes[:, 0]), case.name
        for t in range(T):
            want = ref.retired[t] if t < ref.steps_run else np.ones(case.elems, bool)
            assert np.array_equal(got["done"][t], want.astype(np.int32)), (case.name, t)
        states, steps = ref.states, ref.steps_run
    for t in range(steps):
        gram, note, held = _want_states(case.n, states[t])
        assert np.array_equal(got["state"][t], gram), (case.name, t)
        assert np.array_equal(got["note"][t], note), (case.name, t, got["note"][t], note)
        assert np.array_equal(got["held"][t], held), (case.name, t, np.argwhere(got["held"][t] != held)[:4])
    plen = [0 if not p else len(p) for p in case.prompts]
    for b in range(case.elems):
        assert nr.accepts(case.n, got["ids"][b], plen[b]), (case.name, b)
    # the logits in memory stay the model's own, and a NULL descriptor is the _grammar driver with a NULL grammar
    plain, null = _token(case, mode, driver="grammar"), _token(case, mode, driver="null")
    assert np.array_equal(got["left"], plain["left"])
    for key in ("ids", "done", "left"):
        assert np.array_equal(null[key], plain[key]), (case.name, key)
    assert (null["note"] == -9).all() and (null["held"] == 0xDEAD).all() and not np.array_equal(null["ids"], got["ids"])


def test_the_scripts_reach_what_they_are_for():
    """over the greedy references of the token cases: a note-off refused, a double tie refused, a drum at velocity 0 refused
    (each time the runner-up was taken: the rows are accepted), a program switch between an onset and its offset; a prompt
    that forces disallowed tokens; a mask that intersects the rule"""
    found = set()
    for case in ns.token_cases():
        scaled = np.stack([case.scaled(t) for t in range(case.num_steps)])
        ids, _, _ = nr.greedy(scaled, case.prompts, case.n, case.masks, case.max_len)
        found |= ns.coverage(case, ids)
    assert found >= {"noteoff", "double_tie", "drum", "switch"}, found
    breaks = next(c for c in ns.token_cases() if c.name == "nt_v70_breaks")
    assert not nr.accepts(breaks.n, ns.PROMPT_BREAKS + [1], 0) and nr.accepts(breaks.n, ns.PROMPT_BREAKS + [1], 4)
    masked = next(c for c in ns.token_cases() if c.name == "nt_mask_v70")
    s0 = nr.initial(masked.n)
    both = nr._rule_vector(masked.n, s0, masked.masks[0], 70)
    assert both.sum() < nr._rule_vector(masked.n, s0, None, 70).sum() and both.sum() < masked.masks[0].sum()


@pytest.mark.parametrize("mode", (ss.MODES[0], ss.MODES[2], ss.MODES[5]), ids=lambda m: m[0])
def test_notes_sampled(mode):
    """sample_step_kernel's NOTES form on sampling_script's `tables` case (masks, prompts, max_len) under the toy note
    grammar: every pick of the reference meets sampling_script's margins (asserted before the GPU is asked), so the ids and
    done flags are equal, and so is the note state of every row while it is live"""
    sc = ns.SampledCase(300, mode)
    c, n = sc.case, sc.n
    assert len(c.margins) >= 15
    for b, t, m in c.margins:
        assert m["pick"] >= ss.PICK_MARGIN and m["boundary"] >= ss.BOUNDARY_MARGIN and m["mass"] >= ss.MASS_MARGIN, (b, t, m)

    class View:                                          # what _token reads of a case
        pass

    v = View()
    v.elems, v.num_steps, v.V, v.n, v.logits, v.ss, v.n_ss, v.dim = ss.ROWS, ss.STEPS, c.V, n, c.logits, c.ss, c.n_ss, c.dim
    v.prompts, v.masks, v.max_len = c.prompts, c.masks, c.max_len
    got = _token(v, 0, sampling=c.params, streams=c.streams)
    assert np.array_equal(got["ids"], c.ids), (sc.name, np.argwhere(got["ids"] != c.ids)[:5])
    assert np.array_equal(got["done"], c.done)
    for b in range(ss.ROWS):
        state = nr.initial(n)
        for t in range(ss.STEPS):
            if t and c.done[t - 1, b]:
                break
            state = nr.advance(n, state, int(c.ids[b, t]))
            gram, note, held = _want_states(n, [state])
            assert got["state"][t, b] == gram[0] and got["note"][t, b] == note[0], (sc.name, b, t)
            assert np.array_equal(got["held"][t, b], held[0]), (sc.name, b, t)
        plen = len(c.prompts[b]) if c.prompts[b] else 0
        assert nr.accepts(n, c.ids[b], plen), (sc.name, b)
    greedy = _token(v, 0, driver="notes")
    assert not np.array_equal(greedy["ids"], got["ids"])     # it samples


def test_drivers_refuse_a_mask_that_leaves_the_rule_no_room():
    """MT3_ERR_INVALID for a mask that leaves the worst state after the tie section -- velocity zero, nothing held: no pitch
    and no drum id -- fewer than 2 (token kernel) / 2k (beam kernel) ids, though the event grammar alone has room"""
    lib = _lib.load()
    tok, b2 = next(c for c in ns.token_cases() if c.name == "nt_v70"), next(c for c in ns.beam_cases() if c.name == "n_v70_k2")
    n = tok.n
    pitch_drum = set(range(n.pitch_first, n.pitch_first + n.pitch_count)) | set(range(n.drum_first, n.drum_first + n.drum_count))
    # EOS, the tie, the pitches and drums and one velocity: after a shift the grammar alone allows 1 + 40 + 3 + 1 ids, the
    # note rule EOS and the velocity: 2
    two = gs._mask(70, [i for i in range(70) if i not in pitch_drum | {1, n.tie_id, n.velocity_first}])
    one = gs._mask(70, [i for i in range(70) if i not in pitch_drum | {1, n.tie_id}])
    for mode in (0, 1):
        assert _token(tok, mode, masks=[two, None, None], rc_only=True) == _lib.MT3_OK
        assert _token(tok, mode, masks=[None, None, one], rc_only=True) == _lib.MT3_ERR_INVALID
        assert b"mt3_op_token_steps_notes" in lib.mt3_last_error() and b"fewer than" in lib.mt3_last_error()
    assert _beam(b2, masks=[two, None, None], rc_only=True) == _lib.MT3_ERR_INVALID                      # 2 < 2k = 4
    assert b"mt3_op_beam_search_notes" in lib.mt3_last_error() and b"fewer than" in lib.mt3_last_error()
    assert _beam(b2, masks=None, rc_only=True) == _lib.MT3_OK
