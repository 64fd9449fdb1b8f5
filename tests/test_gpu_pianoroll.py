"""mt3_op_pianoroll / mt3_op_frame_counts and their Python layers (mt3_amd/pianoroll.py, metrics_utils, metrics,
InferenceModel.pianoroll) against the numpy restatement of the rule (tests/pianoroll_ref.py).  Everything is an integer:
every comparison is equality."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib, inference, metrics, metrics_utils, pianoroll  # noqa: E402
from mt3_amd.note_sequences import Note, NoteSequence  # noqa: E402
from tests import pianoroll_cases as cases  # noqa: E402
from tests import pianoroll_ref as ref  # noqa: E402

FPS = [62.5, 100.0]
DRUM = [False, True]
WIDTHS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3 * 1024 + 5]
WIDTH_FPS = 8.0          # one frame is 0.125 s: notes of whole frames are not touched by the 0.05 s rule, and k / 8 is exact


def _check_job(seqs, fps, is_drum):
    """pianorolls of the job == the restatement, roll by roll; returns both lists"""
    before = copy.deepcopy(seqs)
    got = pianoroll.pianorolls(seqs, fps, is_drum)
    want = [ref.pianoroll(s, fps, is_drum) for s in seqs]
    assert seqs == before and len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == torch.float32 and g.is_cuda and tuple(g.shape) == w.shape, (i, tuple(g.shape), w.shape)
        assert torch.equal(g.cpu().double(), torch.from_numpy(w)), "roll %d of %d" % (i, len(want))
    return got, want


# ------------------------------------------------------------------ rolls
@pytest.mark.parametrize("name,ns,fps,is_drum,want", cases.ROLL_CASES, ids=[c[0] for c in cases.ROLL_CASES])
def test_literals_through_the_device(name, ns, fps, is_drum, want):
    got = pianoroll.pianorolls([ns], fps, is_drum)[0]
    assert tuple(got.shape) == want.shape and torch.equal(got.cpu().double(), torch.from_numpy(want))


def _width_sequence(F, fps=WIDTH_FPS):
    """notes in whole frames [a, b): from column 0 into the last column, up to exactly F, and across every lane, wave and
    tile boundary of the scan that fits (the last column of a unit into the first of the next)"""
    at = lambda k: k / fps                              # noqa: E731
    spans = [(0, F - 1, 40), (0, F, 41), (F - 1, F, 42), (0, 1, 43)]
    for b in (4, 64, 256, 1024, 2048, 3072):
        spans += [(b - 1, b + 1, 50), (b - 1, b, 51), (b, b + 1, 52)]
    notes = [Note(at(a), at(b), pitch, 1 + (7 * a + b) % 120) for a, b, pitch in spans if 0 <= a < b <= F]
    notes += [Note(at(a), at(b), 50, 3, 9) for a, b, pitch in spans if pitch == 50 and b <= F]      # a second program on top
    return NoteSequence(notes=notes)


@pytest.mark.parametrize("F", WIDTHS)
def test_widths_around_the_scan_s_units(F):
    ns = _width_sequence(F)
    (got,), (want,) = _check_job([ns], WIDTH_FPS, False)
    assert got.shape[1] == F
    full = next(n for n in ns.notes if n.pitch == 41)
    assert want[41].tolist() == [full.velocity] * F                 # the note that ends exactly at F fills its row
    if F > 1:
        assert want[40, F - 2] != 0 and want[40, F - 1] == 0        # the one that ends in the last column stops before it
    _check_job([ns], WIDTH_FPS, True)                               # every note 0.05 s = 0.4 frames: mostly empty slices


def test_all_widths_in_one_job_at_odd_offsets():
    seqs = [_width_sequence(F) for F in WIDTHS]
    for is_drum in DRUM:
        got, _ = _check_job(seqs, WIDTH_FPS, is_drum)
    assert [g.shape[1] for g in pianoroll.pianorolls(seqs, WIDTH_FPS, False)] == WIDTHS


def test_rows_that_are_not_16_byte_aligned():
    """widths 5, 1023, 7: the second roll starts 128 * 5 floats in and its rows are 1023 floats apart, the third at
    128 * 1028: most rows of the job start off a 16-byte boundary"""
    seqs = [_width_sequence(5), _width_sequence(1023), _width_sequence(7)]
    got, _ = _check_job(seqs, WIDTH_FPS, False)
    assert [g.shape[1] for g in got] == [5, 1023, 7]
    base = got[0].data_ptr()
    assert got[1].data_ptr() - base == 4 * 128 * 5 and got[2].data_ptr() - base == 4 * 128 * 1028      # views of one buffer
    assert any((g[p].data_ptr() % 16) for g in got for p in range(3))


@pytest.mark.parametrize("fps", FPS)
def test_contention_is_exact_and_repeatable(fps):
    ns = NoteSequence(notes=[Note(0.5, 1.5, 64, 127, program=i % 128) for i in range(500)])
    (a,), (want,) = _check_job([ns], fps, False)
    b = pianoroll.pianorolls([ns], fps, False)[0]
    assert a[64, int(0.5 * fps)].item() == 63500.0 and a.max().item() == 63500.0
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert want[64, int(0.5 * fps):int(1.5 * fps)].tolist() == [63500.0] * (int(1.5 * fps) - int(0.5 * fps))


@pytest.mark.parametrize("fps", FPS)
@pytest.mark.parametrize("is_drum", DRUM)
def test_one_long_note_beside_many_short_ones(fps, is_drum):
    rng = np.random.default_rng(11)
    ns = cases.random_sequence(rng, 2000, 58.0, fps)
    ns.notes.insert(1000, Note(0.25, 60.25, 33, 90))
    (got,), _ = _check_job([ns], fps, is_drum)
    if not is_drum:
        assert got.shape[1] == int(fps * 60.25)
        assert bool((got[33, int(0.25 * fps):] >= 90).all().item())


@pytest.mark.parametrize("fps", FPS)
@pytest.mark.parametrize("is_drum", DRUM)
def test_a_job_of_nine_sequences_with_empty_ones(fps, is_drum):
    rng = np.random.default_rng(int(fps) + is_drum)
    sizes = [0, 300, 1, 700, 0, 5, 257, 1200, 0]
    seqs = [cases.random_sequence(rng, n, 1.0 + 3.0 * i, fps) for i, n in enumerate(sizes)]
    got, want = _check_job(seqs, fps, is_drum)
    assert [g.shape[1] for g in got][::4] == [0, 0, 0]
    assert sum(int((w != 0).sum()) for w in want) > 1000           # the comparison above was over real cells


def test_a_job_longer_than_one_launch_s_tables():
    """300 rolls: the tables go to the kernels 128 rolls at a time"""
    rng = np.random.default_rng(3)
    seqs = [cases.random_sequence(rng, int(rng.integers(0, 12)), 2.0, 62.5) for _ in range(300)]
    _check_job(seqs, 62.5, False)
    refs, ests = seqs[:150], seqs[150:]
    want = [ref.frame_counts(ref.pianoroll(r, 62.5, False), ref.pianoroll(e, 62.5, False), 30) for r, e in zip(refs, ests)]
    assert pianoroll.frame_counts(refs, ests).tolist() == [list(w) for w in want]


def test_pitch_128_is_refused_before_upload():
    with pytest.raises(ValueError, match="pitches 0 .. 127"):
        pianoroll.pianorolls([cases.ns_of((0.0, 1.0, 60, 80)), cases.ns_of((0.0, 1.0, 128, 80))])


def test_the_device_skips_what_the_host_would_refuse_and_stays_inside_its_span():
    """the ABI itself, on notes pianorolls() never uploads (pitch 128, pitch -1, a NaN time) and with widths NARROWER than
    the notes: such notes are skipped or cut at the row's end, the gap between the rolls is zeroed, and the sentinels in
    front of the span and behind it stay"""
    start = np.array([0.0, 0.0, 0.0, float("nan"), 0.5, 0.0], np.float64)
    end = np.array([100.0, 1.0, 1.0, 1.0, 1e300, 3.0], np.float64)
    pitch = np.array([5, 128, -1, 7, 9, 11], np.int32)
    vel = np.array([10, 20, 30, 40, 50, 60], np.int32)
    drum = np.zeros(6, np.int32)
    dev = [torch.from_numpy(a).cuda() for a in (start, end, pitch, vel, drum)]
    offs, cols, widths = np.array([0, 5, 6], np.int64), np.array([3, 40], np.int64), np.array([30, 6], np.int32)
    guard, cap = 128 * 3, 128 * 46
    out = torch.full((cap + 4096,), 12345.0, device="cuda", dtype=torch.float32)
    _lib.check(_lib.load().mt3_op_pianoroll(*[d.data_ptr() for d in dev], 6, 2, offs.ctypes.data, cols.ctypes.data,
                                            widths.ctypes.data, 10.0, 0, out.data_ptr(), cap,
                                            torch.cuda.current_stream().cuda_stream))
    y = out.cpu().numpy()
    assert (y[:guard] == 12345.0).all() and (y[cap:] == 12345.0).all()
    first = y[guard: guard + 128 * 30].reshape(128, 30)
    want = np.zeros((128, 30), np.float32)
    want[5, :] = 10                                    # 0 .. 100 s cut at the 30 columns of the row
    want[7, 0:10] = 40                                 # a NaN start counts as frame 0
    want[9, 5:] = 50                                   # 1e300 s cut at the row's end
    assert np.array_equal(first, want)
    assert not y[guard + 128 * 30: 128 * 40].any()     # the gap
    second = y[128 * 40: cap].reshape(128, 6)
    assert second[11].tolist() == [60.0] * 6 and second.sum() == 360.0


# ------------------------------------------------------------------ counts
def _seq_of_width(rng, F, fps, n=60):
    """random notes whose roll is exactly F columns wide at fps (F = 0: no notes)"""
    if F == 0:
        return NoteSequence()
    hi = (F + 0.25) / fps - 0.05                        # a note lengthened to 0.05 s still ends before frame F + 0.25
    notes = []
    for _ in range(n):
        start = float(rng.uniform(0.0, hi))
        notes.append(Note(start, float(rng.uniform(start, hi + 0.05)), int(rng.integers(0, 128)), int(rng.integers(1, 128)),
                          int(rng.integers(0, 128))))
    notes.append(Note(max(0.0, (F + 0.5) / fps - 0.3), (F + 0.5) / fps, 77, 99))
    return NoteSequence(notes=notes)


PAIR_WIDTHS = [(40, 90), (90, 40), (0, 70), (70, 0), (0, 0), (300, 300), (513, 2049)]     # 128 * 513 = 256 * 256.5


@pytest.mark.parametrize("fps", FPS)
def test_seven_pairs_in_one_call(fps):
    rng = np.random.default_rng(17)
    refs = [_seq_of_width(rng, a, fps) for a, _ in PAIR_WIDTHS]
    ests = [_seq_of_width(rng, b, fps) for _, b in PAIR_WIDTHS]
    rolls = [(ref.pianoroll(r, fps, False), ref.pianoroll(e, fps, False)) for r, e in zip(refs, ests)]
    assert [(r.shape[1], e.shape[1]) for r, e in rolls] == PAIR_WIDTHS
    for thr in (30, 0, 126):
        want = [list(ref.frame_counts(r, e, thr)) for r, e in rolls]
        got = pianoroll.frame_counts(refs, ests, fps, thr)
        assert got.dtype == np.int64 and got.shape == (7, 3) and got.tolist() == want
        for i in range(7):                                          # and pair by pair, one call each
            assert pianoroll.frame_counts(refs[i:i + 1], ests[i:i + 1], fps, thr).tolist() == [want[i]]
    assert want[4] == [0, 0, 0] and min(sum(w) for i, w in enumerate(want) if i != 4) > 0


@pytest.mark.parametrize("is_drum", DRUM)
def test_counts_with_drums(is_drum):
    rng = np.random.default_rng(23)
    refs = [cases.random_sequence(rng, 200, 5.0, 62.5) for _ in range(3)]
    ests = [cases.random_sequence(rng, 200, 6.0, 62.5) for _ in range(3)]
    want = [list(ref.frame_counts(ref.pianoroll(r, 62.5, is_drum), ref.pianoroll(e, 62.5, is_drum), 30))
            for r, e in zip(refs, ests)]
    assert pianoroll.frame_counts(refs, ests, 62.5, 30, is_drum).tolist() == want


@pytest.mark.parametrize("name,r,e,thr,counts,prf", cases.COUNT_CASES, ids=[c[0] for c in cases.COUNT_CASES])
def test_count_literals_and_frame_metrics(name, r, e, thr, counts, prf):
    assert pianoroll.roll_pair_counts(r, e, thr) == counts
    for a, b in ((r, e), (torch.from_numpy(r).cuda(), torch.from_numpy(e).float().cuda())):
        got = metrics_utils.frame_metrics(a, b, thr)
        assert isinstance(got, tuple) and all(type(x) is float for x in got) and got == prf


# ------------------------------------------------------------------ the layers above
@pytest.mark.parametrize("is_drum", DRUM)
def test_frame_scores(is_drum):
    rng = np.random.default_rng(29)
    pairs = [(cases.random_sequence(rng, 150, 4.0, 62.5), cases.random_sequence(rng, 150, 4.5, 62.5)) for _ in range(4)]
    pairs.append((NoteSequence(), pairs[0][1]))
    pairs.append((pairs[0][0], NoteSequence()))

    def drumless(ns):
        return ns if is_drum else NoteSequence(notes=[n for n in ns.notes if not n.is_drum])
    many = metrics.frame_scores_many(pairs, is_drum=is_drum)
    for (r, e), got in zip(pairs, many):
        p, rc, f = ref.frame_metrics(ref.pianoroll(drumless(r), 62.5, is_drum), ref.pianoroll(drumless(e), 62.5, is_drum), 30)
        assert got == {"Frame Precision": p, "Frame Recall": rc, "Frame F1": f}
        assert metrics.frame_scores(r, e, is_drum=is_drum) == got
    assert 0.0 < many[0]["Frame F1"] < 1.0
    assert many[4] == many[5] == {"Frame Precision": 0.0, "Frame Recall": 0.0, "Frame F1": 0.0}
    same = metrics.frame_scores(pairs[0][0], pairs[0][0], velocity_threshold=0, is_drum=is_drum)
    assert same == {"Frame Precision": 1.0, "Frame Recall": 1.0, "Frame F1": 1.0}


def test_reference_named_functions_and_the_model_s_method():
    ns = cases.random_sequence(np.random.default_rng(31), 100, 3.0, 62.5)
    before = copy.deepcopy(ns)
    for is_drum in DRUM:
        roll = metrics_utils.get_prettymidi_pianoroll(ns, 62.5, is_drum)
        want = ref.pianoroll(ns, 62.5, is_drum)
        assert isinstance(roll, np.ndarray) and roll.dtype == np.float64 and roll.shape == want.shape
        assert np.array_equal(roll, want)
    assert ns == before
    est = metrics_utils.get_prettymidi_pianoroll(cases.random_sequence(np.random.default_rng(37), 100, 3.5, 62.5), 62.5, False)
    assert metrics_utils.frame_metrics(want, est, 30) == ref.frame_metrics(want, est, 30)
    mine = inference.InferenceModel.pianoroll(ns, fps=100.0)
    assert mine.is_cuda and torch.equal(mine.cpu().double(), torch.from_numpy(ref.pianoroll(ns, 100.0, False)))
    rec = np.zeros(len(ns.notes), metrics_utils.NOTE_DTYPE)         # the record form decode_token_rows returns
    for i, n in enumerate(ns.notes):
        rec[i] = (n.start_time, n.end_time, n.pitch, n.velocity, n.program, n.is_drum, n.instrument, 0)
    assert torch.equal(pianoroll.pianorolls([rec], 100.0)[0], mine)
