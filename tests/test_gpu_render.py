"""mt3_op_render_notes and its Python layers (mt3_amd/render.py, InferenceModel.render) against the float64 restatement of
the rule (tests/render_ref.py, pinned by tests/test_render_ref.py).

The tolerance: |device - reference| <= 2^-16 on normalised output -- half a step of the int16 file the feature exists to
write -- and 2^-16 * max(1, peak / 0.9) on un-normalised output.  The float32 evaluation order itself stays within
2.3e-7 of the rule on the six-note and the late-note case (tests/test_render_arithmetic.py)."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib, inference, metrics_utils, render  # noqa: E402
from mt3_amd.note_sequences import Note, NoteSequence  # noqa: E402
from tests import render_cases as cases  # noqa: E402
from tests import render_ref as ref  # noqa: E402

RATE = cases.RATE
TOL = 2.0 ** -16
TILE = render.TILE


def _ns(notes):
    return NoteSequence(notes=[Note(n[0], n[1], n[2], n[3], 0, bool(n[4]) if len(n) > 4 else False) for n in notes])


def _close(got, want, bound, what=""):
    got = got.cpu().numpy().astype(np.float64) if hasattr(got, "cpu") else np.asarray(got, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    worst = float(np.abs(got - want).max()) if len(want) else 0.0
    print("%s: max |device - reference| = %.3g (bound %.3g)" % (what or "render", worst, bound))
    assert worst <= bound, (what, worst, bound)


def _check_job(note_lists, rate=RATE, lengths=None, normalize=True):
    """render() of the job against the restatement, sequence by sequence; returns the device tensors"""
    seqs = [_ns(n) for n in note_lists]
    before = copy.deepcopy(seqs)
    got = render.render(seqs, rate, lengths, normalize)
    assert seqs == before and len(got) == len(seqs)
    for i, (g, notes) in enumerate(zip(got, note_lists)):
        n = ref.length(notes, rate) if lengths is None else lengths[i]
        assert g.dtype == torch.float32 and g.is_cuda and tuple(g.shape) == (n,), (i, tuple(g.shape), n)
        want = ref.render(notes, rate, n, normalize)
        bound = TOL if normalize else TOL * max(1.0, ref.peak(notes, rate, n) / 0.9)
        _close(g, want, bound, "sequence %d of %d" % (i, len(seqs)))
    return got


def test_one_note():
    (x,) = _check_job([[(0.0, 0.3, 69, 100)]])
    assert x.shape[0] == 5440 and x[0].item() == 0.0 and x.abs().max().item() > 0.89


def test_phase_at_late_times():
    """0.2 s of pitch 96 from 590 s in a 600 s sequence: (k f0) t is in the millions of turns.  Time or phase in float32
    fails this by the whole amplitude."""
    (x,) = render.render([_ns(cases.LATE)], RATE, [cases.LATE_SAMPLES])
    assert x.shape[0] == cases.LATE_SAMPLES
    a, b = cases.LATE_WINDOW
    want = ref.render(cases.LATE, RATE, cases.LATE_SAMPLES, True, (a, b))
    assert np.abs(want).max() > 0.89 and np.count_nonzero(want) > 3000
    _close(x[a:b], want, TOL, "late note")
    assert not x[:a].any().item() and not x[b:].any().item()


def test_a_long_note_sounds_under_every_later_tile():
    """the lower end of the note range: one 30 s note first, then forty 0.1 s notes over the same 30 s.  Every tile's range
    must still begin at the long note, whose running reach covers them all."""
    notes = [(0.0, 30.0, 45, 127)] + [(0.3 + 0.74 * i, 0.4 + 0.74 * i, 60 + i % 24, 100) for i in range(40)]
    (x,) = _check_job([notes], normalize=False)
    without = ref.raw(notes[1:], RATE, len(x))
    t = 29.9                                                          # long after the last short note: only the long one sounds
    tail = x[int(t * RATE): int(t * RATE) + 2048].cpu().numpy()
    assert not without[int(t * RATE):].any() and np.abs(tail).max() > 1e-20


def test_onsets_offsets_and_release_ends_on_and_beside_tile_edges():
    """every note edge at a sample of index k * TILE - 1, k * TILE or k * TILE + 1 (and half a sample off those)"""
    at = lambda n: n / RATE                                           # noqa: E731
    notes = []
    for j, off in enumerate((-1, 0, 1, -0.5, 0.5)):
        notes.append((at(TILE + off), at(2 * TILE + 300 + 7 * j), 50 + j, 100))               # onset on / beside an edge
        notes.append((at(100 + j), at(3 * TILE + off), 60 + j, 90))                           # offset (release begins)
        notes.append((at(200 + j), at(4 * TILE + off) - 0.04, 70 + j, 80))                    # the release's end
        notes.append((at(5 * TILE + off), at(5 * TILE + off), 38 + j, 110, True))             # a drum onset
        notes.append((at(6 * TILE + off) - 0.15, 0.0 + at(6 * TILE), 42 + j, 110, True))      # a drum's last sample
    for normalize in (True, False):
        _check_job([notes], normalize=normalize)
    n = 4 * TILE + 3
    _check_job([notes, notes, notes], lengths=[TILE, TILE + 1, n])    # sequences that end on and beside an edge


def test_six_simultaneous_notes():
    (x,) = _check_job([cases.SIX])
    _check_job([cases.SIX], normalize=False)
    assert x.shape[0] == ref.length(cases.SIX, RATE) and x.abs().max().item() > 0.89


@pytest.mark.parametrize("rate", [8000, 44100])
def test_other_rates(rate):
    """8 kHz: pitch 100 keeps one partial, pitch 88 two; 44.1 kHz: a sample period that is not a binary fraction"""
    _check_job([[(0.0101, 0.2, 100, 100), (0.05, 0.25, 88, 90), (0.07, 0.1, 40, 127, True), (0.1, 0.3, 60, 80)]], rate)


def _random_notes(rng, n, seconds, drums=0.15):
    notes = []
    for _ in range(n):
        start = float(rng.uniform(0.0, seconds))
        notes.append((start, start + float(rng.uniform(0.0, 0.5)), int(rng.integers(21, 109)), int(rng.integers(0, 128)),
                      bool(rng.random() < drums)))
    return notes


def _five(rng):
    long_one = _random_notes(rng, 40, 3.0)
    cut, roomy = _random_notes(rng, 12, 1.0), _random_notes(rng, 6, 0.5)
    lists = [long_one, [], [(0.01, 0.02, 38, 127, True)], cut, roomy]
    lengths = [ref.length(long_one, RATE), 700, ref.length(lists[2], RATE), 9000, ref.length(roomy, RATE) + 5000]
    return lists, lengths


def _call(packed, n, offs, first, n_samples, out, normalize):
    notes = torch.from_numpy(packed).cuda()
    base = notes.data_ptr()
    peaks = torch.full((len(n_samples),), -3.0, device="cuda", dtype=torch.float32)
    _lib.check(_lib.load().mt3_op_render_notes(base, base + 8 * n, base + 16 * n, base + 24 * n, base + 28 * n, base + 32 * n,
                                               n, len(n_samples), offs.ctypes.data, first.ctypes.data, n_samples.ctypes.data,
                                               RATE, normalize, out.data_ptr(), out.numel() - 1000, peaks.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return peaks.cpu().numpy()


def test_a_job_of_five_sequences_between_sentinels():
    """the ABI itself: spans at odd offsets with gaps before, between and after them, which must come back untouched"""
    lists, lengths = _five(np.random.default_rng(5))
    packed, n, offs, n_samples = render._pack([_ns(x) for x in lists], RATE, lengths)
    assert n_samples.tolist() == lengths
    gaps = [333, 1, 17, 0, 1025]
    first = np.cumsum([g + m for g, m in zip(gaps, [0] + lengths[:-1])]).astype(np.int64)
    total = int(first[-1] + lengths[-1]) + 1000
    out = torch.full((total,), 12345.0, device="cuda", dtype=torch.float32)
    peaks = _call(packed, n, offs, first, n_samples, out, 1)
    y = out.cpu().numpy()
    mask = np.ones(total, bool)
    for i, (a, m, notes) in enumerate(zip(first, lengths, lists)):
        mask[a: a + m] = False
        _close(y[a: a + m], ref.render(notes, RATE, m), TOL, "span %d" % i)
        assert abs(peaks[i] - ref.peak(notes, RATE, m)) <= 1e-5 * max(1.0, peaks[i])       # d_peaks: the peak before scaling
    assert mask.sum() == sum(gaps) + 1000 and (y[mask] == 12345.0).all()
    assert not y[first[1]: first[1] + 700].any()                      # no notes, 700 samples: written, as zeros
    # the same through render(): views of ONE buffer, back to back
    got = _check_job(lists, lengths=lengths)
    assert [g.data_ptr() - got[0].data_ptr() for g in got] == [4 * int(v) for v in np.cumsum([0] + lengths[:-1])]


def test_unsorted_notes_and_a_wrong_reach_stay_inside_the_span():
    """what render() never uploads: notes out of order, a reach that is not a running maximum, pitches and times no caller
    should send.  The audio may be wrong; the sentinels around the span may not be touched and nothing may be read past
    the notes (the arrays end where the buffer ends)."""
    rng = np.random.default_rng(9)
    n = 300
    start = rng.uniform(0.0, 2.0, n)
    start[::50] = [np.nan, -1.0, 1e300, np.inf, 0.0, -np.inf]
    end = start + rng.uniform(-0.2, 0.5, n)
    reach = rng.uniform(0.0, 3.0, n)
    pitch = rng.integers(-5, 140, n).astype("<i4")
    velocity = rng.integers(-5, 140, n).astype("<i4")
    drum = rng.integers(0, 2, n).astype("<i4")
    packed = np.concatenate([a.view(np.uint8) for a in (start, end, reach, pitch, velocity, drum)])
    offs, first, n_samples = np.array([0, 120, n], np.int64), np.array([100, 40000], np.int64), np.array([30000, 5000], np.int64)
    out = torch.full((47000,), 12345.0, device="cuda", dtype=torch.float32)
    _call(packed, n, offs, first, n_samples, out, 1)
    y = out.cpu().numpy()
    assert (y[:100] == 12345.0).all() and (y[30100:40000] == 12345.0).all() and (y[45000:] == 12345.0).all()
    assert not (y[100:30100] == 12345.0).all()


def test_the_same_job_gives_the_same_bits_whatever_the_order_of_its_notes():
    rng = np.random.default_rng(7)
    lists = [_random_notes(rng, 60, 2.0), [], _random_notes(rng, 25, 1.0), [(0.0, 0.5, 60, 100)] * 3 + [(0.0, 0.5, 60, 99)]]
    a = render.render([_ns(x) for x in lists])
    b = render.render([_ns(x) for x in lists])
    shuffled = [[x[i] for i in rng.permutation(len(x))] for x in lists]
    assert shuffled[0] != lists[0]
    c = render.render([_ns(x) for x in shuffled])
    for u, v, w in zip(a, b, c):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)) and torch.equal(u.view(torch.int32), w.view(torch.int32))
    assert a[0].abs().max().item() > 0.89 and a[1].numel() == 0


def test_normalising():
    lists = [cases.SIX, [(0.0, 0.2, 60, 0), (0.1, 0.2, 38, 0, True)], [(0.0, 0.3, 69, 3)]]
    got = _check_job(lists)
    ulp = float(np.spacing(np.float32(0.9)))
    for i in (0, 2):
        peak = got[i].abs().max().item()
        print("sequence %d: peak %.9g" % (i, peak))
        assert abs(peak - float(np.float32(0.9))) <= ulp
    assert got[1].numel() == ref.length(lists[1], RATE) > 3800 and not got[1].any().item()      # silent stays zeros
    raw = _check_job(lists, normalize=False)
    assert abs(raw[0].abs().max().item() - ref.peak(cases.SIX, RATE)) < 1e-5 and not raw[1].any().item()


def test_render_wav_data_and_the_model_s_method():
    ns = _ns(cases.SIX + [(0.2, 0.21, 38, 120, True)])
    data = render.render_wav_data(ns)
    from scipy.io import wavfile
    import io
    rate, pcm = wavfile.read(io.BytesIO(data))
    want = ref.wav_samples(ref.render(ns, RATE))
    assert rate == RATE and pcm.dtype == np.int16 and pcm.shape == want.shape
    assert np.abs(pcm.astype(np.int64) - want).max() <= 1 and np.abs(pcm).max() in (29490, 29491)
    rate, pcm = wavfile.read(io.BytesIO(render.render_wav_data(ns, 22050)))
    assert rate == 22050 and np.abs(pcm.astype(np.int64) - ref.wav_samples(ref.render(ns, 22050))).max() <= 1
    mine = inference.InferenceModel.render(ns)
    assert mine.is_cuda and torch.equal(mine, render.render([ns])[0])
    rec = np.zeros(len(ns.notes), metrics_utils.NOTE_DTYPE)         # the record form decode_token_rows returns
    for i, n in enumerate(ns.notes):
        rec[i] = (n.start_time, n.end_time, n.pitch, n.velocity, n.program, n.is_drum, n.instrument, 0)
    assert torch.equal(render.render([rec])[0], mine)
