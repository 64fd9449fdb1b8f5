"""mt3_op_note_levels and mt3_op_level_velocities against the numpy rule (mt3_amd/velocity.py: levels_reference,
velocities_reference), bit for bit, on scripted log-mel: no frontend is involved in the first tests.  Then six notes of
known gain through the product's frontend and `estimate`, and `velocities=` through InferenceModel on the trained fixture.

Seeds: the log-mel rng 5; the notes of a levels case rng 100 + its note count; the levels of the velocity groups rng 7."""
import dataclasses
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib, note_arrays, note_sequences, spectrograms, velocity  # noqa: E402
from oracle import frontend  # noqa: E402
from tests import velocity_cases as cases  # noqa: E402

CKPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mt3_synthetic_ckpt.npz")
T, MEL = 16, 512
NAN = float("nan")


@pytest.fixture(scope="module")
def table():
    return velocity.harmonic_bins(frontend.mel_weight_matrix_tf32())


def scripted_logmel(rows, seed=5):
    """float32 [rows, 512] of mixed sign with +0.0, -0.0 and a few NaN"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 4.0, (rows, MEL)).astype(np.float32)
    x[rng.random(x.shape) < 0.01] = 0.0
    x[rng.random(x.shape) < 0.01] = -0.0
    x[rng.random(x.shape) < 0.002] = NAN
    return x


# three files of 2, 1 and 3 segments; file 0 fills its rows, so the rows after its last frame are file 1's; file 1 has no
# notes; file 2's last segment is short
SEGMENTS, N_FRAMES = (2, 1, 3), (32, 9, 41)
ROW0 = (0, 32, 48)


@pytest.fixture(scope="module")
def seamed():
    """(host log-mel, device log-mel): every row no note may read -- past a file's n_frames, and all of file 1 -- holds
    1e30, so a read across a seam shows in the level"""
    x = scripted_logmel(T * sum(SEGMENTS))
    for row0, segments, n in zip(ROW0, SEGMENTS, N_FRAMES):
        x[row0 + n: row0 + T * segments] = 1e30
    x[ROW0[1]: ROW0[2]] = 1e30
    return x, torch.from_numpy(x).cuda()


def level_job(n_notes):
    """n_notes notes over files 0 and 2: the frames start with 0, the last valid one, one past it and -1, the keys with
    pitches 0, 21, 60, 108, 127 and a drum; the rest is drawn"""
    rng = np.random.default_rng(100 + n_notes)
    counts = (n_notes // 2, 0, n_notes - n_notes // 2)
    frame, key = [], []
    for n, frames in zip(counts, N_FRAMES):
        special = [0, frames - 1, frames, -1, frames - 3, frames - 8, frames - 9, 2 ** 31 - 1]
        f = np.array((special + rng.integers(-2, frames + 2, max(n - len(special), 0)).tolist())[:n], np.int64)
        k = np.array(([0, 21, 60, 108, 127, 128] + rng.integers(0, 129, max(n - 6, 0)).tolist())[:n], np.int64)
        if n > 6:                                     # more drums than one in 129
            k[rng.random(n) < 0.15] = 128
        by = np.argsort(k == 128, kind="stable")      # the pitched notes first, as `pack` lays a file out
        frame.append(f[by])
        key.append(k[by])
    files = cases.files(*[(first, row0, n, int((k != 128).sum()), frames) for first, row0, n, k, frames in
                          zip(note_arrays.offsets(counts)[:-1], ROW0, counts, key, N_FRAMES)])
    velocity_in = [rng.integers(1, 128, n) for n in counts]
    return velocity.Packed(note_arrays.pack([frame, key, velocity_in], velocity.NOTE_LAYOUT), n_notes, files,
                           T * sum(SEGMENTS), [np.arange(n) for n in counts])


def columns(packed):
    n = packed.n_notes
    return [packed.notes[4 * n * k: 4 * n * (k + 1)].view("<i4") for k in range(3)]


def check_job(packed, host, dev, table, window=8, quantile=0.5, th=None):
    th = velocity.thresholds() if th is None else th
    got = velocity.run(packed, dev, MEL, *table, th, window, quantile)
    frame, key, velocity_in = columns(packed)
    level = velocity.levels_reference(host, packed.files, frame, key, *table, window=window)
    want = (level,) + velocity.velocities_reference(level, velocity_in, packed.files, th, quantile)
    for name, g, w in zip(("level", "velocity", "anchor", "measured"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=w.dtype == np.float64), name
    return got


@pytest.mark.parametrize("n_notes", [1, 7, 8, 9, 63, 65, 257])
def test_levels_equal_the_rule(seamed, table, n_notes):
    host, dev = seamed
    packed = level_job(n_notes)
    level = check_job(packed, host, dev, table)[0]
    assert np.nanmax(np.abs(level), initial=0.0) < 1e3                 # nothing was read across a seam
    frame, key, _ = columns(packed)
    for f, n_frames in ((0, N_FRAMES[0]), (2, N_FRAMES[2])):
        a, n = int(packed.files["first"][f]), int(packed.files["n_notes"][f])
        out = (frame[a: a + n] < 0) | (frame[a: a + n] >= n_frames) | (key[a: a + n] == 127)
        assert np.isnan(level[a: a + n][out]).all()
    if n_notes >= 63:
        assert (~np.isnan(level)).sum() > n_notes // 2


@pytest.mark.parametrize("window", [1, 3, 9, 64])
def test_levels_at_other_windows(seamed, table, window):
    host, dev = seamed
    check_job(level_job(65), host, dev, table, window=window)


def velocity_op(level, velocity_in, files, th, quantile):
    """mt3_op_level_velocities alone, on uploaded levels"""
    n, n_files = len(level), len(files)
    d_level, d_in = torch.from_numpy(level).cuda(), torch.from_numpy(velocity_in.astype(np.int32)).cuda()
    d_th = torch.from_numpy(th).cuda()
    d_out = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    d_anchor = torch.full((n_files, 2), 123.0, dtype=torch.float64, device="cuda")
    d_measured = torch.full((n_files, 2), -7, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().mt3_op_level_velocities(
        d_level.data_ptr(), n, files.ctypes.data, n_files, quantile, d_th.data_ptr(), d_in.data_ptr(), d_out.data_ptr(),
        d_anchor.data_ptr(), d_measured.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return d_out.cpu().numpy(), d_anchor.cpu().numpy(), d_measured.cpu().numpy()


def group_levels(rng, n, pattern):
    if pattern == "equal":
        return np.full(n, -1.25)
    if pattern == "ties":                             # runs of equal values across every rank
        return rng.integers(-2, 3, n).astype(np.float64) * 0.75
    if pattern == "signs":                            # negative and positive, +-0.0, tiny and huge: the 64-bit image
        x = rng.normal(0.0, 1.5, n) * 10.0 ** rng.integers(-3, 2, n)
        x[rng.random(n) < 0.05] = 0.0
        x[rng.random(n) < 0.05] = -0.0
        x[rng.random(n) < 0.02] = np.inf
        x[rng.random(n) < 0.02] = -np.inf
        x[rng.random(n) < 0.02] = 5e-324
        return x
    assert pattern == "holes"                         # measured and unmeasured notes mixed
    x = rng.normal(0.0, 1.0, n)
    x[rng.random(n) < 0.3] = NAN
    return x


@pytest.fixture(scope="module")
def velocity_job():
    """groups of 1, 2, 255, 256, 257 and 5000 notes in every pattern, a file with only drums, a file with only unmeasured
    notes, an empty file"""
    rng = np.random.default_rng(7)
    sizes = [(1, 2), (255, 256), (257, 5000), (2, 1), (256, 255), (5000, 257)]
    patterns = ["equal", "ties", "signs", "holes"]
    level, rows, first = [], [], 0
    for shift in range(4):
        for k, (n_pitched, n_drum) in enumerate(sizes):
            if shift and max(n_pitched, n_drum) == 5000 and shift != k % 4:
                continue                              # the 5000s: once per pattern is enough
            level += [group_levels(rng, n_pitched, patterns[(k + shift) % 4]),
                      group_levels(rng, n_drum, patterns[(k + shift + 1) % 4])]
            rows.append((first, 0, n_pitched + n_drum, n_pitched, 1))
            first += n_pitched + n_drum
    for n_pitched, n_drum, values in ((0, 10, rng.normal(0, 1, 10)), (4, 3, np.full(7, NAN)), (0, 0, np.zeros(0)),
                                      (3, 0, np.array([NAN, 2.0, NAN]))):
        level.append(values)
        rows.append((first, 0, n_pitched + n_drum, n_pitched, 1))
        first += n_pitched + n_drum
    level = np.concatenate(level)
    return level, rng.integers(1, 128, len(level)).astype(np.int32), cases.files(*rows)


@pytest.mark.parametrize("quantile", [0.0, 0.5, 1.0, 0.37])
def test_velocities_equal_the_rule(velocity_job, quantile):
    level, velocity_in, files = velocity_job
    th = velocity.thresholds()
    got = velocity_op(level, velocity_in, files, th, quantile)
    want = velocity.velocities_reference(level, velocity_in, files, th, quantile)
    for name, g, w in zip(("velocity", "anchor", "measured"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=w.dtype == np.float64), name
    velocities, anchor, measured = got
    unmeasured = np.isnan(level)
    assert np.array_equal(velocities[unmeasured], velocity_in[unmeasured])
    assert np.isnan(anchor[-3]).all() and measured[-3].tolist() == [0, 0]          # the file of unmeasured notes
    assert np.isnan(anchor[-4, 0]) and measured[-4].tolist() == [0, 10]            # the file with only drums
    assert len(set(velocities[~unmeasured].tolist())) > 40 and velocities.min() >= 1 and velocities.max() <= 127


def test_the_same_job_twice_gives_the_same_bytes_and_more_files_than_one_launch(seamed, table):
    """130 files (three launches of each kernel) that share the seamed log-mel's rows, run twice"""
    host, dev = seamed
    rng = np.random.default_rng(11)
    counts = rng.integers(0, 7, 130)
    frame = [rng.integers(-1, 42, n) for n in counts]
    key = [np.sort(rng.integers(0, 129, n)) for n in counts]            # 128, the drums, last
    rows = [(first, ROW0[f % 3], n, int((k != 128).sum()), N_FRAMES[f % 3])
            for f, (first, n, k) in enumerate(zip(note_arrays.offsets(counts)[:-1], counts, key))]
    packed = velocity.Packed(note_arrays.pack([frame, key, [np.full(n, 64) for n in counts]], velocity.NOTE_LAYOUT),
                             int(counts.sum()), cases.files(*rows), T * sum(SEGMENTS), [])
    one = check_job(packed, host, dev, table, quantile=0.25)
    two = velocity.run(packed, dev, MEL, *table, velocity.thresholds(), 8, 0.25)
    for a, b in zip(one, two):
        assert a.tobytes() == b.tobytes()
    big = level_job(257)
    one, two = (velocity.run(big, dev, MEL, *table, velocity.thresholds(), 8, 0.5) for _ in range(2))
    for a, b in zip(one, two):
        assert a.tobytes() == b.tobytes()


def six_note_sequence(onsets):
    return note_sequences.NoteSequence(notes=[note_sequences.Note(t, t + 0.2, 60, 100) for t in onsets], total_time=3.0)


def test_six_notes_through_the_products_frontend():
    onsets, samples = cases.six_notes()
    logmel = spectrograms.compute_spectrogram_batch(torch.from_numpy(samples.reshape(2, 32768)).cuda(), [256, 256])
    assert logmel.shape == (2, 256, 512)
    ns = six_note_sequence(onsets)
    out, records = velocity.estimate([logmel], [ns], return_levels=True, **cases.SIX_KW)
    level = records[0]["levels"]
    print("level - level[2] - ln(v / 60):", (level - level[2] - np.log(np.array(cases.SIX_VELOCITIES) / 60.0)).tolist())
    assert [n.velocity for n in out[0].notes] == list(cases.SIX_VELOCITIES)
    assert records[0]["anchors"][0] == level[2] and np.isnan(records[0]["anchors"][1])
    assert records[0]["measured"].tolist() == [6, 0]
    assert [dataclasses.replace(n, velocity=100) for n in out[0].notes] == ns.notes and out[0] is not ns
    assert [n.velocity for n in ns.notes] == [100] * 6                  # the caller's sequence is untouched
    # the (tensor, n_frames) form: the notes past the file's frames keep their velocity; two files in one job
    both = velocity.estimate([(logmel, 200), logmel], [ns, ns], **cases.SIX_KW)
    # the anchor is now the 40, rank floor(0.4 * 3) = 1 of 4: 1 + #{v : v - 0.5 <= 60 * gain / 40}
    assert [n.velocity for n in both[0].notes] == [30, 60, 90, 120, 100, 100]
    assert [n.velocity for n in both[1].notes] == list(cases.SIX_VELOCITIES)
    with pytest.raises(ValueError, match="n_frames must be 0 .. 512"):
        velocity.estimate([(logmel, 513)], [ns])
    with pytest.raises(ValueError, match="contiguous CUDA float32"):
        velocity.estimate([logmel.cpu()], [ns])
    with pytest.raises(ValueError, match="contiguous CUDA float32"):
        velocity.estimate([logmel[:, :, ::2]], [ns])


# ------------------------------------------------------------------------------------------- through the model
needs_fixture = pytest.mark.skipif(not os.path.exists(CKPT), reason="the trained fixture checkpoint is absent")


@needs_fixture
def test_velocities_through_the_model():
    from mt3_amd import checkpoints, inference, synthetic
    model = inference.InferenceModel(checkpoints.load_compact_npz(CKPT), "mt3", dtype="float32")
    _, wav = synthetic.synth_music(8.192, seed=21)
    plain = model(wav)
    flat, = {n.velocity for n in plain.notes}                           # one velocity bin: every decoded note has the same
    assert len(plain.notes) > 4
    got = model(wav, velocities=True)
    assert [dataclasses.replace(n, velocity=flat) for n in got.notes] == plain.notes
    assert dataclasses.replace(got, notes=plain.notes) == plain
    known = model.note_velocities(wav, plain)
    assert [n.velocity for n in got.notes] == [n.velocity for n in known.notes]
    again, record = model.note_velocities(wav, plain, return_levels=True)
    assert again == known and record["levels"].shape == (len(plain.notes),) and record["measured"][0] > 4
    assert all(n.velocity == flat for n, level in zip(known.notes, record["levels"]) if np.isnan(level))
    print("velocities:", sorted(n.velocity for n in got.notes))
    assert len({n.velocity for n in got.notes}) > 1
    assert model(wav) == plain                                          # no state is left behind
    # a dict of estimate's keywords; several files as one job, each ranked on its own
    soft = model(wav, velocities=dict(gamma=1.0, anchor_velocity=60))
    assert [n.velocity for n in soft.notes] == \
        [n.velocity for n in model.note_velocities(wav, plain, gamma=1.0, anchor_velocity=60).notes]
    assert [n.velocity for n in soft.notes] != [n.velocity for n in got.notes]
    half = wav[: 3 * 32768 // 2]
    many = model.transcribe_many([wav, half], velocities=True)
    assert many[0] == got and len(many[1].notes) > 2
    as_decoded = dataclasses.replace(many[1], notes=[dataclasses.replace(n, velocity=flat) for n in many[1].notes])
    assert model.note_velocities(half, as_decoded) == many[1] != as_decoded
    with pytest.raises(ValueError, match="velocities= takes"):
        model(wav, velocities=dict(loudness=1))


def test_a_model_that_decodes_velocities_refuses():
    from mt3_amd import inference, network
    cfg = network.T5Config(dtype="float32", num_encoder_layers=1, num_decoder_layers=1)
    model = inference.InferenceModel("random:0", "ismir2021", config=cfg)
    with pytest.raises(ValueError, match="one velocity bin"):
        model(np.zeros(16000, np.float32), velocities=True)
    with pytest.raises(ValueError, match="one velocity bin"):
        model.transcribe_many([np.zeros(16000, np.float32)], velocities={})
