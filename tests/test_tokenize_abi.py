"""The target tokenizer's C entry points on a box without a GPU: symbols, prototypes, struct layouts and every argument
check of include/mt3_hip.h -- all of which come before any HIP call, so the "device" pointers here are host memory (or
null) that must come back untouched.  No CUDA call in this file."""
import ctypes as C
import inspect

import numpy as np
import pytest

from mt3_amd import _lib, inference, note_sequences, tokenize, transcribe, vocabularies

INVALID = _lib.MT3_ERR_INVALID


@pytest.fixture(scope="module")
def codec():
    return vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1))


def test_symbols_structs_and_version():
    lib, _P = _lib.load(), C.c_void_p
    for name in ("mt3_codec_tokenize_rule", "mt3_notes_tokenize", "mt3_op_tokenize_notes"):
        fn = getattr(lib, name)
        assert fn.restype is _lib.SIGNATURES[name][0] and list(fn.argtypes) == _lib.SIGNATURES[name][1]
    assert lib.mt3_abi_version() == 4
    assert C.sizeof(_lib.TokenizeRule) == 4 * (12 + 128)
    assert C.sizeof(_lib.TokenizeFile) == 24 == tokenize.FILE_DTYPE.itemsize
    assert C.sizeof(_lib.TokenizeRow) == 16 == tokenize.ROW_DTYPE.itemsize
    for struct, dtype in ((_lib.TokenizeFile, tokenize.FILE_DTYPE), (_lib.TokenizeRow, tokenize.ROW_DTYPE)):
        assert [(n, getattr(struct, n).offset) for n, _ in struct._fields_] == [(n, dtype.fields[n][1]) for n in dtype.names]


def test_rule_from_codec(codec):
    full = tokenize.tokenize_rule(codec, note_sequences.NoteEncodingWithTiesSpec, 1536, "full")
    assert (full.spec, full.vocab, full.max_shift_steps, full.shift_first) == (_lib.SPEC_TIES, 1536, 1000, 3)
    for name, event in (("pitch_first", "pitch"), ("velocity_first", "velocity"), ("tie_id", "tie"),
                        ("program_first", "program"), ("drum_first", "drum")):
        assert getattr(full, name) == codec.event_type_range(event)[0] + 3
    assert full.velocity_count == 2 and list(full.program_map) == list(range(128))
    assert list(tokenize.tokenize_rule(codec, note_sequences.NoteEncodingSpec, 1536, "midi_class").program_map) == \
        [8 * (p // 8) for p in range(128)]
    assert list(tokenize.tokenize_rule(codec, note_sequences.NoteEncodingSpec, 1536, "flat").program_map) == [-1] * 128
    lib, out = _lib.load(), _lib.TokenizeRule()
    for args, word in (((None, 2, 1536, 0, C.byref(out)), b"null"), ((C.byref(codec.desc), 2, 1536, 0, None), b"null"),
                       ((C.byref(codec.desc), _lib.SPEC_ONSETS, 1536, 0, C.byref(out)), b"spec"),
                       ((C.byref(codec.desc), 3, 1536, 0, C.byref(out)), b"spec"),
                       ((C.byref(codec.desc), 2, 1536, 3, C.byref(out)), b"granularity"),
                       ((C.byref(codec.desc), 2, 1000, 0, C.byref(out)), b"vocab")):
        assert lib.mt3_codec_tokenize_rule(*args) == INVALID
        assert lib.mt3_last_error().startswith(b"mt3_codec_tokenize_rule: ") and word in lib.mt3_last_error()
    with pytest.raises(ValueError):
        tokenize.tokenize_rule(codec, note_sequences.NoteOnsetEncodingSpec)


class _Job:
    """a well-formed call on host memory; `call(name=value)` swaps one argument, `rule(field=value)` one rule field"""

    def __init__(self, codec):
        self.codec = codec
        self.events = np.zeros((6, 8), np.int32)
        self.files = np.zeros(1, tokenize.FILE_DTYPE)
        self.files[0] = (0, 8, 0, 2, 0)
        self.rows = np.zeros(2, tokenize.ROW_DTYPE)
        self.out = np.full((5, 2 * 16), 7, np.int32)
        e, o = self.events, self.out
        self.args = dict(rule=self.rule(), step=e[0].ctypes.data, pitch=e[1].ctypes.data, program=e[2].ctypes.data,
                         velbin=e[3].ctypes.data, is_drum=e[4].ctypes.data, note=e[5].ctypes.data, n_events=8,
                         files=self.files.ctypes.data, n_files=1, rows_table=self.rows.ctypes.data, rows=2, stride=16,
                         ids=o[0].ctypes.data, lengths=o[1].ctypes.data, truncated=o[2].ctypes.data,
                         note_of=o[3].ctypes.data, is_onset=o[4].ctypes.data, stream=None)

    def rule(self, **fields):
        r = tokenize.tokenize_rule(self.codec, note_sequences.NoteEncodingWithTiesSpec, 1536)
        for k, v in fields.items():
            if k == "program_map":
                r.program_map[v[0]] = v[1]
            else:
                setattr(r, k, v)
        return r

    def call(self, **swap):
        a = dict(self.args, **swap)
        return _lib.load().mt3_op_tokenize_notes(
            None if a["rule"] is None else C.byref(a["rule"]), a["step"], a["pitch"], a["program"], a["velbin"], a["is_drum"],
            a["note"], a["n_events"], a["files"], a["n_files"], a["rows_table"], a["rows"], a["stride"], a["ids"],
            a["lengths"], a["truncated"], a["note_of"], a["is_onset"], a["stream"])

    def untouched(self):
        return (self.out == 7).all() and not self.events.any()


def test_op_rejects_bad_arguments_before_any_device_call(codec):
    lib, job = _lib.load(), _Job(codec)
    bad = [(dict(rule=None), b"null rule")]
    bad += [({name: None}, b"null event array") for name in ("step", "pitch", "program", "velbin", "is_drum", "note")]
    bad += [({name: None}, b"null table") for name in ("files", "rows_table")]
    bad += [({name: None}, b"null output") for name in ("ids", "lengths", "truncated", "note_of", "is_onset")]
    bad += [(dict(rows=0), b"rows"), (dict(rows=-3), b"rows"), (dict(n_files=0), b"n_files"), (dict(n_events=-1), b"n_events"),
            (dict(stride=1), b"stride"), (dict(stride=0), b"stride"), (dict(stride=-5), b"stride"),
            (dict(stride=(1 << 20) + 1), b"stride"),
            (dict(rule=job.rule(spec=_lib.SPEC_ONSETS)), b"spec"), (dict(rule=job.rule(spec=3)), b"spec"),
            (dict(rule=job.rule(max_shift_steps=0)), b"max_shift_steps"),
            (dict(rule=job.rule(velocity_count=0)), b"velocity_count"),
            (dict(rule=job.rule(program_map=(5, -2))), b"program_map"), (dict(rule=job.rule(program_map=(127, 128))), b"program_map"),
            (dict(rule=job.rule(vocab=3)), b"vocab"),
            (dict(rule=job.rule(shift_first=2)), b"id base"), (dict(rule=job.rule(shift_first=536)), b"id base"),
            (dict(rule=job.rule(pitch_first=1536 - 127)), b"id base"), (dict(rule=job.rule(pitch_first=0)), b"id base"),
            (dict(rule=job.rule(velocity_first=1535)), b"id base"), (dict(rule=job.rule(tie_id=1536)), b"id base"),
            (dict(rule=job.rule(tie_id=-1)), b"id base"), (dict(rule=job.rule(program_first=1536 - 127)), b"id base"),
            (dict(rule=job.rule(drum_first=2 ** 31 - 1)), b"id base"), (dict(rule=job.rule(vocab=1388)), b"id base")]
    for swap, word in bad:
        assert job.call(**swap) == INVALID, swap
        err = lib.mt3_last_error()
        assert err.startswith(b"mt3_op_tokenize_notes: ") and word in err, (swap, err)
    # all device pointers null: the argument checks come first, and a bad stride is still what is reported
    nulls = {name: None for name in ("step", "pitch", "program", "velbin", "is_drum", "note", "files", "rows_table", "ids",
                                     "lengths", "truncated", "note_of", "is_onset")}
    assert job.call(stride=1, **nulls) == INVALID and b"stride" in lib.mt3_last_error()
    assert job.call(rows=0, **nulls) == INVALID and b"rows" in lib.mt3_last_error()
    assert job.untouched()


def test_host_entry_point_rejects_the_same(codec):
    lib, job = _lib.load(), _Job(codec)
    ids, note_of, is_onset = np.zeros(16, np.int32), np.zeros(16, np.int32), np.zeros(16, np.uint8)
    length, cut = C.c_int32(), C.c_int32()
    e = job.events

    def call(rule, n_events=8, stride=16, step=e[0].ctypes.data, ids_ptr=ids.ctypes.data):
        return lib.mt3_notes_tokenize(None if rule is None else C.byref(rule), step, e[1].ctypes.data, e[2].ctypes.data,
                                      e[3].ctypes.data, e[4].ctypes.data, e[5].ctypes.data, n_events, 0, 2 ** 31 - 1, stride,
                                      ids_ptr, note_of.ctypes.data, is_onset.ctypes.data, C.byref(length), C.byref(cut))

    for kw, word in ((dict(rule=None), b"null rule"), (dict(rule=job.rule(), stride=1), b"stride"),
                     (dict(rule=job.rule(), n_events=-1), b"n_events"), (dict(rule=job.rule(), step=None), b"null event array"),
                     (dict(rule=job.rule(), ids_ptr=None), b"null output"), (dict(rule=job.rule(spec=0)), b"spec"),
                     (dict(rule=job.rule(program_map=(0, 200))), b"program_map")):
        assert call(**kw) == INVALID, kw
        assert lib.mt3_last_error().startswith(b"mt3_notes_tokenize: ") and word in lib.mt3_last_error()
    assert call(job.rule(), n_events=0, step=None) == _lib.MT3_OK and length.value == 2 and cut.value == 0
    assert ids[:3].tolist() == [job.rule().tie_id, 1, 0]


def test_python_surface_and_command_line(tmp_path):
    assert list(inspect.signature(tokenize.target_rows).parameters)[:7] == ["sequences", "n_frames", "codec", "spec", "granularity",
                                                                           "stride", "shifts"]
    assert list(inspect.signature(tokenize.target_rows_host).parameters)[:7] == \
        list(inspect.signature(tokenize.target_rows).parameters)[:7]
    assert list(inspect.signature(tokenize.target_rows_reference).parameters)[:5] == ["ns", "n_frames", "codec", "spec", "granularity"]
    assert list(inspect.signature(tokenize.pack).parameters)[:3] == ["sequences", "codec", "spec"]
    sn = inspect.signature(inference.InferenceModel.score_notes).parameters
    assert list(sn) == ["self", "audio", "ns", "sample_rate", "shifts", "granularity", "return_note_scores"]
    assert (sn["sample_rate"].default, sn["shifts"].default, sn["granularity"].default, sn["return_note_scores"].default) == \
        (16000, None, "full", False)
    assert callable(inference.InferenceModel.score_notes_many) and callable(inference.InferenceModel.targets)
    wav, refs = tmp_path / "tune.wav", tmp_path / "refs"
    wav.write_bytes(b"")                                   # plan() only checks that the files exist
    refs.mkdir()
    (refs / "tune.mid").write_bytes(b"")
    args, outputs = transcribe.plan(["--checkpoint", "random:0", "--score-midi", str(refs), "--score-shifts=-0.1,0,0.1", str(wav)])
    assert args.score_midi == str(refs) and args.score_shifts == [-0.1, 0.0, 0.1]
    assert transcribe.midi_scores_path(outputs) == str(tmp_path / "midi_scores.json")
    assert transcribe.plan(["--checkpoint", "random:0", str(wav)])[0].score_midi is None
    for argv in (["--score-midi", str(tmp_path)], ["--score-shifts", "0.1"], ["--score-midi", str(refs), "--score-shifts", "x"]):
        with pytest.raises(SystemExit):
            transcribe.plan(["--checkpoint", "random:0"] + argv + [str(wav)])
    rec = transcribe.midi_score_record("a.wav", {"loss": np.array([1.0, 2.0]), "best_shift": 0.0})
    assert rec == {"audio": "a.wav", "loss": [1.0, 2.0], "best_shift": 0.0}
