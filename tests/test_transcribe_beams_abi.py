"""mt3_engine_transcribe_beams on a box without a GPU: exported, typed, and every argument error the header lists that
needs no device comes back as MT3_ERR_INVALID with the function's name, before anything is written to h_stats.  (The two
rejections that need a finalized engine -- a decode in flight, a synthetic EOS schedule -- are in
tests/test_gpu_transcribe_beams.py.)"""
import ctypes as C
import subprocess
import sys

from mt3_amd import _lib

NAME = b"mt3_engine_transcribe_beams"


def _create(lib, **over):
    """an engine that is created but not finalized: its configuration is all the argument checks read"""
    cfg = dict(vocab_size=1536, emb_dim=512, num_heads=6, head_dim=64, mlp_dim=1024, num_encoder_layers=8,
               num_decoder_layers=8, input_depth=512, input_length=256, max_decode_len=1024, max_batch=16,
               compute_dtype=_lib.MT3_F32, decode_chains=1, kv_cache_dtype=0, dense_dtype=0, options=0)
    cfg.update(over)
    ec = _lib.EngineConfig(*[cfg[n] for n, _ in _lib.EngineConfig._fields_])
    h = C.c_void_p()
    assert lib.mt3_engine_create(C.byref(ec), C.byref(h)) == _lib.MT3_OK, lib.mt3_last_error()
    return h


def _rejected(lib, h, n_segments=4, k=4, steps=8, flags=0, x=1 << 20, ids=1 << 21):
    """the call with (never dereferenced) non-null buffers unless told otherwise; True when it is refused as specified"""
    st = _lib.TranscribeStats()
    st.slots = st.refills = -7
    rc = lib.mt3_engine_transcribe_beams(h, x, n_segments, k, steps, flags, ids, None, None, C.byref(st), None)
    return rc == _lib.MT3_ERR_INVALID and NAME in lib.mt3_last_error() and st.slots == -7 and st.refills == -7


def test_transcribe_beams_is_exported_and_typed():
    lib = _lib.load()
    assert "mt3_engine_transcribe_beams" in _lib.SIGNATURES and hasattr(lib, "mt3_engine_transcribe_beams")
    res, args = _lib.SIGNATURES["mt3_engine_transcribe_beams"]
    assert res is C.c_int and len(args) == 11 and args[9] == C.POINTER(_lib.TranscribeStats)
    assert lib.mt3_abi_version() == 4                       # an additive entry point


def test_null_engine_is_rejected():
    lib = _lib.load()
    for k, flags in ((4, 0), (0, 0), (9, 0), (2, _lib.DECODE_BEAM1)):
        assert _rejected(lib, None, k=k, flags=flags)


def test_bad_arguments_are_rejected_before_any_device_work():
    lib = _lib.load()
    h = _create(lib)
    try:
        for flags in (_lib.DECODE_BEAM1, _lib.DECODE_EARLY_EXIT, _lib.DECODE_ASYNC, 1 << 8, 1 << 20):
            assert _rejected(lib, h, flags=flags), flags
        for k in (0, -1, 9, 64):
            assert _rejected(lib, h, k=k), k
        assert _rejected(lib, h, x=None)
        assert _rejected(lib, h, ids=None)
        for n in (0, -3):
            assert _rejected(lib, h, n_segments=n), n
        for steps in (0, -1, 1025):
            assert _rejected(lib, h, steps=steps), steps
        # arguments in range reach the check that needs a device-side engine: still refused, the engine is not finalized
        assert _rejected(lib, h, flags=_lib.DECODE_NO_GRAPH | _lib.DECODE_SINGLE_STREAM)
        assert b"not finalized" in lib.mt3_last_error()
    finally:
        lib.mt3_engine_destroy(h)


def test_engine_shapes_the_beam_step_cannot_take_are_rejected():
    lib = _lib.load()
    for over, k, word in ((dict(max_batch=4), 8, b"max_batch"), (dict(vocab_size=2176), 4, b"vocab"),
                          (dict(num_decoder_layers=17), 4, b"16 decoder layers")):
        h = _create(lib, **over)
        try:
            assert _rejected(lib, h, k=k), over
            assert word in lib.mt3_last_error(), (over, lib.mt3_last_error())
        finally:
            lib.mt3_engine_destroy(h)


def test_command_line_lists_the_decoding_options():
    r = subprocess.run([sys.executable, "-m", "mt3_amd.transcribe", "--help"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "--decoding" in r.stdout and "--num-beams" in r.stdout
    assert "beam1" in r.stdout and "greedy" in r.stdout
