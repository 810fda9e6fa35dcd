"""CPU: the C ABI of the HMM sessions -- the header declares the entries with the signatures _lib.ABI binds, the built
library exports them, sk_hmms_rec is 96 bytes with the fields where the header puts them, and every refusal the arguments
alone decide is made before a device is looked for: the same codes and messages on any machine.  No compute calls here."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

ENTRIES = ("sk_hmms_open", "sk_hmms_push_i16", "sk_hmms_push_dev_i16", "sk_hmms_push_f64", "sk_hmms_push_dev_f64",
           "sk_hmms_reset", "sk_hmms_close", "sk_last_hmms_plan")
CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64}


def test_header_declares_and_library_exports_the_entries():
    from squigglekit_amd import _lib, api
    text = open(os.path.join(ROOT, "include", "squigglekit_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
        assert m, name
        res, argt = _lib.ABI[name]
        assert res is C.c_int
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == len(argt), (name, args)
        for a, t in zip(args, argt):                                   # pointers bind as pointers, integers by width
            if "*" in a:
                assert t is C.c_void_p or issubclass(t, C._Pointer), (name, a, t)
            else:
                assert t is CTYPE[a.split()[0]], (name, a, t)
    for name, value in (("SK_HMMS_MAX_SESSIONS", 8), ("SK_HMMS_MAX_SLOTS", 1048576)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), code), name
        assert getattr(_lib, name) == value
    _lib.build()
    lib = C.CDLL(_lib.SO_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert api.HmmStream and api.last_hmm_stream_plan and api.polya_decide


def test_record_is_96_bytes_with_the_headers_fields():
    from squigglekit_amd import _lib
    text = open(os.path.join(ROOT, "include", "squigglekit_hip.h")).read()
    body = re.search(r"typedef struct sk_hmms_rec \{(.*?)\} sk_hmms_rec;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = [d.strip() for d in body.split(";") if d.strip()]
    assert decl == ["double  score", "int32_t final_state, n_used", "int32_t enter[SK_HMM_STATES]", "double  v[SK_HMM_STATES]",
                    "int32_t pushes, flags"], decl
    dt = _lib.HMMS_DTYPE
    assert dt.itemsize == 96
    assert [(n, dt.fields[n][1]) for n in dt.names] == [("score", 0), ("final_state", 8), ("n_used", 12), ("enter", 16),
                                                        ("v", 40), ("pushes", 88), ("flags", 92)]
    # the first 40 bytes are sk_hmm_rec, field for field
    for n in _lib.HMM_DTYPE.names:
        assert dt.fields[n] == _lib.HMM_DTYPE.fields[n], n
    assert dt["v"].shape == (6,) and dt["enter"].shape == (6,) and _lib.SK_HMMS_MAX_SAMPLES == 0x7fffff00


def err(L):
    return L.sk_last_error().decode()


def good_model():
    from squigglekit_amd import api
    return api.polya_model("synth_raw")


def test_open_refusals_come_from_the_arguments_alone():
    from squigglekit_amd import _lib
    L = _lib.load()
    INV = _lib.SK_ERR_INVALID
    h = C.c_int32(-7)
    good = good_model()
    a = good.arrays()
    bad = []
    m = _lib.HmmModel.from_arrays(7, a["linit"], a["ltrans"], a["c"], a["mu"], a["h"])
    bad.append((m, "nstates must lie in [1, 6]"))
    li = a["linit"].copy(); li[:] = -np.inf
    bad.append((_lib.HmmModel.from_arrays(6, li, a["ltrans"], a["c"], a["mu"], a["h"]), "at least one linit must be finite"))
    lt = a["ltrans"].copy(); lt[2, 3] = np.nan
    bad.append((_lib.HmmModel.from_arrays(6, a["linit"], lt, a["c"], a["mu"], a["h"]), "ltrans must be finite or -inf"))
    hh = a["h"].copy(); hh[1, 0] = -1.0
    bad.append((_lib.HmmModel.from_arrays(6, a["linit"], a["ltrans"], a["c"], a["mu"], hh), "h must be finite and >= 0"))
    cc = a["c"].copy(); cc[0] = -np.inf
    bad.append((_lib.HmmModel.from_arrays(6, a["linit"], a["ltrans"], cc, a["mu"], a["h"]), "every state needs a component"))
    for model, words in bad:
        assert L.sk_hmms_open(C.byref(model), 4, C.byref(h)) == INV and "sk_hmm_model: " + words in err(L), err(L)
        assert h.value == -7
    assert L.sk_hmms_open(None, 4, C.byref(h)) == INV and "NULL sk_hmm_model" in err(L)
    assert L.sk_hmms_open(C.byref(good), 4, None) == INV and "NULL handle" in err(L)
    for nslots in (0, -3, 1048577):
        assert L.sk_hmms_open(C.byref(good), nslots, C.byref(h)) == INV and "nslots = %d" % nslots in err(L)
    assert h.value == -7
    if L.sk_device_count() <= 0:                                        # good arguments pass the checks and then need a device
        assert L.sk_hmms_open(C.byref(good), 1048576, C.byref(h)) == _lib.SK_ERR_NO_DEVICE, err(L)


def test_push_reset_close_refusals_come_from_the_arguments_alone():
    from squigglekit_amd import _lib
    L = _lib.load()
    INV, UNS = _lib.SK_ERR_INVALID, _lib.SK_ERR_UNSUPPORTED
    i32 = lambda *v: np.array(v, dtype=np.int32)                        # noqa: E731
    i64 = lambda *v: np.array(v, dtype=np.int64)                        # noqa: E731
    q = lambda a: None if a is None else _lib.ptr(a)                    # noqa: E731
    rows = np.zeros((3, 8), dtype=np.int16)                             # never followed: every call below is refused first
    vals = np.zeros(24)
    out = np.full(96 * 3, 0xAB, dtype=np.uint8)

    def push16(fn, handle, slots, lens, m=None, r=rows, stride=8, o=out):
        m = len(slots) if m is None else m
        return getattr(L, fn)(handle, q(slots), m, q(r), stride, q(lens), q(o))

    def push64(fn, handle, slots, off, m=None, v=vals, o=out):
        m = len(slots) if m is None else m
        return getattr(L, fn)(handle, q(slots), m, q(v), q(off), q(o))

    for fn in ("sk_hmms_push_i16", "sk_hmms_push_dev_i16"):
        for handle in (-1, 8, 99):
            assert push16(fn, handle, i32(0), i32(2)) == INV and "handle %d is outside [0, 8)" % handle in err(L)
        assert push16(fn, 0, i32(0), i32(2), m=-1) == INV and "m < 0" in err(L)
        assert push16(fn, 0, None, i32(2), m=1) == INV and "NULL slots/len" in err(L)
        assert push16(fn, 0, i32(0), None) == INV and "NULL slots/len" in err(L)
        assert push16(fn, 0, i32(0), i32(2), r=None) == INV and "NULL rows" in err(L)
        assert push16(fn, 0, i32(0), i32(2), o=None) == INV and "NULL out" in err(L)
        assert push16(fn, 0, i32(0), i32(2), stride=-8) == INV and "stride < 0" in err(L)
        assert push16(fn, 0, i32(0, 1), i32(2, 2), stride=1 << 31) == INV and "stride = 2147483648" in err(L)
        assert push16(fn, 0, i32(0, 1), i32(2, 2), m=1 << 20, stride=1 << 20) == UNS and "1048576 rows" in err(L)
    for fn in ("sk_hmms_push_f64", "sk_hmms_push_dev_f64"):
        for handle in (-1, 8, 99):
            assert push64(fn, handle, i32(0), i64(0, 2)) == INV and "handle %d is outside [0, 8)" % handle in err(L)
        assert push64(fn, 0, i32(0), i64(0, 2), m=-1) == INV and "m < 0" in err(L)
        assert push64(fn, 0, None, i64(0, 2), m=1) == INV and "NULL slots/off" in err(L)
        assert push64(fn, 0, i32(0), None) == INV and "NULL slots/off" in err(L)
        assert push64(fn, 0, i32(0), i64(0, 2), v=None) == INV and "NULL values" in err(L)
        assert push64(fn, 0, i32(0), i64(0, 2), o=None) == INV and "NULL out" in err(L)
    # what the host forms can read: the lengths, the offsets and the slot numbers
    for lens, words in ((i32(2, -1, 0), "entry 1: len = -1 is outside [0, stride = 8]"),
                        (i32(2, 3, 9), "entry 2: len = 9 is outside [0, stride = 8]")):
        assert push16("sk_hmms_push_i16", 0, i32(0, 1, 2), lens) == INV and words in err(L), err(L)
    assert push64("sk_hmms_push_f64", 0, i32(0, 1, 2), i64(0, 5, 4, 9)) == INV and "entry 1: off decreases" in err(L), err(L)
    for slots, words in ((i32(0, -1, 2), "entry 1: slot -1 is outside [0, 1048576)"),
                         (i32(1048576, 1, 2), "entry 0: slot 1048576 is outside [0, 1048576)"),
                         (i32(3, 5, 3), "entry 2: slot 3 appears twice")):
        assert push16("sk_hmms_push_i16", 0, slots, i32(1, 1, 1)) == INV and words in err(L), err(L)
        assert push64("sk_hmms_push_f64", 0, slots, i64(0, 1, 2, 3)) == INV and words in err(L), err(L)
        assert L.sk_hmms_reset(0, q(slots), 3, None) == INV and words in err(L), err(L)
    assert np.all(out == 0xAB)                                          # a refused push writes nothing
    # reset: the calibration pairs must be finite
    for cal, k in ((np.array([[0.0, 1.0], [np.nan, 1.0]]), 1), (np.array([[0.0, np.inf], [0.0, 1.0]]), 0),
                   (np.array([[0.0, 1.0], [3.0, -np.inf]]), 1)):
        assert L.sk_hmms_reset(0, q(i32(4, 5)), 2, q(cal)) == INV and "entry %d: the calibration pair" % k in err(L), err(L)
    for handle in (-1, 8):
        assert L.sk_hmms_reset(handle, q(i32(0)), 1, None) == INV and "handle %d is outside" % handle in err(L)
        assert L.sk_hmms_close(handle) == INV and "handle %d is outside" % handle in err(L)
    assert L.sk_hmms_reset(0, None, 2, None) == INV and "NULL slots" in err(L)
    assert L.sk_hmms_reset(0, q(i32(0)), -1, None) == INV and "m < 0" in err(L)
    # a handle inside the range is the session's to know: with a device "unknown HMM session handle", without one the call
    # ends where the device is looked for.  The refusals that need a session -- a handle that is not open, a slot at or
    # above nslots -- are pinned on the GPU (tests/test_gpu_hmmstream.py: test_lifecycle_and_session_refusals); a slot whose
    # total would pass 0x7fffff00 samples cannot be reached at test size and is not tested.
    if L.sk_device_count() <= 0:
        assert push16("sk_hmms_push_i16", 3, i32(0), i32(2)) == _lib.SK_ERR_NO_DEVICE, err(L)
        assert push64("sk_hmms_push_f64", 3, i32(0), i64(0, 2)) == _lib.SK_ERR_NO_DEVICE, err(L)
        assert L.sk_hmms_close(0) == _lib.SK_ERR_NO_DEVICE
        assert L.sk_last_hmms_plan(None, None) == _lib.SK_ERR_NO_DEVICE
