"""CPU: the C ABI of the event sessions -- the header declares the entries with the signatures _lib.ABI binds, the built
library exports them, and every refusal the arguments alone decide is made before a device is looked for: the same codes
and messages on any machine.  No compute calls here."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

ENTRIES = ("sk_evs_open", "sk_evs_push_i16", "sk_evs_push_dev_i16", "sk_evs_fetch", "sk_evs_reset", "sk_evs_close",
           "sk_last_evs_plan")
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
    for name, value in (("SK_EVS_MAX_SESSIONS", 8), ("SK_EVS_MAX_SLOTS", 1048576)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), code), name
        assert getattr(_lib, name) == value
    _lib.build()
    lib = C.CDLL(_lib.SO_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert api.EventStream and api.last_event_plan
    assert _lib.DET_EVENT_DTYPE.itemsize == 24


def err(L):
    return L.sk_last_error().decode()


def test_open_refusals_come_from_the_arguments_alone():
    from squigglekit_amd import _lib
    L = _lib.load()
    INV = _lib.SK_ERR_INVALID
    h = C.c_int32(-7)
    good = _lib.DetParams()
    for p, words in ((_lib.DetParams(0, 6, 1.4, 9.0, 0.2), "1 <= w_short <= w_long <= 64"),
                     (_lib.DetParams(7, 6, 1.4, 9.0, 0.2), "1 <= w_short <= w_long <= 64"),
                     (_lib.DetParams(3, 65, 1.4, 9.0, 0.2), "1 <= w_short <= w_long <= 64"),
                     (_lib.DetParams(3, 6, float("nan"), 9.0, 0.2), "thresholds must be finite"),
                     (_lib.DetParams(3, 6, 1.4, float("inf"), 0.2), "thresholds must be finite"),
                     (_lib.DetParams(3, 6, 1.4, 9.0, -0.1), "peak_height"),
                     (_lib.DetParams(3, 6, 1.4, 9.0, float("nan")), "peak_height")):
        assert L.sk_evs_open(C.byref(p), 4, C.byref(h)) == INV and words in err(L), err(L)
        assert h.value == -7
    assert L.sk_evs_open(None, 4, C.byref(h)) == INV and "NULL" in err(L)
    assert L.sk_evs_open(C.byref(good), 4, None) == INV and "NULL" in err(L)
    for nslots in (0, -3, 1048577):
        assert L.sk_evs_open(C.byref(good), nslots, C.byref(h)) == INV and "nslots = %d" % nslots in err(L)
    assert h.value == -7
    if L.sk_device_count() <= 0:                                        # good arguments pass the checks and then need a device
        assert L.sk_evs_open(C.byref(good), 1048576, C.byref(h)) == _lib.SK_ERR_NO_DEVICE, err(L)


def test_push_fetch_reset_close_refusals_come_from_the_arguments_alone():
    from squigglekit_amd import _lib
    L = _lib.load()
    INV, UNS = _lib.SK_ERR_INVALID, _lib.SK_ERR_UNSUPPORTED
    i32 = lambda *v: np.array(v, dtype=np.int32)                        # noqa: E731
    rows = np.zeros((3, 8), dtype=np.int16)                             # never followed: every call below is refused first
    off = np.full(4, -5, dtype=np.int64)
    rec = np.full(24 * 8, 0xAB, dtype=np.uint8)

    def push(fn, handle, slots, lens, m=None, r=rows, stride=8, end=None, o=off, out=rec, cap=8):
        m = len(slots) if m is None else m
        q = lambda a: None if a is None else _lib.ptr(a)                # noqa: E731
        return getattr(L, fn)(handle, q(slots), m, q(r), stride, q(lens), q(end), q(o), q(out), cap)

    for fn in ("sk_evs_push_i16", "sk_evs_push_dev_i16"):
        for handle in (-1, 8, 99):
            assert push(fn, handle, i32(0), i32(2)) == INV and "handle %d is outside [0, 8)" % handle in err(L)
        assert push(fn, 0, i32(0), i32(2), m=-1) == INV and "m < 0" in err(L)
        assert push(fn, 0, None, i32(2), m=1) == INV and "NULL slots/len" in err(L)
        assert push(fn, 0, i32(0), None) == INV and "NULL slots/len" in err(L)
        assert push(fn, 0, i32(0), i32(2), r=None) == INV and "NULL rows" in err(L)
        assert push(fn, 0, i32(0), i32(2), o=None) == INV and "NULL off" in err(L)
        assert push(fn, 0, i32(0), i32(2), out=None) == INV and "NULL rec with a cap" in err(L)
        assert push(fn, 0, i32(0), i32(2), cap=-1) == INV and "cap < 0" in err(L)
        assert push(fn, 0, i32(0), i32(2), stride=-8) == INV and "stride < 0" in err(L)
        assert push(fn, 0, i32(0, 1), i32(2, 2), stride=1 << 31) == INV and "stride = 2147483648" in err(L)
        assert push(fn, 0, i32(0, 1), i32(2, 2), m=1 << 20, stride=1 << 20) == UNS and "1048576 rows" in err(L)
    # what the host form can read: the lengths and the slot numbers
    for lens, words in ((i32(2, -1, 0), "entry 1: len = -1 is outside [0, stride = 8]"),
                        (i32(2, 3, 9), "entry 2: len = 9 is outside [0, stride = 8]")):
        assert push("sk_evs_push_i16", 0, i32(0, 1, 2), lens) == INV and words in err(L), err(L)
    for slots, words in ((i32(0, -1, 2), "entry 1: slot -1 is outside [0, 1048576)"),
                         (i32(1048576, 1, 2), "entry 0: slot 1048576 is outside [0, 1048576)"),
                         (i32(3, 5, 3), "entry 2: slot 3 appears twice")):
        assert push("sk_evs_push_i16", 0, slots, i32(1, 1, 1)) == INV and words in err(L), err(L)
    assert np.all(off == -5) and np.all(rec == 0xAB)                    # a refused push writes nothing
    # a handle inside the range is the session's to know: with a device "unknown event session handle", without one the
    # call ends where the device is looked for.  The refusals that need a session -- a handle that is not open, a slot at
    # or above nslots, samples for an ended slot -- are pinned on the GPU (tests/test_gpu_evstream.py:
    # test_refusals_that_need_the_session, test_reset_mid_read_and_a_push_to_an_ended_slot); a slot whose total would pass
    # 2^31 - 1 samples cannot be reached at test size and is not tested.
    if L.sk_device_count() <= 0:
        assert push("sk_evs_push_i16", 3, i32(0), i32(2)) == _lib.SK_ERR_NO_DEVICE, err(L)
    for handle in (-1, 8):
        assert L.sk_evs_reset(handle, _lib.ptr(i32(0)), 1) == INV and "handle %d is outside" % handle in err(L)
        assert L.sk_evs_close(handle) == INV and "handle %d is outside" % handle in err(L)
        assert L.sk_evs_fetch(handle, _lib.ptr(rec), 8) == INV and "handle %d is outside" % handle in err(L)
    assert L.sk_evs_reset(0, None, 2) == INV and "NULL slots" in err(L)
    assert L.sk_evs_reset(0, _lib.ptr(i32(0)), -1) == INV and "m < 0" in err(L)
    assert L.sk_evs_fetch(0, _lib.ptr(rec), -1) == INV and "cap < 0" in err(L)
    assert L.sk_evs_fetch(0, None, 4) == INV and "NULL rec with a cap" in err(L)
    if L.sk_device_count() <= 0:
        assert L.sk_evs_close(0) == _lib.SK_ERR_NO_DEVICE
        assert L.sk_evs_fetch(0, _lib.ptr(rec), 8) == _lib.SK_ERR_NO_DEVICE
        assert L.sk_last_evs_plan(None, None, None) == _lib.SK_ERR_NO_DEVICE
