"""CPU: the C ABI of the mapping sessions -- the header declares the entries, the built library exports them, _lib.ABI
lists them, sk_map_rec is 32 bytes, and every refusal the arguments alone decide is made before a device is looked for:
the same codes and messages on any machine.  No compute calls here."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

ENTRIES = ("sk_map_open", "sk_map_push", "sk_map_push_dev", "sk_map_reset", "sk_map_close", "sk_last_map_plan")


def test_header_declares_and_library_exports_the_entries():
    from squigglekit_amd import _lib, api
    text = open(os.path.join(ROOT, "include", "squigglekit_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.ABI
    for name, value in (("SK_MAP_MAX_SESSIONS", 8), ("SK_MAP_MAX_SLOTS", 65536), ("SK_MAP_MAX_TARGETS", 65536),
                        ("SK_MAP_MAX_CHUNK", 65536)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), code), name
        assert getattr(_lib, name) == value
    assert re.search(r"#define\s+SK_MAP_MAX_STATE_BYTES\s+\(\(int64_t\)1\s*<<\s*35\)", code)
    assert _lib.SK_MAP_MAX_STATE_BYTES == 1 << 35
    _lib.build()
    lib = C.CDLL(_lib.SO_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    # sk_map_rec: the fields of the header, 32 bytes, sk_hit's fields first and where sk_hit has them
    m = re.search(r"typedef struct sk_map_rec \{(.*?)\} sk_map_rec;", code, flags=re.S)
    fields = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"\b(double|int32_t)\b", "", m.group(1)))
    assert fields == list(_lib.MAPREC_DTYPE.names) == ["dist", "start", "end", "n", "flags", "rows", "pushes"]
    assert _lib.MAPREC_DTYPE.itemsize == 32 and api.MAPREC_DTYPE is _lib.MAPREC_DTYPE
    for f in _lib.HIT_DTYPE.names:
        assert _lib.MAPREC_DTYPE.fields[f][:2] == _lib.HIT_DTYPE.fields[f][:2], f


def err(L):
    return L.sk_last_error().decode()


def test_open_refusals_come_from_the_arguments_alone():
    from squigglekit_amd import _lib
    L = _lib.load()
    INV, UNS = _lib.SK_ERR_INVALID, _lib.SK_ERR_UNSUPPORTED
    vals = np.zeros(64)
    h = C.c_int32(-7)

    def open_(lens, nslots, values=vals, handle=h, off=None):
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64) if off is None else off
        return L.sk_map_open(None if values is None else _lib.ptr(values), None if off is False else _lib.ptr(off),
                             len(lens), nslots, None if handle is None else C.byref(handle))

    for lens, nslots, code, words in (
            ([10, 0, 5], 4, INV, ("target 1 is empty",)),
            ([10, 5], 0, INV, ("nslots = 0", "1 .. 65536")),
            ([10, 5], 65537, INV, ("nslots = 65537", "1 .. 65536")),
            ([10, 5], -3, INV, ("nslots = -3",)),
            ([], 4, INV, ("ntargets = 0", "1 .. 65536")),
            # 65 536 slots x 50 000 points x 12 bytes = 39 321 600 000 > 2^35
            ([20000, 30000], 65536, UNS, ("row state of 39321600000 bytes", "65536 slots", "50000 target points",
                                         "cap of 34359738368")),
            ([1] * 32768, 65536, UNS, ("nslots * ntargets = 2147483648", "1073741824"))):
        rc = open_(lens, nslots)
        assert rc == code and all(w in err(L) for w in words), (lens[:4], nslots, rc, err(L))
        assert h.value == -7                                            # nothing was written
    assert open_([10], 4, values=None) == INV and "NULL" in err(L)
    assert open_([10], 4, handle=None) == INV and "NULL" in err(L)
    assert open_([10], 4, off=False) == INV and "NULL" in err(L)
    assert open_([10, 5], 4, off=np.array([0, 10, 4], dtype=np.int64)) == INV and "target 1: bad length -6" in err(L)
    # the largest state under the cap passes the checks (and then needs a device)
    if L.sk_device_count() <= 0:
        assert open_([20000, 23687], 65536) == _lib.SK_ERR_NO_DEVICE, err(L)


def test_push_reset_close_refusals_come_from_the_arguments_alone():
    from squigglekit_amd import _lib
    L = _lib.load()
    INV, UNS = _lib.SK_ERR_INVALID, _lib.SK_ERR_UNSUPPORTED
    vals = np.zeros(8)                                                  # never followed: every call below is refused first
    out = np.full(32 * 8, 0xAB, dtype=np.uint8)
    i32 = lambda *v: np.array(v, dtype=np.int32)                        # noqa: E731
    i64 = lambda *v: np.array(v, dtype=np.int64)                        # noqa: E731

    def push(fn, handle, slots, off, values=vals, o=out, m=None):
        m = len(slots) if m is None else m
        return getattr(L, fn)(handle, None if slots is None else _lib.ptr(slots), m,
                              None if values is None else _lib.ptr(values), None if off is None else _lib.ptr(off),
                              None if o is None else _lib.ptr(o))

    for fn in ("sk_map_push", "sk_map_push_dev"):
        for handle in (-1, 8, 99):
            assert push(fn, handle, i32(0), i64(0, 2)) == INV and "handle %d is outside [0, 8)" % handle in err(L)
        assert push(fn, 0, i32(0), i64(0, 2), m=-1) == INV and "m < 0" in err(L)
        assert push(fn, 0, None, i64(0, 2), m=1) == INV and "NULL slots/off/out" in err(L)
        assert push(fn, 0, i32(0), None) == INV and "NULL slots/off/out" in err(L)
        assert push(fn, 0, i32(0), i64(0, 2), o=None) == INV and "NULL slots/off/out" in err(L)
        assert push(fn, 0, i32(0), i64(0, 2), values=None) == INV and "NULL values" in err(L)
        assert push(fn, 0, i32(0, 1), i64(0, 4, 2)) == INV and "entry 1: offsets not increasing" in err(L)
        rc = push(fn, 0, i32(0, 1, 2), i64(0, 65536, 65540, 65540 + 65537))
        assert rc == UNS and "entry 2: chunk of 65537 points" in err(L) and "65536" in err(L)
    # the slot numbers of the host form: outside the ABI's range, or twice
    for slots, words in ((i32(0, -1), ("entry 1: slot -1 is outside [0, 65536)",)),
                         (i32(65536), ("entry 0: slot 65536 is outside [0, 65536)",)),
                         (i32(3, 5, 3), ("entry 2: slot 3 appears twice",))):
        rc = push("sk_map_push", 0, slots, np.arange(len(slots) + 1, dtype=np.int64))
        assert rc == INV and all(w in err(L) for w in words), (slots, rc, err(L))
    assert np.all(out == 0xAB)
    # a handle inside the range is the session's to know: with a device "unknown mapping session handle", without one
    # the call ends where the device is looked for
    rc = push("sk_map_push", 3, i32(0), i64(0, 2))
    if L.sk_device_count() <= 0:
        assert rc == _lib.SK_ERR_NO_DEVICE, err(L)
    for handle in (-1, 8):
        assert L.sk_map_reset(handle, _lib.ptr(i32(0)), 1) == INV and "handle %d is outside" % handle in err(L)
        assert L.sk_map_close(handle) == INV and "handle %d is outside" % handle in err(L)
    assert L.sk_map_reset(0, None, 2) == INV and "NULL slots" in err(L)
    assert L.sk_map_reset(0, _lib.ptr(i32(0)), -1) == INV and "m < 0" in err(L)
    if L.sk_device_count() <= 0:
        assert L.sk_map_close(0) == _lib.SK_ERR_NO_DEVICE
        assert L.sk_last_map_plan(None, None, None) == _lib.SK_ERR_NO_DEVICE
