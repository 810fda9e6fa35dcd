"""CPU: the C ABI of the live mapping sessions -- the header declares the entries with the signatures _lib.ABI binds, the
built library exports them, the two records are 40 bytes, and every refusal the arguments alone decide is made before a
device is looked for: the same codes and messages on any machine.  No compute calls here."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

ENTRIES = ("sk_live_open", "sk_live_push_i16", "sk_live_push_dev_i16", "sk_live_fetch", "sk_live_hits", "sk_live_reset",
           "sk_live_close", "sk_last_live_plan", "sk_live_last_ms")
CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}


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
        for a, t in zip(args, argt):                                   # pointers bind as pointers, numbers by type
            if "*" in a:
                assert t is C.c_void_p or issubclass(t, C._Pointer), (name, a, t)
            else:
                assert t is CTYPE[a.split()[0]], (name, a, t)
    for name, value in (("SK_LIVE_MAX_SESSIONS", 8), ("SK_LIVE_MAX_CALIB", 8192)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), code), name
        assert getattr(_lib, name) == value
    m = re.search(r"enum\s*\{\s*SK_LIVE_CALIBRATING\s*=\s*0\s*,\s*SK_LIVE_MAPPING\s*=\s*1\s*,\s*SK_LIVE_UNDECIDABLE\s*=\s*2\s*\}", code)
    assert m and (_lib.SK_LIVE_CALIBRATING, _lib.SK_LIVE_MAPPING, _lib.SK_LIVE_UNDECIDABLE) == (0, 1, 2)
    _lib.build()
    lib = C.CDLL(_lib.SO_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert api.LiveMap and api.last_live_plan and api.live_rule
    assert _lib.LIVEINFO_DTYPE.itemsize == 40 and _lib.LIVEBEST_DTYPE.itemsize == 40
    assert C.sizeof(_lib.LiveRule) == 24
    # the structs as the header spells them: field names in order
    for struct, dtype in (("sk_live_info", _lib.LIVEINFO_DTYPE), ("sk_live_best", _lib.LIVEBEST_DTYPE)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), code, flags=re.S).group(1)
        names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
        assert tuple(names) == dtype.names, (struct, names)


def err(L):
    return L.sk_last_error().decode()


def test_open_refusals_come_from_the_arguments_alone():
    from squigglekit_amd import _lib
    L = _lib.load()
    INV, UNS = _lib.SK_ERR_INVALID, _lib.SK_ERR_UNSUPPORTED
    h = C.c_int32(-7)
    good = _lib.DetParams()
    tg = np.zeros(30, dtype=np.float64)
    toff = np.array([0, 10, 30], dtype=np.int64)

    def op(p=good, calib=40, t=tg, o=toff, T=2, S=4, hd=h):
        q = lambda a: None if a is None else _lib.ptr(a)                # noqa: E731
        return L.sk_live_open(None if p is None else C.byref(p), calib, q(t), q(o), T, S, None if hd is None else C.byref(hd))

    # sk_evs_open's first: the parameters, the handle
    assert op(p=_lib.DetParams(0, 6, 1.4, 9.0, 0.2)) == INV and "1 <= w_short <= w_long <= 64" in err(L)
    assert op(p=_lib.DetParams(3, 6, float("nan"), 9.0, 0.2)) == INV and "thresholds must be finite" in err(L)
    assert op(p=_lib.DetParams(3, 6, 1.4, 9.0, -0.1)) == INV and "peak_height" in err(L)
    assert op(p=None) == INV and "NULL" in err(L)
    assert op(hd=None) == INV and "NULL handle" in err(L)
    # the calibration length
    for calib in (-1, 0, 1, 8193):
        assert op(calib=calib) == INV and "calib = %d is outside 2 .. 8192" % calib in err(L), err(L)
    # then sk_map_open's: the targets, nslots, the caps
    assert op(t=None) == INV and "NULL targets/target_off" in err(L)
    assert op(o=None) == INV and "NULL targets/target_off" in err(L)
    for T in (0, 65537):
        assert op(T=T) == INV and "ntargets = %d is outside 1 .. 65536" % T in err(L)
    for S in (0, -3, 65537):
        assert op(S=S) == INV and "nslots = %d is outside 1 .. 65536" % S in err(L)
    assert op(o=np.array([0, 10, 10], dtype=np.int64)) == INV and "target 1 is empty" in err(L)
    assert op(o=np.array([0, 10, 5], dtype=np.int64)) == INV and "target 1: bad length -5" in err(L)
    big = np.array([0, 1 << 30], dtype=np.int64)
    assert op(o=big, T=1, S=65536) == UNS and "row state of" in err(L) and "above the cap" in err(L)
    # the order: a bad calib is named before bad targets, bad parameters before a bad calib
    assert op(calib=1, t=None) == INV and "calib = 1" in err(L)
    assert op(p=_lib.DetParams(7, 6, 1.4, 9.0, 0.2), calib=1) == INV and "w_short" in err(L)
    assert h.value == -7
    if L.sk_device_count() <= 0:                                        # good arguments pass the checks and then need a device
        assert op() == _lib.SK_ERR_NO_DEVICE, err(L)


def test_push_fetch_hits_reset_close_refusals_come_from_the_arguments_alone():
    from squigglekit_amd import _lib
    L = _lib.load()
    INV, UNS = _lib.SK_ERR_INVALID, _lib.SK_ERR_UNSUPPORTED
    i32 = lambda *v: np.array(v, dtype=np.int32)                        # noqa: E731
    rows = np.zeros((3, 8), dtype=np.int16)                             # never followed: every call below is refused first
    out = np.full(3 * 2 * 32, 0xAB, dtype=np.uint8)
    info = np.full(3 * 40, 0xAB, dtype=np.uint8)
    best = np.full(3 * 40, 0xAB, dtype=np.uint8)
    good = _lib.LiveRule(100, 400, 0.5, 0.05)
    NONE = object()

    def push(fn, handle, slots, lens, m=None, r=rows, stride=8, end=None, rule=None, o=out, nf=info, b=NONE):
        m = len(slots) if m is None else m
        q = lambda a: None if a is None else _lib.ptr(a)                # noqa: E731
        if b is NONE:
            b = best if rule is not None else None
        return getattr(L, fn)(handle, q(slots), m, q(r), stride, q(lens), q(end), None if rule is None else C.byref(rule),
                              q(o), q(nf), q(b))

    for fn in ("sk_live_push_i16", "sk_live_push_dev_i16"):
        for handle in (-1, 8, 99):
            assert push(fn, handle, i32(0), i32(2)) == INV and "live session handle %d is outside [0, 8)" % handle in err(L)
        # sk_evs_push_i16's, in its order
        assert push(fn, 0, i32(0), i32(2), m=-1) == INV and "m < 0" in err(L)
        assert push(fn, 0, i32(0), i32(2), stride=-8) == INV and "stride < 0" in err(L)
        assert push(fn, 0, None, i32(2), m=1) == INV and "NULL slots/len" in err(L)
        assert push(fn, 0, i32(0), None) == INV and "NULL slots/len" in err(L)
        assert push(fn, 0, i32(0), i32(2), r=None) == INV and "NULL rows" in err(L)
        assert push(fn, 0, i32(0, 1), i32(2, 2), stride=1 << 31) == INV and "stride = 2147483648" in err(L)
        assert push(fn, 0, i32(0, 1), i32(2, 2), m=1 << 20, stride=1 << 20) == UNS and "1048576 rows" in err(L)
        # the new ones
        assert push(fn, 0, i32(0), i32(2), o=None) == INV and "NULL out/info" in err(L)
        assert push(fn, 0, i32(0), i32(2), nf=None) == INV and "NULL out/info" in err(L)
        assert push(fn, 0, i32(0), i32(2), b=best) == INV and "best without a rule" in err(L)
        assert push(fn, 0, i32(0), i32(2), rule=good, b=None) == INV and "a rule without best" in err(L)
        for rule in (_lib.LiveRule(100, 400, float("nan"), 0.05), _lib.LiveRule(100, 400, 0.5, float("nan"))):
            assert push(fn, 0, i32(0), i32(2), rule=rule) == INV and "must be numbers" in err(L)
        for g in (0, -5):
            assert push(fn, 0, i32(0), i32(2), rule=_lib.LiveRule(100, g, 0.5, 0.05)) == INV and \
                "give_up_rows = %d is below 1" % g in err(L)
    # what the host form can read: the lengths and the slot numbers
    for lens, words in ((i32(2, -1, 0), "entry 1: len = -1 is outside [0, stride = 8]"),
                        (i32(2, 3, 9), "entry 2: len = 9 is outside [0, stride = 8]")):
        assert push("sk_live_push_i16", 0, i32(0, 1, 2), lens) == INV and words in err(L), err(L)
    for slots, words in ((i32(0, -1, 2), "entry 1: slot -1 is outside"),
                         (i32(3, 5, 3), "entry 2: slot 3 appears twice")):
        assert push("sk_live_push_i16", 0, slots, i32(1, 1, 1), rule=good) == INV and words in err(L), err(L)
    assert np.all(out == 0xAB) and np.all(info == 0xAB) and np.all(best == 0xAB)   # a refused push writes nothing
    if L.sk_device_count() <= 0:
        assert push("sk_live_push_i16", 3, i32(0), i32(2)) == _lib.SK_ERR_NO_DEVICE, err(L)
    # fetch, hits, reset, close
    off = np.full(4, -5, dtype=np.int64)
    vals = np.full(8, 7.0)
    hits = np.full(3 * 2 * 2 * 24, 0xAB, dtype=np.uint8)
    cnt = np.full(6, -9, dtype=np.int32)
    for handle in (-1, 8):
        assert L.sk_live_fetch(handle, _lib.ptr(off), _lib.ptr(vals), 8) == INV and "handle %d is outside" % handle in err(L)
        assert L.sk_live_hits(handle, _lib.ptr(i32(0)), 1, 2, np.inf, _lib.ptr(hits), _lib.ptr(cnt)) == INV and \
            "handle %d is outside" % handle in err(L)
        assert L.sk_live_reset(handle, _lib.ptr(i32(0)), 1) == INV and "handle %d is outside" % handle in err(L)
        assert L.sk_live_close(handle) == INV and "handle %d is outside" % handle in err(L)
    assert L.sk_live_fetch(0, None, _lib.ptr(vals), 8) == INV and "NULL off" in err(L)
    assert L.sk_live_fetch(0, _lib.ptr(off), _lib.ptr(vals), -1) == INV and "cap < 0" in err(L)
    assert L.sk_live_fetch(0, _lib.ptr(off), None, 4) == INV and "NULL values with a cap" in err(L)
    assert L.sk_live_hits(0, _lib.ptr(i32(0)), -1, 2, np.inf, _lib.ptr(hits), _lib.ptr(cnt)) == INV and "m < 0" in err(L)
    assert L.sk_live_hits(0, _lib.ptr(i32(0)), 1, 0, np.inf, _lib.ptr(hits), _lib.ptr(cnt)) == INV and "max_hits 0" in err(L)
    assert L.sk_live_hits(0, _lib.ptr(i32(0)), 1, 2, float("nan"), _lib.ptr(hits), _lib.ptr(cnt)) == INV and "max_dist is NaN" in err(L)
    assert L.sk_live_hits(0, None, 1, 2, np.inf, _lib.ptr(hits), _lib.ptr(cnt)) == INV and "NULL slots/out/count" in err(L)
    assert L.sk_live_hits(0, _lib.ptr(i32(1, 1)), 2, 2, np.inf, _lib.ptr(hits), _lib.ptr(cnt)) == INV and "appears twice" in err(L)
    assert L.sk_live_reset(0, None, 2) == INV and "NULL slots" in err(L)
    assert L.sk_live_reset(0, _lib.ptr(i32(0)), -1) == INV and "m < 0" in err(L)
    assert np.all(off == -5) and np.all(vals == 7.0) and np.all(hits == 0xAB) and np.all(cnt == -9)
    if L.sk_device_count() <= 0:
        assert L.sk_live_close(0) == _lib.SK_ERR_NO_DEVICE
        assert L.sk_live_fetch(0, _lib.ptr(off), _lib.ptr(vals), 8) == _lib.SK_ERR_NO_DEVICE
        assert L.sk_last_live_plan(None, None, None) == _lib.SK_ERR_NO_DEVICE
