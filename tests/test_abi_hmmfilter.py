"""CPU: the C ABI of the filtered HMM sessions -- the header declares sk_hmms_open_ex, sk_hmms_filter and
sk_hmms_filter_dev with the signatures _lib.ABI binds, the built library exports them, sk_hmms_filt is 64 bytes with the
fields where the header puts them, and every refusal the arguments alone decide is made before a device is looked for: the
same codes and messages on any machine.  No compute calls here."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

ENTRIES = ("sk_hmms_open_ex", "sk_hmms_filter", "sk_hmms_filter_dev")
CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64}


class Filt(C.Structure):
    """sk_hmms_filt as a C compiler lays it out"""
    _fields_ = [("loglik", C.c_double), ("n_used", C.c_int32), ("flags", C.c_int32), ("post", C.c_double * 6)]


def err(L):
    return L.sk_last_error().decode()


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
        for a, t in zip(args, argt):
            if "*" in a:
                assert t is C.c_void_p or issubclass(t, C._Pointer), (name, a, t)
            else:
                assert t is CTYPE[a.split()[0]], (name, a, t)
    assert re.search(r"#define\s+SK_HMMS_FILTER\s+1\b", code) and _lib.SK_HMMS_FILTER == 1
    _lib.build()
    lib = C.CDLL(_lib.SO_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert api.HmmStream.filter and api.polya_decide_post


def test_filter_record_is_64_bytes_with_the_headers_fields():
    from squigglekit_amd import _lib
    text = open(os.path.join(ROOT, "include", "squigglekit_hip.h")).read()
    body = re.search(r"typedef struct sk_hmms_filt \{(.*?)\} sk_hmms_filt;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = [d.strip() for d in body.split(";") if d.strip()]
    assert decl == ["double  loglik", "int32_t n_used, flags", "double  post[SK_HMM_STATES]"], decl
    assert C.sizeof(Filt) == 64
    dt = _lib.HMMS_FILT_DTYPE
    assert dt.itemsize == 64
    assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(Filt, n).offset) for n, _ in Filt._fields_] \
        == [("loglik", 0), ("n_used", 8), ("flags", 12), ("post", 16)]
    assert dt["post"].shape == (6,)
    # loglik, n_used and flags lie where sk_hmm_post has them: the filter is the head of that record, then final_post
    for n, m in (("loglik", "loglik"), ("n_used", "n_used"), ("flags", "flags"), ("post", "final_post")):
        assert dt.fields[n] == _lib.HMM_POST_DTYPE.fields[m], n


def test_open_ex_refusals_come_from_the_arguments_alone():
    from squigglekit_amd import _lib, api
    L = _lib.load()
    INV = _lib.SK_ERR_INVALID
    h = C.c_int32(-7)
    good = api.polya_model("synth_raw")
    for flags in (2, 3, -1, 1 << 30, 0x100):                             # unknown bits, alone or beside the known one
        assert L.sk_hmms_open_ex(C.byref(good), 4, flags, C.byref(h)) == INV and "SK_HMMS_FILTER" in err(L), err(L)
        assert L.sk_hmms_open_ex(None, 0, flags, None) == INV and "flags" in err(L), err(L)     # ... decided first
    for flags in (0, 1):                                                 # then sk_hmms_open's refusals, in its words
        a = good.arrays()
        li = a["linit"].copy(); li[:] = -np.inf
        bad = _lib.HmmModel.from_arrays(6, li, a["ltrans"], a["c"], a["mu"], a["h"])
        assert L.sk_hmms_open_ex(C.byref(bad), 4, flags, C.byref(h)) == INV and "at least one linit must be finite" in err(L)
        assert L.sk_hmms_open_ex(None, 4, flags, C.byref(h)) == INV and "NULL sk_hmm_model" in err(L)
        assert L.sk_hmms_open_ex(C.byref(good), 4, flags, None) == INV and "NULL handle" in err(L)
        for nslots in (0, -3, 1048577):
            assert L.sk_hmms_open_ex(C.byref(good), nslots, flags, C.byref(h)) == INV and "nslots = %d" % nslots in err(L)
        if L.sk_device_count() <= 0:                                     # good arguments pass the checks and then need a device
            assert L.sk_hmms_open_ex(C.byref(good), 1048576, flags, C.byref(h)) == _lib.SK_ERR_NO_DEVICE, err(L)
    assert h.value == -7


def test_filter_refusals_come_from_the_arguments_alone():
    from squigglekit_amd import _lib
    L = _lib.load()
    INV = _lib.SK_ERR_INVALID
    i32 = lambda *v: np.array(v, dtype=np.int32)                        # noqa: E731
    q = lambda a: None if a is None else _lib.ptr(a)                    # noqa: E731
    out = np.full(64 * 3, 0xAB, dtype=np.uint8)
    for fn in (L.sk_hmms_filter, L.sk_hmms_filter_dev):
        for handle in (-1, 8, 99):
            assert fn(handle, q(i32(0)), 1, q(out)) == INV and "handle %d is outside [0, 8)" % handle in err(L)
        assert fn(0, q(i32(0)), -1, q(out)) == INV and "m < 0" in err(L)
        assert fn(0, None, 1, q(out)) == INV and "NULL slots" in err(L)
        assert fn(0, q(i32(0)), 1, None) == INV and "NULL out" in err(L)
    # what the host form can read: the slot numbers (a slot twice is allowed: the call only reads)
    for slots, words in ((i32(0, -1, 2), "entry 1: slot -1 is outside [0, 1048576)"),
                         (i32(1048576, 1, 2), "entry 0: slot 1048576 is outside [0, 1048576)")):
        assert L.sk_hmms_filter(0, q(slots), 3, q(out)) == INV and words in err(L), err(L)
    assert np.all(out == 0xAB)                                          # a refused call writes nothing
    # a handle inside the range is the session's to know (tests/test_gpu_hmmfilter.py pins those refusals); without a
    # device the call ends where the device is looked for -- also with a slot twice, and with m == 0 and NULL pointers
    if L.sk_device_count() <= 0:
        assert L.sk_hmms_filter(3, q(i32(5, 5, 5)), 3, q(out)) == _lib.SK_ERR_NO_DEVICE, err(L)
        assert L.sk_hmms_filter_dev(3, q(i32(5, 5, 5)), 3, q(out)) == _lib.SK_ERR_NO_DEVICE, err(L)
        assert L.sk_hmms_filter(3, None, 0, None) == _lib.SK_ERR_NO_DEVICE, err(L)
        assert np.all(out == 0xAB)
