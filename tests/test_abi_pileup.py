"""The reference pile-up in the C ABI: the record's layout, the symbols in the header and in the ctypes table, the tuning
switch in the one table.  The refusals need a device (an entry point looks for its context first): they are in
tests/test_gpu_pileup.py, but for the one that is checked here, marked gpu."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

FIELDS = (("level", 0, 8), ("level_sd", 8, 8), ("vmin", 16, 8), ("vmax", 24, 8), ("dwell_mean", 32, 8), ("dwell_sd", 40, 8),
          ("depth", 48, 4), ("n", 52, 4), ("shared", 56, 4), ("pad", 60, 4))


def test_record_layout():
    from squigglekit_amd import _lib, api
    assert C.sizeof(_lib.PileRec) == 64 and _lib.PILE_DTYPE.itemsize == 64 and api.PILE_DTYPE is _lib.PILE_DTYPE
    for name, off, size in FIELDS:
        f = getattr(_lib.PileRec, name)
        assert (f.offset, f.size) == (off, size), name
        assert _lib.PILE_DTYPE.fields[name][1] == off and _lib.PILE_DTYPE.fields[name][0].itemsize == size, name
    assert [n for n, _ in _lib.PileRec._fields_] == [n for n, _, _ in FIELDS] == list(_lib.PILE_DTYPE.names)
    header = open(os.path.join(ROOT, "include", "squigglekit_hip.h")).read()
    m = re.search(r"typedef struct sk_pile_rec \{[^\n]*\n(.*?)\} sk_pile_rec;", header, flags=re.S)
    assert m and "64 bytes" in header[m.start():m.end()]
    names = re.findall(r"\b([a-z_]+)\s*[,;]", re.sub(r"\b(double|int32_t)\b", "", m.group(1)))
    assert names == [n for n, _, _ in FIELDS]


def test_symbols_in_header_table_and_library():
    from squigglekit_amd import _lib
    header = open(os.path.join(ROOT, "include", "squigglekit_hip.h")).read()
    L = _lib.load()
    for name, nargs in (("sk_pileup", 15), ("sk_pileup_dev", 15), ("sk_last_pileup_plan", 4)):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.ABI and len(_lib.ABI[name][1]) == nargs and _lib.ABI[name][0] is C.c_int, name
        assert hasattr(L, name)
    assert "Reference pile-up" in header and "tests/pileup_ref.py" in header
    table = open(os.path.join(ROOT, "squigglekit_amd", "csrc", "sk_runtime.hip")).read()
    assert '{"SK_PILE_LDS_ENTRIES",' in table
    src = open(os.path.join(ROOT, "squigglekit_amd", "csrc", "sk_pileup.hip")).read()
    assert 'sk_tune("SK_PILE_LDS_ENTRIES")' in src and "sk_pileup.hip" in open(os.path.join(ROOT, "squigglekit_amd", "csrc", "Makefile")).read()


def test_without_a_device_the_call_says_so():
    from squigglekit_amd import _lib
    L = _lib.load()
    if L.sk_device_count() > 0:
        pytest.skip("a GPU is visible here")
    one = np.zeros(1, dtype=np.int64)
    rc = L.sk_pileup(_lib.ptr(one), None, None, None, None, None, None, 0, 0, _lib.ptr(one), 0, None, None, None, 0)
    assert rc == _lib.SK_ERR_NO_DEVICE


@pytest.mark.gpu
def test_refusals_by_the_arguments_alone(gpu):
    """SK_ERR_INVALID for what the arguments alone decide, SK_ERR_UNSUPPORTED beyond the limits: nothing is launched"""
    L = gpu.load()
    so, sp, v, tl = np.zeros(2, dtype=np.int64), np.zeros((1, 2), dtype=np.int32), np.zeros(1), np.array([4], dtype=np.int64)
    so[1] = 1
    out = np.full(4 * 64, 0xAB, dtype=np.uint8)
    eo = np.zeros(5, dtype=np.int64)
    p = gpu.ptr

    def call(span_off=p(so), spans=p(sp), value=p(v), npairs=1, nrows=1, tlen=p(tl), nt=1, o=p(out), ent_off=None,
             ent_row=None, cap=0):
        rc = L.sk_pileup(span_off, spans, value, None, None, None, None, npairs, nrows, tlen, nt, o, ent_off, ent_row, cap)
        return rc, L.sk_last_error().decode()
    for kw, code, word in ((dict(npairs=-1), gpu.SK_ERR_INVALID, "negative"), (dict(nrows=-1), gpu.SK_ERR_INVALID, "negative"),
                           (dict(nt=-1), gpu.SK_ERR_INVALID, "negative"), (dict(span_off=None), gpu.SK_ERR_INVALID, "NULL"),
                           (dict(tlen=None), gpu.SK_ERR_INVALID, "NULL"), (dict(spans=None), gpu.SK_ERR_INVALID, "NULL"),
                           (dict(value=None), gpu.SK_ERR_INVALID, "NULL"), (dict(o=None), gpu.SK_ERR_INVALID, "NULL out"),
                           (dict(ent_off=p(eo)), gpu.SK_ERR_INVALID, "go together"),
                           (dict(ent_off=p(eo), ent_row=p(sp), cap=-1), gpu.SK_ERR_INVALID, "ent_cap"),
                           (dict(nrows=2 ** 31), gpu.SK_ERR_UNSUPPORTED, "2^31 - 1 rows"),
                           (dict(tlen=p(np.array([2 ** 40 + 1], dtype=np.int64))), gpu.SK_ERR_UNSUPPORTED, "2^40")):
        rc, msg = call(**kw)
        assert rc == code and word in msg, (kw.keys(), rc, msg)
        assert np.all(out == 0xAB)
    rc, msg = call()
    assert rc == 0, msg
    assert np.frombuffer(out.tobytes(), dtype=gpu.PILE_DTYPE)["n"].tolist() == [1, 0, 0, 0]
