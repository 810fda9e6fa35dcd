"""CPU: the C ABI of the adaptive-band DTW -- the header declares its three entries, the built library exports them, and
every refusal is made from the arguments alone, before a device is looked for: the same codes and messages on any
machine, and the ones sk_dtw_pairs gives where the two share a rule.  No compute calls here."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT

ENTRIES = ("sk_dtw_band", "sk_dtw_band_dev", "sk_last_band_plan")
PAIR = np.dtype([("query", "<i4"), ("target", "<i4")])


def test_header_declares_and_library_exports_the_entries():
    from squigglekit_amd import _lib
    text = open(os.path.join(ROOT, "include", "squigglekit_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.ABI
    assert re.search(r"SK_BAND_PINNED\s*=\s*0\s*,\s*SK_BAND_FREE\s*=\s*1", code)
    assert re.search(r"SK_FLAG_BAND_LOST\s*=\s*16", code)
    assert (_lib.SK_BAND_PINNED, _lib.SK_BAND_FREE, _lib.SK_FLAG_BAND_LOST) == (0, 1, 16)
    _lib.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert _lib.tunables()["SK_BAND_WAVES"][0] == "1"               # the one switch of the kernel, in the one table


def call(L, fn, values, off, pairs, band, end, rec, spans):
    from squigglekit_amd import _lib
    pr = np.zeros(len(pairs), dtype=PAIR)
    if len(pairs):
        pr["query"], pr["target"] = zip(*pairs)
    rc = getattr(L, fn)(_lib.ptr(values), None if off is None else _lib.ptr(off), 0 if off is None else off.size - 1,
                        _lib.ptr(pr), len(pr), band, end, None if rec is None else _lib.ptr(rec),
                        None if spans is None else _lib.ptr(spans))
    return rc, L.sk_last_error().decode()


def test_refusals_come_from_the_arguments_alone():
    from squigglekit_amd import _lib
    L = _lib.load()
    lens = [30, 0, 2 ** 20 + 1, 50, 2 ** 20]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    values = np.zeros(64)                                           # never followed: every call below is refused first
    INV, UNS = _lib.SK_ERR_INVALID, _lib.SK_ERR_UNSUPPORTED
    for fn in ("sk_dtw_band", "sk_dtw_band_dev"):
        for pairs, band, end, code, words in (
                ([(0, 3)], 100, 0, INV, ("band width 100", "64, 128 or 256")),
                ([(0, 3)], 0, 0, INV, ("band width 0",)),
                ([(0, 3)], 512, 1, INV, ("band width 512",)),
                ([(0, 3)], 128, 2, INV, ("end mode 2",)),
                ([(0, 3)], 128, -1, INV, ("end mode -1",)),
                ([(0, 3), (1, 3)], 64, 0, INV, ("pair 1", "empty query", "sequence 1")),
                ([(0, 5)], 64, 1, INV, ("pair 0", "target index 5 outside [0, 5)")),
                ([(0, 3), (0, 3), (-1, 0)], 256, 0, INV, ("pair 2", "query index -1 outside [0, 5)")),
                ([(3, 0), (2, 3)], 128, 0, UNS, ("pair 1", "query of 1048577 points", "sequence 2", "at most 1048576")),
                ([(3, 2)], 128, 1, UNS, ("pair 0", "target of 1048577 points", "at most 1048576"))):
            rec = np.full(len(pairs) * 24, 0xAB, dtype=np.uint8)
            sp = np.full(4096, 0xAB, dtype=np.uint8)
            rc, msg = call(L, fn, values, off, pairs, band, end, rec, sp)
            assert rc == code and all(w in msg for w in words), (fn, pairs, band, end, rc, msg)
            assert np.all(rec == 0xAB) and np.all(sp == 0xAB), (fn, pairs)      # nothing was written
        rec = np.full(24, 0xAB, dtype=np.uint8)
        rc, msg = call(L, fn, values, off, [(0, 3)], 128, 0, None, None)        # NULL records
        assert rc == INV and "NULL off/pairs/out" in msg
        rc, msg = call(L, fn, values, None, [(0, 3)], 128, 0, rec, None)        # NULL off
        assert rc == INV and "NULL off/pairs/out" in msg
        pr = np.zeros(1, dtype=PAIR)
        f = getattr(L, fn)
        assert f(_lib.ptr(values), _lib.ptr(off), 5, _lib.ptr(pr), 2 ** 27 + 1, 128, 0, _lib.ptr(rec), None) == UNS
        assert "134217728" in L.sk_last_error().decode()
        assert f(_lib.ptr(values), _lib.ptr(off), 5, _lib.ptr(pr), -1, 128, 0, _lib.ptr(rec), None) == INV
        assert np.all(rec == 0xAB)
    # 2^20 points on either side is inside the limit: such a list passes the checks (and then needs a device)
    rec = np.full(24, 0xAB, dtype=np.uint8)
    rc, msg = call(L, "sk_dtw_band_dev", values, off, [(4, 4)], 64, 0, rec, None)
    if L.sk_device_count() <= 0:
        assert rc == _lib.SK_ERR_NO_DEVICE, (rc, msg)
    # the shared rules read as sk_dtw_pairs reads them
    src = open(os.path.join(ROOT, "squigglekit_amd", "csrc", "sk_pairs.hip")).read()
    for text in ('"pair %lld: empty query (sequence %d)"', '"pair %lld: query index %d outside [0, %d)"',
                 '"pair %lld: target index %d outside [0, %d)"', '"NULL off/pairs/out"', '"npairs %lld above 134217728"'):
        assert text in src and text in open(os.path.join(ROOT, "squigglekit_amd", "csrc", "sk_band.hip")).read(), text
