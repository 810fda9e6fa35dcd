"""CPU: the C ABI of the hit lists over a pair list -- the header declares its five entries, the built library exports
them, and every refusal the arguments alone decide is made before a device is looked for: the same codes and messages on
any machine.  No compute calls here."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT

ENTRIES = ("sk_dtw_pairs_hits", "sk_dtw_pairs_hits_dev", "sk_map_hits", "sk_map_hits_dev", "sk_last_pair_hits_plan")
PAIR = np.dtype([("query", "<i4"), ("target", "<i4")])
INF = float("inf")


def test_header_declares_and_library_exports_the_entries():
    from squigglekit_amd import _lib
    text = open(os.path.join(ROOT, "include", "squigglekit_hip.h")).read()
    assert "Hit lists over a pair list" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.ABI
    _lib.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert "SK_ROWHITS_ONE_WAVE" in _lib.tunables() and "SK_HITS_ROW_BYTES" in _lib.tunables()


def call(L, fn, values, off, pairs, K, max_dist, out, count, npairs=None):
    from squigglekit_amd import _lib
    pr = np.zeros(max(1, len(pairs)), dtype=PAIR)
    if len(pairs):
        pr["query"][:len(pairs)], pr["target"][:len(pairs)] = zip(*pairs)
    rc = getattr(L, fn)(_lib.ptr(values), None if off is None else _lib.ptr(off), 0 if off is None else off.size - 1,
                        _lib.ptr(pr), len(pairs) if npairs is None else npairs, K, max_dist,
                        None if out is None else _lib.ptr(out), None if count is None else _lib.ptr(count))
    return rc, L.sk_last_error().decode()


def test_pair_list_refusals_come_from_the_arguments_alone():
    from squigglekit_amd import _lib
    L = _lib.load()
    lens = [30, 0, 1025, 50, 1024]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    values = np.zeros(64)                                           # never followed: every call below is refused first
    INV, UNS = _lib.SK_ERR_INVALID, _lib.SK_ERR_UNSUPPORTED
    for fn in ("sk_dtw_pairs_hits", "sk_dtw_pairs_hits_dev"):
        for pairs, K, md, code, words in (
                ([(0, 3)], 0, INF, INV, ("max_hits 0 outside 1..64",)),
                ([(0, 3)], 65, INF, INV, ("max_hits 65 outside 1..64",)),
                ([(0, 3)], -1, 1.0, INV, ("max_hits -1",)),
                ([(0, 3)], 8, float("nan"), INV, ("max_dist is NaN",)),
                ([(0, 5)], 8, INF, INV, ("pair 0", "target index 5 outside [0, 5)")),
                ([(0, 3), (0, 3), (-1, 0)], 8, INF, INV, ("pair 2", "query index -1 outside [0, 5)")),
                ([(0, 3), (1, 3)], 2, 1.0, INV, ("pair 1", "empty query", "sequence 1")),
                ([(3, 0), (2, 3)], 2, INF, UNS, ("pair 1", "query of 1025 points", "sequence 2", "at most 1024"))):
            out = np.full(len(pairs) * 64 * 24, 0xAB, dtype=np.uint8)
            cnt = np.full(len(pairs) * 4, 0xAB, dtype=np.uint8)
            rc, msg = call(L, fn, values, off, pairs, K, md, out, cnt)
            assert rc == code and all(w in msg for w in words), (fn, pairs, K, md, rc, msg)
            assert np.all(out == 0xAB) and np.all(cnt == 0xAB), (fn, pairs)      # nothing was written
        out = np.full(64 * 24, 0xAB, dtype=np.uint8)
        cnt = np.full(4, 0xAB, dtype=np.uint8)
        for o, c in ((None, cnt), (out, None), (None, None)):
            rc, msg = call(L, fn, values, off, [(0, 3)], 8, INF, o, c)
            assert rc == INV and "NULL out/count" in msg, (fn, rc, msg)
        rc, msg = call(L, fn, values, None, [(0, 3)], 8, INF, out, cnt)
        assert rc == INV and "NULL off/pairs/out" in msg
        assert call(L, fn, values, off, [], 8, INF, out, cnt, npairs=-1)[0] == INV
        rc, msg = call(L, fn, values, off, [], 8, INF, out, cnt, npairs=2 ** 27 + 1)
        assert rc == UNS and "134217728" in msg
        # an empty list is no work and no error, with or without buffers, on any machine
        assert call(L, fn, values, off, [], 8, INF, out, cnt)[0] == 0
        assert call(L, fn, values, off, [], 1, 0.0, None, None)[0] == 0
        assert np.all(out == 0xAB) and np.all(cnt == 0xAB)
    # a query of 1 024 points is inside the limit: such a list passes the checks (and then needs a device)
    out = np.full(24, 0xAB, dtype=np.uint8)
    cnt = np.full(4, 0xAB, dtype=np.uint8)
    rc, msg = call(L, "sk_dtw_pairs_hits_dev", values, off, [(4, 3)], 1, INF, out, cnt)
    if L.sk_device_count() <= 0:
        assert rc == _lib.SK_ERR_NO_DEVICE, (rc, msg)


def test_session_refusals_come_from_the_arguments_alone():
    from squigglekit_amd import _lib
    L = _lib.load()
    INV = _lib.SK_ERR_INVALID
    out = np.full(4 * 64 * 24, 0xAB, dtype=np.uint8)
    cnt = np.full(16, 0xAB, dtype=np.uint8)
    slots = np.array([0, 1], dtype=np.int32)
    for fn in ("sk_map_hits", "sk_map_hits_dev"):
        f = getattr(L, fn)
        for handle, sl, m, K, md, o, c, words in (
                (-1, slots, 2, 2, INF, out, cnt, ("handle -1 is outside",)),
                (_lib.SK_MAP_MAX_SESSIONS, slots, 2, 2, INF, out, cnt, ("handle %d is outside" % _lib.SK_MAP_MAX_SESSIONS,)),
                (0, slots, -1, 2, INF, out, cnt, ("m < 0",)),
                (0, slots, 2, 0, INF, out, cnt, ("max_hits 0 outside 1..64",)),
                (0, slots, 2, 65, INF, out, cnt, ("max_hits 65 outside 1..64",)),
                (0, slots, 2, 2, float("nan"), out, cnt, ("max_dist is NaN",)),
                (0, None, 2, 2, INF, out, cnt, ("NULL slots/out/count",)),
                (0, slots, 2, 2, INF, None, cnt, ("NULL slots/out/count",)),
                (0, slots, 2, 2, INF, out, None, ("NULL slots/out/count",))):
            rc = f(handle, None if sl is None else _lib.ptr(sl), m, K, md, None if o is None else _lib.ptr(o),
                   None if c is None else _lib.ptr(c))
            msg = L.sk_last_error().decode()
            assert rc == INV and all(w in msg for w in words), (fn, handle, m, K, rc, msg)
            assert np.all(out == 0xAB) and np.all(cnt == 0xAB)
    for bad, words in ((np.array([0, -1], dtype=np.int32), ("entry 1", "slot -1 is outside")),
                       (np.array([0, _lib.SK_MAP_MAX_SLOTS], dtype=np.int32), ("entry 1", "is outside")),
                       (np.array([3, 3], dtype=np.int32), ("entry 1", "slot 3 appears twice"))):
        rc = L.sk_map_hits(0, _lib.ptr(bad), 2, 2, INF, _lib.ptr(out), _lib.ptr(cnt))
        msg = L.sk_last_error().decode()
        assert rc == INV and all(w in msg for w in words), (bad, rc, msg)
    assert np.all(out == 0xAB) and np.all(cnt == 0xAB)
