#!/usr/bin/env python3
"""Throughput of the hit lists over a pair list and from a mapping session's rows (csrc/sk_pairhits.hip): one JSON line,
also written to --out (profiles/pair_hits_throughput.json).  Recorded, not gated.

    python tools/pair_hits_throughput.py [--scale 1.0] [--out FILE]

Device resident on both sides.  Times are HIP events around the launches of a call (sk_last_kernel_ms: the library
records them on its own stream), medians of 5 after one warm-up call; the push of run (c), which records no events, is
wall clock around call + synchronisation, and so is the `wall_ms` beside every event figure.

(a) many short rows   200 000 targets x 4 000 points x one 200-point query, K = 1 and 8, against sk_dtw_pairs_dev on the
                      same list in the same run.  The rows (9.6 GB) pass the 2 GiB row buffer slice after slice.
(b) few long rows     3 000 queries of 300 - 500 points against a 100 000-point reference and its reversal, K = 2 and 8,
                      against sk_dtw_pairs_dev; the slices, and `over_pairs_share` = 1 - pairs_ms / hits_ms: what the
                      select AND the stores of the last rows add to the sweep (an upper bound of the select's share).
                      Then the same list with SK_HITS_ROW_BYTES = 8 GiB, one slice: what the slicing itself costs (a
                      sweep over 100 000 columns is one long serial walk per wavefront, and a slice of a quarter of the
                      pairs takes nearly as long as the whole list).
(c) a session         512 slots against the same two targets: sk_map_hits_dev at K = 2 and 8 beside one push of 50 points
                      in the same run -- with the long tier (a workgroup of 16 wavefronts per row) and with the rows
                      forced through one wavefront each (SK_ROWHITS_ONE_WAVE=1): the A/B that justifies the tier.
--scale shrinks the counts (targets of (a), queries of (b), slots of (c)) for a quick look."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["SK_TUNING"] = "1"                   # (SK_ROWHITS_ONE_WAVE is a tuning switch)
from squigglekit_amd import _lib, api     # noqa: E402

REPS = 5


def timed(L, call):
    """medians over REPS calls after a warm-up: (event ms of the call's launches, wall ms of call + sync)"""
    ev, wall = [], []
    a, b = C.c_float(), C.c_float()
    for k in range(REPS + 1):
        _lib.check(L.sk_sync())
        t0 = time.perf_counter()
        _lib.check(call())
        _lib.check(L.sk_sync())
        dt = (time.perf_counter() - t0) * 1e3
        _lib.check(L.sk_last_kernel_ms(C.byref(a), C.byref(b)))
        if k:
            ev.append(float(b.value))
            wall.append(dt)
    return {"event_ms": statistics.median(ev), "wall_ms": statistics.median(wall), "n": REPS}


def wall_only(L, call, before=None):
    out = []
    for k in range(REPS + 1):
        if before:
            before()
        _lib.check(L.sk_sync())
        t0 = time.perf_counter()
        _lib.check(call())
        _lib.check(L.sk_sync())
        if k:
            out.append((time.perf_counter() - t0) * 1e3)
    return {"wall_ms": statistics.median(out), "n": REPS}


def upload(L, a):
    p = L.sk_dev_alloc(max(a.nbytes, 8))
    assert p, L.sk_last_error()
    _lib.check(L.sk_dev_upload(C.c_void_p(p), _lib.ptr(a), a.nbytes))
    return p


def pair_list(L, values, off, pairs, Ks):
    """sk_dtw_pairs_dev and sk_dtw_pairs_hits_dev at every K on one list over the pool (values, off)"""
    pr = api._as_pairs(pairs)
    n = len(pr)
    d_val, d_rec = upload(L, values), L.sk_dev_alloc(n * 24)
    d_out, d_cnt = L.sk_dev_alloc(n * max(Ks) * 24), L.sk_dev_alloc(n * 4)
    res = {"pairs": n, "columns": int(sum(int(off[t + 1] - off[t]) for t in pr["target"]))}
    res["dtw_pairs"] = timed(L, lambda: L.sk_dtw_pairs_dev(C.c_void_p(d_val), _lib.ptr(off), off.size - 1, _lib.ptr(pr), n, 0,
                                                           C.c_void_p(d_rec)))
    for K in Ks:
        r = timed(L, lambda: L.sk_dtw_pairs_hits_dev(C.c_void_p(d_val), _lib.ptr(off), off.size - 1, _lib.ptr(pr), n, K,
                                                     float("inf"), C.c_void_p(d_out), C.c_void_p(d_cnt)))
        r["plan"] = api.last_pair_hits_plan()
        r["over_pairs_share"] = 1.0 - res["dtw_pairs"]["event_ms"] / r["event_ms"]
        res["hits_K%d" % K] = r
    first = np.zeros(n * max(Ks), dtype=api.HIT_DTYPE)
    rec = np.zeros(n, dtype=api.HIT_DTYPE)
    _lib.check(L.sk_dev_download(_lib.ptr(first), C.c_void_p(d_out), n * Ks[-1] * 24))
    _lib.check(L.sk_dev_download(_lib.ptr(rec), C.c_void_p(d_rec), rec.nbytes))
    res["hit1_is_dtw_pairs"] = bool(first[:n * Ks[-1]].reshape(n, Ks[-1])[:, 0].tobytes() == rec.tobytes())
    for p in (d_val, d_rec, d_out, d_cnt):
        L.sk_dev_free(C.c_void_p(p))
    return res


def session(L, ys, S, Ks, rng):
    T = len(ys)
    slots = np.arange(S, dtype=np.int32)
    d_slots = upload(L, slots)
    chunk = rng.normal(size=S * 50)
    d_vals = upload(L, chunk)
    d_rec = L.sk_dev_alloc(T * S * 32)
    d_out, d_cnt = L.sk_dev_alloc(T * S * max(Ks) * 24), L.sk_dev_alloc(T * S * 4)
    off = np.arange(S + 1, dtype=np.int64) * 50
    res = {"slots": S, "targets": [len(y) for y in ys]}
    with api.MapStream(ys, S) as ms:
        push = lambda: L.sk_map_push_dev(ms.handle, C.c_void_p(d_slots), S, C.c_void_p(d_vals), _lib.ptr(off), C.c_void_p(d_rec))   # noqa: E731
        _lib.check(push())
        res["push_50"] = wall_only(L, push)
        for tier, env in (("long_tier", None), ("one_wave", "1")):
            if env:
                os.environ["SK_ROWHITS_ONE_WAVE"] = env
            for K in Ks:
                r = timed(L, lambda: L.sk_map_hits_dev(ms.handle, C.c_void_p(d_slots), S, K, float("inf"), C.c_void_p(d_out),
                                                       C.c_void_p(d_cnt)))
                r["plan"] = api.last_pair_hits_plan()
                r["of_a_push"] = r["wall_ms"] / res["push_50"]["wall_ms"]
                res["%s_K%d" % (tier, K)] = r
            os.environ.pop("SK_ROWHITS_ONE_WAVE", None)
    for p in (d_slots, d_vals, d_rec, d_out, d_cnt):
        L.sk_dev_free(C.c_void_p(p))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_hits_throughput.json"))
    args = ap.parse_args()
    L = _lib.ensure_init()
    rng = np.random.default_rng(1)
    res = {"scale": args.scale}
    # (a)
    nt = max(64, int(200000 * args.scale))
    values = rng.standard_normal(200 + nt * 4000)
    off = np.concatenate([[0], 200 + 4000 * np.arange(nt + 1, dtype=np.int64)])
    res["a_short_rows"] = pair_list(L, values, off, np.stack([np.zeros(nt, dtype=np.int64), 1 + np.arange(nt)], axis=1), (1, 8))
    del values
    # (b)
    ref = rng.normal(size=100000)
    ys = [ref, np.ascontiguousarray(ref[::-1])]
    nq = max(8, int(3000 * args.scale))
    qs = [rng.normal(size=int(n)) for n in rng.integers(300, 501, size=nq)]
    t, q = np.divmod(np.arange(2 * nq), nq)
    values, off = api._as_pool(qs + ys)
    res["b_long_rows"] = pair_list(L, values, off, np.stack([q, nq + t], axis=1), (2, 8))
    os.environ["SK_HITS_ROW_BYTES"] = str(8 << 30)              # the same list in ONE slice: what the slicing costs
    res["b_long_rows_one_slice"] = pair_list(L, values, off, np.stack([q, nq + t], axis=1), (2,))
    os.environ.pop("SK_HITS_ROW_BYTES")
    # (c)
    res["c_session"] = session(L, ys, max(4, int(512 * args.scale)), (2, 8), rng)
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
