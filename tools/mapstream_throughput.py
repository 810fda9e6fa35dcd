#!/usr/bin/env python3
"""Throughput of a mapping session (csrc/sk_mapstream.hip, MODE_PAIRS_CHAIN of csrc/sk_sdtw.hip): one JSON line, also
written to --out (profiles/mapstream_throughput.json).  Recorded, not gated.

    python tools/mapstream_throughput.py [--slots 512] [--chunk 50] [--pushes 10] [--reads 3] [--target 100000]
                                         [--piece 8192] [--overlap 2048] [--out FILE]

The selective-sequencing shape: --slots channels, every one pushed --chunk points at a time, --pushes pushes per read,
against a --target-point reference and its reversal -- untiled, and tiled at --piece / --overlap.  Device resident on
both sides (sk_map_push_dev; sk_dtw_pairs_dev), wall clock around call + synchronisation.

per_push_ms   one push of all slots: median, min and max over the pushes of --reads reads after a warm-up read; and by
              push index (the first push of a read is fresh, the others continue: the same sweep, the stored row read too)
read_ms       the --pushes pushes of a read, summed (median over the reads)
one_shot_ms   ONE sk_dtw_pairs_dev call on the same slots x (chunk x pushes)-point queries and the same targets, in the
              same run -- code the session does not share beyond k_sdtw's cell loop; a session pays --pushes sweeps of the
              whole target where the one-shot call pays one, so read_ms / one_shot_ms is the price of having a record
              after every chunk
plan          sk_last_map_plan() after the last push: bytes of row state, entries, launches"""
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
os.environ["SK_TUNING"] = "1"
from squigglekit_amd import _lib, api     # noqa: E402


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def shape(L, name, ys, S, E, P, reads, rng):
    T, N = len(ys), E * P
    queries = rng.normal(size=(reads + 1, S, N))                        # read 0 is the warm-up
    d_vals, d_slots = L.sk_dev_alloc(S * N * 8), L.sk_dev_alloc(S * 4)
    d_rec = L.sk_dev_alloc(T * S * 32)
    slots = np.arange(S, dtype=np.int32)
    _lib.check(L.sk_dev_upload(C.c_void_p(d_slots), _lib.ptr(slots), slots.nbytes))
    off = np.arange(S + 1, dtype=np.int64) * E
    per_push, by_index, per_read = [], [[] for _ in range(P)], []
    with api.MapStream(ys, S) as ms:
        for r in range(reads + 1):
            ms.reset(slots)
            total = 0.0
            for p in range(P):
                chunk = np.ascontiguousarray(queries[r, :, p * E:(p + 1) * E])
                _lib.check(L.sk_dev_upload(C.c_void_p(d_vals), _lib.ptr(chunk), chunk.nbytes))
                _lib.check(L.sk_sync())
                t0 = time.perf_counter()
                _lib.check(L.sk_map_push_dev(ms.handle, C.c_void_p(d_slots), S, C.c_void_p(d_vals), _lib.ptr(off), C.c_void_p(d_rec)))
                _lib.check(L.sk_sync())
                dt = (time.perf_counter() - t0) * 1e3
                total += dt
                if r > 0:
                    per_push.append(dt)
                    by_index[p].append(dt)
            if r > 0:
                per_read.append(total)
        plan = api.last_map_plan()
        last = np.zeros((T, S), dtype=api.MAPREC_DTYPE)
        _lib.check(L.sk_dev_download(_lib.ptr(last), C.c_void_p(d_rec), last.nbytes))
    # the one-shot call on the last read's whole queries: the pool is the queries, then the targets
    pool = np.concatenate([queries[reads].reshape(-1)] + [np.asarray(y, dtype=np.float64) for y in ys])
    poff = np.concatenate([np.arange(S, dtype=np.int64) * N, S * N + np.concatenate([[0], np.cumsum([len(y) for y in ys])])])
    t, q = np.divmod(np.arange(T * S, dtype=np.int64), S)
    pairs = np.zeros(T * S, dtype=api.PAIR_DTYPE)
    pairs["query"], pairs["target"] = q, S + t
    d_pool, d_hit = L.sk_dev_alloc(pool.nbytes), L.sk_dev_alloc(T * S * 24)
    _lib.check(L.sk_dev_upload(C.c_void_p(d_pool), _lib.ptr(pool), pool.nbytes))
    one = []
    for k in range(reads + 1):
        _lib.check(L.sk_sync())
        t0 = time.perf_counter()
        _lib.check(L.sk_dtw_pairs_dev(C.c_void_p(d_pool), _lib.ptr(poff), S + T, _lib.ptr(pairs), T * S, 0, C.c_void_p(d_hit)))
        _lib.check(L.sk_sync())
        if k > 0:
            one.append((time.perf_counter() - t0) * 1e3)
    hits = np.zeros((T, S), dtype=api.HIT_DTYPE)
    _lib.check(L.sk_dev_download(_lib.ptr(hits), C.c_void_p(d_hit), hits.nbytes))
    for p in (d_vals, d_slots, d_rec, d_pool, d_hit):
        L.sk_dev_free(C.c_void_p(p))
    cells_push = float(S) * E * float(sum(len(y) for y in ys))
    return {"shape": name, "targets": T, "target_points": int(sum(len(y) for y in ys)), "lane_groups": T * S,
            "per_push_ms": spread(per_push), "per_push_ms_by_index": [statistics.median(v) for v in by_index],
            "read_ms": spread(per_read), "one_shot_ms": spread(one),
            "read_over_one_shot": statistics.median(per_read) / statistics.median(one),
            "cells_per_s_push": cells_push / (statistics.median(per_push) / 1e3),
            "cells_per_s_one_shot": cells_push * P / (statistics.median(one) / 1e3),
            "same_records_as_one_shot": bool(api.map_hits(last).tobytes() == hits.tobytes()), "plan": plan}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=512)
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--pushes", type=int, default=10)
    ap.add_argument("--reads", type=int, default=3)
    ap.add_argument("--target", type=int, default=100000)
    ap.add_argument("--piece", type=int, default=8192)
    ap.add_argument("--overlap", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.ensure_init()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernels_sha import kernels_sha
    rng = np.random.default_rng(5)
    ref = rng.normal(size=a.target)
    targets = [ref, np.ascontiguousarray(ref[::-1])]
    pieces, _ = api.tile_targets(targets, a.piece, a.overlap)
    res = {"tool": "mapstream_throughput", "kernels_sha": kernels_sha(ROOT), "note": "one run on one MI355X",
           "slots": a.slots, "chunk": a.chunk, "pushes": a.pushes, "reads": a.reads, "target": a.target, "piece": a.piece,
           "overlap": a.overlap,
           "shapes": [shape(L, name, ys, a.slots, a.chunk, a.pushes, a.reads, rng)
                      for name, ys in (("untiled", targets), ("tiled", pieces))]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
