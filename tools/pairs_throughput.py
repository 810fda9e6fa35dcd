#!/usr/bin/env python3
"""Throughput of DTW over a pair list (csrc/sk_pairs.hip, MODE_PAIRS / MODE_PAIRS_GLOBAL of csrc/sk_sdtw.hip): one JSON
line, also written to --out (profiles/pairs_throughput.json).  Recorded, not gated.

    python tools/pairs_throughput.py [--reads 200000] [--samples 4000] [--query 200] [--reps 5]
                                     [--map 3000,100000] [--target 100000] [--piece 8192] [--overlap 2048] [--out FILE]

degenerate   the list every other entry point could take: ONE query of --query points x --reads targets of --samples
             points, device resident (sk_dtw_pairs_dev over the float64 pA image of a seeded int16 batch), both modes,
             beside the exact single pass over the int16 rows as tools/hits_throughput.py times it (sk_motifseq_dev_i16
             under SK_DTW_SCHEME=full), alternated in the same run.  The step loop is the same code: `ratio_sweep` =
             pairs sweep time / exact sweep time (HIP events around the sweeps alone, sk_last_kernel_ms) is expected
             within run-to-run noise of 1 against the exact pass of the SAME feed, `ratio_sweep_f64` (sk_motifseq_dev_f64
             under SK_DTW_SCHEME=full over the same float64 values: float64 feeds keep the literal NaN-safe selects, two
             v_cndmask per double select, where the int16 feed's v_min_f64 does one); `ratio_wall` compares the calls
             (the exact call also filters and normalises, the pairs call also plans on the host).
mapping      --map queries of 300 .. 500 points against a --target-point reference and its reversal (api.map_queries, host
             form: the wall clock includes the upload), untiled and tiled at --piece / --overlap: cells per second."""
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
os.environ["SK_TUNING"] = "1"                   # (SK_DTW_SCHEME is a tuning switch)
from squigglekit_amd import _lib, api, synth     # noqa: E402


def main_ms(L):
    ms = C.c_float()
    _lib.check(L.sk_last_kernel_ms(None, C.byref(ms)))
    return float(ms.value) / 1e3


def summary(xs):
    return {"median_s": statistics.median(xs), "min_s": min(xs), "max_s": max(xs)}


def degenerate(L, R, M, N, reps):
    stride = (M + 7) // 8 * 8
    motif = synth.synthetic_motif(N)
    d_raw, d_len = L.sk_dev_alloc(R * stride * 2), L.sk_dev_alloc(R * 4)
    d_pool, d_off = L.sk_dev_alloc((R * M + N) * 8), L.sk_dev_alloc((R + 1) * 8)
    d_out = L.sk_dev_alloc(R * 24)
    _lib.check(L.sk_synth_squiggles_dev(C.c_void_p(d_raw), stride, R, M, 2025, _lib.ptr(motif), motif.size))
    _lib.check(L.sk_synth_pa_dev(C.c_void_p(d_raw), stride, R, M, 16.0, 1493.94, 8192.0, C.c_void_p(d_pool), C.c_void_p(d_off)))
    _lib.check(L.sk_dev_upload(C.c_void_p(d_pool + R * M * 8), _lib.ptr(motif), motif.nbytes))    # the query: sequence R
    lens = np.full(R, M, dtype=np.int32)
    _lib.check(L.sk_dev_upload(C.c_void_p(d_len), _lib.ptr(lens), lens.nbytes))
    _lib.check(L.sk_sync())
    off = np.concatenate([np.arange(R + 1, dtype=np.int64) * M, [R * M + N]]).astype(np.int64)
    pairs = np.zeros(R, dtype=api.PAIR_DTYPE)
    pairs["query"], pairs["target"] = R, np.arange(R)

    def run_pairs(mode):
        _lib.check(L.sk_dtw_pairs_dev(C.c_void_p(d_pool), _lib.ptr(off), R + 1, _lib.ptr(pairs), R, mode, C.c_void_p(d_out)))
        _lib.check(L.sk_sync())

    def run_full():
        os.environ["SK_DTW_SCHEME"] = "full"
        try:
            _lib.check(L.sk_motifseq_dev_i16(C.c_void_p(d_raw), stride, C.c_void_p(d_len), R, _lib.ptr(motif), motif.size,
                                             0, 0, 1200, C.c_void_p(d_out)))
            _lib.check(L.sk_sync())
        finally:
            os.environ.pop("SK_DTW_SCHEME", None)

    def run_full_f64():
        os.environ["SK_DTW_SCHEME"] = "full"
        try:
            _lib.check(L.sk_motifseq_dev_f64(C.c_void_p(d_pool), C.c_void_p(d_off), R, R * M, M, _lib.ptr(motif), motif.size,
                                             0, 0, 1200, C.c_void_p(d_out)))
            _lib.check(L.sk_sync())
        finally:
            os.environ.pop("SK_DTW_SCHEME", None)

    calls = {"pairs_subsequence": lambda: run_pairs(0), "pairs_global": lambda: run_pairs(1), "exact_full_i16": run_full,
             "exact_full_f64": run_full_f64}
    wall = {k: [] for k in calls}
    sweep = {k: [] for k in calls}
    for f in calls.values():                          # warm-up
        f()
    for _ in range(reps):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            wall[k].append(time.perf_counter() - t0)
            sweep[k].append(main_ms(L))
    for p in (d_raw, d_len, d_pool, d_off, d_out):
        L.sk_dev_free(C.c_void_p(p))
    cells = float(R) * M * N
    res = {"reads": R, "samples": M, "query": N, "cells": cells}
    for k in calls:
        res[k] = {"wall": summary(wall[k]), "sweep": summary(sweep[k]),
                  "cells_per_s_sweep": cells / statistics.median(sweep[k])}
    res["ratio_sweep"] = statistics.median(sweep["pairs_subsequence"]) / statistics.median(sweep["exact_full_i16"])
    res["ratio_sweep_f64"] = statistics.median(sweep["pairs_subsequence"]) / statistics.median(sweep["exact_full_f64"])
    res["ratio_wall"] = statistics.median(wall["pairs_subsequence"]) / statistics.median(wall["exact_full_i16"])
    return res


def mapping(L, Q, T, piece, overlap, reps):
    rng = np.random.default_rng(5)
    ref = rng.normal(size=T)
    targets = [ref, np.ascontiguousarray(ref[::-1])]
    lens = rng.integers(300, 501, size=Q)
    queries = [rng.normal(size=int(n)) for n in lens]
    res = {"queries": Q, "target": T, "query_points": int(lens.sum())}
    pieces, tiling = api.tile_targets(targets, piece, overlap)
    for name, ys in (("untiled", targets), ("tiled", pieces)):
        cells = float(lens.sum()) * float(sum(len(y) for y in ys))
        wall, sweep = [], []
        api.map_queries(queries[:8], ys)              # warm-up: a few pairs through the same kernels
        for _ in range(reps):
            t0 = time.perf_counter()
            rec, _ = api.map_queries(queries, ys)
            wall.append(time.perf_counter() - t0)
            sweep.append(main_ms(L))
        if name == "tiled":
            t0 = time.perf_counter()
            api.merge_tiles(rec, tiling)
            res["merge_tiles_s"] = time.perf_counter() - t0
        res[name] = {"targets": len(ys), "pairs": Q * len(ys), "cells": cells, "wall": summary(wall),
                     "sweep": summary(sweep), "cells_per_s_sweep": cells / statistics.median(sweep),
                     "cells_per_s_wall": cells / statistics.median(wall)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200000)
    ap.add_argument("--samples", type=int, default=4000)
    ap.add_argument("--query", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--map", default="3000,100000", help="query counts of the mapping shape (comma list; empty: none)")
    ap.add_argument("--map_reps", type=int, default=1)
    ap.add_argument("--target", type=int, default=100000)
    ap.add_argument("--piece", type=int, default=8192)
    ap.add_argument("--overlap", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.ensure_init()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernels_sha import kernels_sha
    res = {"tool": "pairs_throughput", "kernels_sha": kernels_sha(ROOT), "piece": a.piece, "overlap": a.overlap}
    if a.reads > 0:
        res["degenerate"] = degenerate(L, a.reads, a.samples, a.query, a.reps)
    res["mapping"] = [mapping(L, int(q), a.target, a.piece, a.overlap, a.map_reps) for q in a.map.split(",") if q]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
