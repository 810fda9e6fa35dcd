#!/usr/bin/env python3
"""Throughput of the warping paths over a pair list (csrc/sk_pairpath.hip) against the records-only call in the same run:
one JSON line, also written to --out (profiles/pair_paths_throughput.json).  Recorded, not gated.

    python tools/pair_paths_throughput.py [--reads 200000] [--samples 4000] [--query 200] [--reps 5]
                                          [--map 100000] [--target 100000] [--out FILE]

degenerate   ONE query of --query points x --reads targets of --samples points, device resident (the float64 pA image of
             a seeded int16 batch; the query is the batch's motif in the same pA units, so that a match spans about as
             many columns as the query has points -- a z-scored query against pA values matches one column):
             sk_dtw_pairs_dev (the records) against sk_dtw_pairs_paths_dev (records, then paths), alternated; then the paths alone from the
             records of that call (have_records = 1), as is and with every pair forced into the scratch tier
             (SK_PATH_LDS_BYTES=0) -- the same pairs through both tiers, which is what a larger LDS budget could buy.
mapping      --map queries of 300 .. 500 points against a --target-point reference and its reversal, best target only
             (host form: the wall clock includes the upload of the pool): api.dtw_pairs over the best pairs against
             api.dtw_pairs_paths over them, then the paths alone from supplied records.
Per paths call: the share of pairs per tier, the bytes of a scratch slab, the wavefronts that shared the listed pairs
(sk_last_pair_paths_tiers).  Times are medians of --reps after a warm-up; `kernels` is the main interval of
sk_last_kernel_ms (the sweeps and the path launches, with the one read-back between them)."""
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
os.environ["SK_TUNING"] = "1"                   # (SK_PATH_LDS_BYTES is a tuning switch)
from squigglekit_amd import _lib, api, synth     # noqa: E402


def main_s(L):
    ms = C.c_float()
    _lib.check(L.sk_last_kernel_ms(None, C.byref(ms)))
    return float(ms.value) / 1e3


def summary(xs):
    return {"median_s": statistics.median(xs), "min_s": min(xs), "max_s": max(xs)}


def tiers(npairs):
    listed, slab, waves = api.last_pair_paths_tiers()
    return {"pairs": int(npairs), "lds_share": 1.0 - listed / max(npairs, 1), "scratch_share": listed / max(npairs, 1),
            "slab_bytes": int(slab), "scratch_waves": int(waves)}


def timed(calls, reps, L):
    wall = {k: [] for k in calls}
    kern = {k: [] for k in calls}
    info = {}
    for k, f in calls.items():                        # warm-up
        info[k] = f()
    for _ in range(reps):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            wall[k].append(time.perf_counter() - t0)
            kern[k].append(main_s(L))
    out = {}
    for k in calls:
        out[k] = {"wall": summary(wall[k]), "kernels": summary(kern[k])}
        if info[k]:
            out[k]["tiers"] = info[k]
    return out


def degenerate(L, R, M, N, reps):
    stride = (M + 7) // 8 * 8
    motif = synth.synthetic_motif(N)
    d_raw = L.sk_dev_alloc(R * stride * 2)
    d_pool, d_off = L.sk_dev_alloc((R * M + N) * 8), L.sk_dev_alloc((R + 1) * 8)
    d_out, d_sp = L.sk_dev_alloc(R * 24), L.sk_dev_alloc(R * N * 8)
    _lib.check(L.sk_synth_squiggles_dev(C.c_void_p(d_raw), stride, R, M, 2025, _lib.ptr(motif), motif.size))
    _lib.check(L.sk_synth_pa_dev(C.c_void_p(d_raw), stride, R, M, 16.0, 1493.94, 8192.0, C.c_void_p(d_pool), C.c_void_p(d_off)))
    query = np.ascontiguousarray((motif * 93.4 + 511.0 + 16.0) * (1493.94 / 8192.0))              # the motif as the reads hold it, in pA
    _lib.check(L.sk_dev_upload(C.c_void_p(d_pool + R * M * 8), _lib.ptr(query), query.nbytes))    # the query: sequence R
    _lib.check(L.sk_sync())
    L.sk_dev_free(C.c_void_p(d_raw))
    off = np.concatenate([np.arange(R + 1, dtype=np.int64) * M, [R * M + N]]).astype(np.int64)
    pairs = np.zeros(R, dtype=api.PAIR_DTYPE)
    pairs["query"], pairs["target"] = R, np.arange(R)

    def records():
        _lib.check(L.sk_dtw_pairs_dev(C.c_void_p(d_pool), _lib.ptr(off), R + 1, _lib.ptr(pairs), R, 0, C.c_void_p(d_out)))
        _lib.check(L.sk_sync())

    def paths(have, lds=None):
        if lds is not None:
            os.environ["SK_PATH_LDS_BYTES"] = str(lds)
        try:
            _lib.check(L.sk_dtw_pairs_paths_dev(C.c_void_p(d_pool), _lib.ptr(off), R + 1, _lib.ptr(pairs), R, 0,
                                                C.c_void_p(d_out), have, C.c_void_p(d_sp)))
            _lib.check(L.sk_sync())
        finally:
            os.environ.pop("SK_PATH_LDS_BYTES", None)
        return tiers(R)

    res = {"reads": R, "samples": M, "query": N, "cells": float(R) * M * N}
    res.update(timed({"records": records, "records_and_paths": lambda: paths(0), "paths_only": lambda: paths(1),
                      "paths_only_all_scratch": lambda: paths(1, 0)}, reps, L))
    res["mismatches"] = int(L.sk_last_path_mismatches())
    rec = np.zeros(R, dtype=api.HIT_DTYPE)
    _lib.check(L.sk_dev_download(_lib.ptr(rec), C.c_void_p(d_out), rec.nbytes))
    w = (rec["end"] - rec["start"] + 1)[~np.isnan(rec["dist"])]
    res["window_columns"] = {"median": float(np.median(w)), "p99": float(np.percentile(w, 99)), "max": int(w.max())}
    res["ratio_kernels"] = (res["records_and_paths"]["kernels"]["median_s"] / res["records"]["kernels"]["median_s"])
    for p in (d_pool, d_off, d_out, d_sp):
        L.sk_dev_free(C.c_void_p(p))
    return res


def mapping(L, Q, T, reps):
    rng = np.random.default_rng(5)
    ref = rng.normal(size=T)
    targets = [ref, np.ascontiguousarray(ref[::-1])]
    lens = rng.integers(300, 501, size=Q)
    queries = []
    for n in lens:                                    # windows of the reference, each point once or twice, with noise
        src = targets[int(rng.integers(0, 2))]
        w = int(n) * 2 // 3
        a = int(rng.integers(0, T - w))
        q = np.repeat(src[a:a + w], rng.integers(1, 3, size=w))[:int(n)]
        queries.append(q + rng.normal(scale=0.05, size=q.size))
    rec, best = api.map_queries(queries, targets)
    pool = api._as_pool(queries + targets)
    pr = np.stack([np.arange(Q), Q + best], axis=1)
    mine = rec[best, np.arange(Q)]

    def paths(records=None, lds=None):
        if lds is not None:
            os.environ["SK_PATH_LDS_BYTES"] = str(lds)
        try:
            api.dtw_pairs_paths(pool, pr, records=records)
        finally:
            os.environ.pop("SK_PATH_LDS_BYTES", None)
        return tiers(Q)

    res = {"queries": Q, "target": T, "query_points": int(lens.sum()), "cells_best_target": float(lens.sum()) * T}
    def records():
        api.dtw_pairs(pool, pr)

    res.update(timed({"records": records, "records_and_paths": paths,
                      "paths_only": lambda: paths(mine), "paths_only_all_scratch": lambda: paths(mine, 0)}, reps, L))
    res["mismatches"] = int(api.last_path_mismatches())
    w = mine["end"] - mine["start"] + 1
    res["window_columns"] = {"median": float(np.median(w)), "p99": float(np.percentile(w, 99)), "max": int(w.max())}
    res["ratio_kernels"] = (res["records_and_paths"]["kernels"]["median_s"] / res["records"]["kernels"]["median_s"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200000)
    ap.add_argument("--samples", type=int, default=4000)
    ap.add_argument("--query", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--map", type=int, default=100000, help="queries of the mapping shape (0: none)")
    ap.add_argument("--target", type=int, default=100000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.ensure_init()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernels_sha import kernels_sha
    res = {"tool": "pair_paths_throughput", "kernels_sha": kernels_sha(ROOT)}
    if a.reads > 0:
        res["degenerate"] = degenerate(L, a.reads, a.samples, a.query, a.reps)
    if a.map > 0:
        res["mapping"] = mapping(L, a.map, a.target, a.reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
