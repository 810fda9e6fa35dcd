#!/usr/bin/env python3
"""Throughput of the adaptive-band DTW (csrc/sk_band.hip) against the full-matrix global mode in the same run: one JSON
line, also written to --out (profiles/band_throughput.json).  Recorded, not gated.

    python tools/band_throughput.py [--pairs 20000] [--query 10000] [--target 6000] [--distinct 256] [--reps 5]
                                    [--full-pairs 20000] [--full-points 1000] [--out FILE]

band     --pairs pairs of a --query-point query against a --target-point target, device resident.  A target is normal
         draws; its query is every target level repeated geometric(0.6) times plus N(0, 0.3) noise, cut or padded (last
         level) to --query points.  --distinct such pairs are made and the list cycles through them.  Per W = 64 / 128 /
         256: sk_dtw_band_dev records only and with paths (pinned end), medians of --reps after a warm-up;
         cells/s = pairs * (N + M - 1) * W / time.  paths_extra_s = with paths - records only: the direction-word stores
         and the back-trace on top of the forward sweep.
full     --full-pairs pairs of --full-points x --full-points normal draws through sk_dtw_pairs_dev in global mode: the
         full-matrix cell rate (pairs * N * M / time) to compare against.
Times: `kernels` is the main interval of sk_last_kernel_ms, `wall` the host clock around the call and its sync."""
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


def main_s(L):
    ms = C.c_float()
    _lib.check(L.sk_last_kernel_ms(None, C.byref(ms)))
    return float(ms.value) / 1e3


def summary(xs):
    return {"median_s": statistics.median(xs), "min_s": min(xs), "max_s": max(xs)}


def timed(f, reps, L):
    f()                                                 # warm-up
    wall, kern = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        wall.append(time.perf_counter() - t0)
        kern.append(main_s(L))
    return {"wall": summary(wall), "kernels": summary(kern)}


def upload(L, seqs):
    values, off = api._as_pool(seqs)
    d = L.sk_dev_alloc(values.nbytes)
    _lib.check(L.sk_dev_upload(C.c_void_p(d), _lib.ptr(values), values.nbytes))
    return d, off


def band(L, P, N, M, distinct, reps):
    rng = np.random.default_rng(7)
    seqs = []
    for _ in range(distinct):
        y = rng.normal(size=M)
        x = np.repeat(y, rng.geometric(0.6, size=M))
        x = np.concatenate([x, np.full(max(N - x.size, 0), y[-1])])[:N] + rng.normal(scale=0.3, size=N)
        seqs += [x, y]
    d_pool, off = upload(L, seqs)
    pairs = np.zeros(P, dtype=api.PAIR_DTYPE)
    k = np.arange(P) % distinct
    pairs["query"], pairs["target"] = 2 * k, 2 * k + 1
    d_rec, d_sp = L.sk_dev_alloc(P * 24), L.sk_dev_alloc(P * N * 8)
    res = {"pairs": P, "query": N, "target": M, "distinct_pairs": distinct, "end": "pinned", "widths": {}}

    def call(W, spans):
        _lib.check(L.sk_dtw_band_dev(C.c_void_p(d_pool), _lib.ptr(off), off.size - 1, _lib.ptr(pairs), P, W, 0,
                                     C.c_void_p(d_rec), C.c_void_p(d_sp) if spans else None))
        _lib.check(L.sk_sync())

    for W in api.BAND_WIDTHS:
        cells = float(P) * (N + M - 1) * W
        r = {"cells": cells}
        r["records"] = timed(lambda: call(W, False), reps, L)
        r["records_and_paths"] = timed(lambda: call(W, True), reps, L)
        r["mismatches"] = int(L.sk_last_path_mismatches())
        slab, waves, steps = api.last_band_plan()
        r["plan"] = {"slab_bytes": int(slab), "waves": int(waves), "steps_max": int(steps)}
        rec = np.zeros(P, dtype=api.HIT_DTYPE)
        _lib.check(L.sk_dev_download(_lib.ptr(rec), C.c_void_p(d_rec), rec.nbytes))
        r["lost"] = int(np.count_nonzero(rec["flags"] & _lib.SK_FLAG_BAND_LOST))
        r["dist_per_query_point_median"] = float(np.median(rec["dist"]) / N)
        tr, tp = r["records"]["kernels"]["median_s"], r["records_and_paths"]["kernels"]["median_s"]
        r["cells_per_s_records"] = cells / tr
        r["cells_per_s_paths"] = cells / tp
        r["paths_extra_s"] = tp - tr
        res["widths"][str(W)] = r
    for p in (d_pool, d_rec, d_sp):
        L.sk_dev_free(C.c_void_p(p))
    return res


def full(L, P, n, distinct, reps):
    rng = np.random.default_rng(8)
    d_pool, off = upload(L, [rng.normal(size=n) for _ in range(2 * distinct)])
    pairs = np.zeros(P, dtype=api.PAIR_DTYPE)
    k = np.arange(P) % distinct
    pairs["query"], pairs["target"] = 2 * k, 2 * k + 1
    d_rec = L.sk_dev_alloc(P * 24)

    def call():
        _lib.check(L.sk_dtw_pairs_dev(C.c_void_p(d_pool), _lib.ptr(off), off.size - 1, _lib.ptr(pairs), P,
                                      _lib.SK_PAIRS_GLOBAL, C.c_void_p(d_rec)))
        _lib.check(L.sk_sync())

    res = {"pairs": P, "points": n, "distinct_pairs": distinct, "cells": float(P) * n * n}
    res.update(timed(call, reps, L))
    res["cells_per_s"] = res["cells"] / res["kernels"]["median_s"]
    for p in (d_pool, d_rec):
        L.sk_dev_free(C.c_void_p(p))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=20000)
    ap.add_argument("--query", type=int, default=10000)
    ap.add_argument("--target", type=int, default=6000)
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--full-pairs", type=int, default=20000)
    ap.add_argument("--full-points", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.ensure_init()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernels_sha import kernels_sha
    res = {"tool": "band_throughput", "kernels_sha": kernels_sha(ROOT)}
    res["band"] = band(L, a.pairs, a.query, a.target, min(a.distinct, a.pairs), a.reps)
    if a.full_pairs > 0:
        res["full"] = full(L, a.full_pairs, a.full_points, min(a.distinct, a.full_pairs), a.reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
