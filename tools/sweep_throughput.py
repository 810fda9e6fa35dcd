#!/usr/bin/env python3
"""Segmenter parameter sweep throughput (csrc/sk_sweep.hip): one JSON line.

    python tools/sweep_throughput.py [--reads 100000] [--samples 4000] [--reps 5] [--out FILE]

Device-resident int16 rows (sk_synth_squiggles_dev, seeded).  For each grid, one sk_segment_sweep_dev_i16 call against
one sk_segment_dev_i16 call per set over the same buffers, the two alternated `reps` times after a warm-up: seconds
(median, min, max; wall clock around each, which ends in a stream synchronisation) and the ratio of the medians.
Grids: 64 sets = 8 std_scale values x 8 run-hopping sets (eight mask passes), 8 run-hopping sets (one group: several
reads per wavefront), 64 per-sample sets (error >= corrector).  The summaries of the sweep are checked against the
per-set calls' segment counts on the way."""
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
from squigglekit_amd import _lib, api          # noqa: E402


def grids():
    fast8 = dict(window=[100, 150], seg_dist=[0, 50], error=[3, 5])
    return {
        "64_sets_8_groups": api.sweep_grid(std_scale=[0.5, 0.625, 0.75, 0.875, 1.0, 1.125, 1.25, 1.5], **fast8),
        "8_sets_1_group": api.sweep_grid(**fast8),
        "64_sets_general": api.sweep_grid(error=[50, 60, 70, 80], corrector=[0, 50], window=[100, 150], seg_dist=[0, 50],
                                          stall_len=[0.25, 0.5]),
    }


def stats(xs):
    return {"median_s": statistics.median(xs), "min_s": min(xs), "max_s": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--samples", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.ensure_init()
    R, N = a.reads, a.samples
    stride = (N + 7) // 8 * 8
    d_sig = L.sk_dev_alloc(R * stride * 2)
    d_len = L.sk_dev_alloc(R * 4)
    max_segs = 64
    d_segs = L.sk_dev_alloc(R * 2 * max_segs * 4)
    d_nsegs = L.sk_dev_alloc(R * 4)
    d_sums = L.sk_dev_alloc(64 * 64)
    _lib.check(L.sk_synth_squiggles_dev(C.c_void_p(d_sig), stride, R, N, 2025, None, 0))
    lens = np.full(R, N, dtype=np.int32)
    _lib.check(L.sk_dev_upload(C.c_void_p(d_len), _lib.ptr(lens), lens.nbytes))
    _lib.check(L.sk_sync())
    out = {"reads": R, "samples": N, "reps": a.reps, "timing": "wall clock per call, ends in a stream sync"}
    nsegs = np.zeros(R, dtype=np.int32)
    for name, sets in grids().items():
        arr = (_lib.SweepSet * len(sets))(*sets)

        def sweep():
            _lib.check(L.sk_segment_sweep_dev_i16(C.c_void_p(d_sig), stride, C.c_void_p(d_len), R, arr, len(sets),
                                                  C.c_void_p(d_sums), None))

        def loop(check=None):
            for k, s in enumerate(sets):
                _lib.check(L.sk_segment_dev_i16(C.c_void_p(d_sig), stride, C.c_void_p(d_len), R, C.byref(s.seg),
                                                C.c_void_p(d_segs), C.c_void_p(d_nsegs), max_segs))
                if check is not None:
                    _lib.check(L.sk_sync())
                    _lib.check(L.sk_dev_download(_lib.ptr(nsegs), C.c_void_p(d_nsegs), nsegs.nbytes))
                    assert int(nsegs.astype(np.int64).sum()) == int(check[k]["segs"]), (name, k)
            _lib.check(L.sk_sync())
        sweep()
        sums = np.zeros(len(sets), dtype=_lib.SWEEP_SUM_DTYPE)
        _lib.check(L.sk_dev_download(_lib.ptr(sums), C.c_void_p(d_sums), sums.nbytes))
        loop(check=sums)                                   # (warm-up of the per-set route, and the check)
        ts, tl = [], []
        for _ in range(a.reps):
            t = time.perf_counter(); sweep(); ts.append(time.perf_counter() - t)
            t = time.perf_counter(); loop(); tl.append(time.perf_counter() - t)
        out[name] = {"sets": len(sets), "sweep": stats(ts), "per_set_calls": stats(tl),
                     "speedup": statistics.median(tl) / statistics.median(ts)}
    for p in (d_sig, d_len, d_segs, d_nsegs, d_sums):
        L.sk_dev_free(C.c_void_p(p))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
