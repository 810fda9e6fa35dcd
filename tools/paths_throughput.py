#!/usr/bin/env python3
"""MotifSeq alignment-path throughput (csrc/sk_path.hip): one JSON line.

    python tools/paths_throughput.py [--reads 200000] [--samples 4000] [--motif 200] [--reps 5] [--calls LIST]
                                     [--out FILE]

Device-resident int16 rows (sk_synth_squiggles_dev, seeded; the C4 shape by default).  Alternated `reps` times after a
warm-up, over the same buffers: sk_motifseq_hits_dev_i16 (the baseline: the hit list alone, the code of the commit
before paths existed) and sk_motifseq_paths_dev_i16 (hit list, then the path pass), each with K = 1 and K = 8.  Seconds
per call (median, min, max; wall clock around each call, which ends in a stream synchronisation), reads per second,
`paths_over_hits` = the paths call's median over the hit-list call's, and `path_pass_share_est` = 1 - hits / paths.
`widths`: the distribution of the window width W = end - start + 1 over the hits of the K = 8 call (what the path pass
sweeps, N x W cells per hit, against the N x n of the row pass) and the share the LDS tier takes.  The records of the
paths call are checked against the hit-list call's, the spans against the records, and the self-check counter against 0.
The path kernels alone come from a kernel trace:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/paths_throughput.py --calls paths_k8 --reps 3"""
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
from squigglekit_amd import _lib, synth          # noqa: E402


def stats(xs, reads):
    med = statistics.median(xs)
    return {"median_s": med, "min_s": min(xs), "max_s": max(xs), "reads_per_s": reads / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200000)
    ap.add_argument("--samples", type=int, default=4000)
    ap.add_argument("--motif", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", default="hits_k1,paths_k1,hits_k8,paths_k8", help="which calls to time (comma list)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.ensure_init()
    R, M, N = a.reads, a.samples, a.motif
    stride = (M + 7) // 8 * 8
    motif = synth.synthetic_motif(N)
    moff = np.array([0, motif.size], dtype=np.int32)
    d_sig = L.sk_dev_alloc(R * stride * 2)
    d_len = L.sk_dev_alloc(R * 4)
    d_out = L.sk_dev_alloc(R * 8 * 24)
    d_cnt = L.sk_dev_alloc(R * 4)
    d_spans = L.sk_dev_alloc(R * 8 * N * 8)
    _lib.check(L.sk_synth_squiggles_dev(C.c_void_p(d_sig), stride, R, M, 2025, _lib.ptr(motif), motif.size))
    lens = np.full(R, M, dtype=np.int32)
    _lib.check(L.sk_dev_upload(C.c_void_p(d_len), _lib.ptr(lens), lens.nbytes))
    _lib.check(L.sk_sync())

    def hits(K):
        _lib.check(L.sk_motifseq_hits_dev_i16(C.c_void_p(d_sig), stride, C.c_void_p(d_len), R, _lib.ptr(motif),
                                              _lib.ptr(moff), 1, 0, 0, 1200, K, float("inf"), C.c_void_p(d_out),
                                              C.c_void_p(d_cnt)))
        _lib.check(L.sk_sync())

    def paths(K):
        _lib.check(L.sk_motifseq_paths_dev_i16(C.c_void_p(d_sig), stride, C.c_void_p(d_len), R, _lib.ptr(motif),
                                               _lib.ptr(moff), 1, 0, 0, 1200, K, float("inf"), C.c_void_p(d_out),
                                               C.c_void_p(d_cnt), C.c_void_p(d_spans)))
        _lib.check(L.sk_sync())

    calls = {"hits_k1": lambda: hits(1), "paths_k1": lambda: paths(1), "hits_k8": lambda: hits(8),
             "paths_k8": lambda: paths(8)}
    calls = {k: calls[k] for k in a.calls.split(",")}
    for f in calls.values():                          # warm-up
        f()
    hits(8)                                           # the check: same records, spans that fit them, no mismatch
    want = np.zeros(R * 8, dtype=_lib.HIT_DTYPE)
    _lib.check(L.sk_dev_download(_lib.ptr(want), C.c_void_p(d_out), want.nbytes))
    paths(8)
    assert L.sk_last_path_mismatches() == 0, "the path self-check counted a mismatch"
    got = np.zeros(R * 8, dtype=_lib.HIT_DTYPE)
    _lib.check(L.sk_dev_download(_lib.ptr(got), C.c_void_p(d_out), got.nbytes))
    assert got.tobytes() == want.tobytes(), "the paths call's records differ from the hit list's"
    rows = min(R, 2000)
    sp = np.zeros((rows, 8, N, 2), dtype=np.int32)
    _lib.check(L.sk_dev_download(_lib.ptr(sp), C.c_void_p(d_spans), sp.nbytes))
    g = got.reshape(R, 8)[:rows]
    live = g["start"] >= 0
    assert np.array_equal(sp[:, :, 0, 0][live], g["start"][live]) and np.array_equal(sp[:, :, -1, 1][live], g["end"][live])
    assert np.all(sp[~live] == -1)
    w = (got["end"] - got["start"] + 1)[got["start"] >= 0].astype(np.int64)
    words = N * ((w + 15) // 16)
    widths = {"hits": int(w.size), "min": int(w.min()), "median": float(np.median(w)), "p90": float(np.percentile(w, 90)),
              "p99": float(np.percentile(w, 99)), "max": int(w.max()), "median_over_samples": float(np.median(w)) / M,
              "lds_tier_share": float(np.mean((words <= 6400) & (w <= 1024)))}
    times = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, f in calls.items():
            t = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t)
    out = {"reads": R, "samples": M, "motif": N, "reps": a.reps,
           "timing": "wall clock per call, ends in a stream sync", "widths": widths}
    for k in calls:
        out[k] = stats(times[k], R)
    for K in ("k1", "k8"):
        if "hits_" + K in out and "paths_" + K in out:
            h, p = out["hits_" + K]["median_s"], out["paths_" + K]["median_s"]
            out["paths_over_hits_" + K] = p / h
            out["path_pass_share_est_" + K] = 1.0 - h / p
    for p in (d_sig, d_len, d_out, d_cnt, d_spans):
        L.sk_dev_free(C.c_void_p(p))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
