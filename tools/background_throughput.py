#!/usr/bin/env python3
"""MotifSeq read-background throughput (csrc/sk_bg.hip beside the hit-list path): one JSON line.

    python tools/background_throughput.py [--reads 200000] [--samples 4000] [--motif 200] [--reps 5] [--calls LIST]
                                          [--out FILE]

Device-resident int16 rows (sk_synth_squiggles_dev, seeded; the shape of tools/hits_throughput.py).  Alternated `reps`
times after a warm-up, over the same buffers: sk_motifseq_background_dev_i16 and sk_motifseq_hits_dev_i16 -- the
yardstick, code the background records do not touch -- with K = 1 and K = 8.  Seconds per call (median, min, max; wall
clock around each call, which ends in a stream synchronisation), reads per second, and per K the ratio background /
hits of the medians.  The hit lists of the background call are checked against the hit-list call's on the way, and the
share of unflagged reads with std > 0 and mad > 0 is reported.  The time of k_row_background itself comes from a
kernel trace of the K = 8 background call alone, in a run of its own without counters:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/background_throughput.py --calls bg_k8 --reps 3
"""
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
    ap.add_argument("--calls", default="hits_k1,bg_k1,hits_k8,bg_k8", help="which calls to time (comma list)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.ensure_init()
    R, M = a.reads, a.samples
    stride = (M + 7) // 8 * 8
    motif = synth.synthetic_motif(a.motif)
    moff = np.array([0, motif.size], dtype=np.int32)
    d_sig = L.sk_dev_alloc(R * stride * 2)
    d_len = L.sk_dev_alloc(R * 4)
    d_out = L.sk_dev_alloc(R * 8 * 24)
    d_cnt = L.sk_dev_alloc(R * 4)
    d_bg = L.sk_dev_alloc(R * 48)
    _lib.check(L.sk_synth_squiggles_dev(C.c_void_p(d_sig), stride, R, M, 2025, _lib.ptr(motif), motif.size))
    lens = np.full(R, M, dtype=np.int32)
    _lib.check(L.sk_dev_upload(C.c_void_p(d_len), _lib.ptr(lens), lens.nbytes))
    _lib.check(L.sk_sync())

    def hits(K):
        _lib.check(L.sk_motifseq_hits_dev_i16(C.c_void_p(d_sig), stride, C.c_void_p(d_len), R, _lib.ptr(motif),
                                              _lib.ptr(moff), 1, 0, 0, 1200, K, float("inf"), C.c_void_p(d_out),
                                              C.c_void_p(d_cnt)))
        _lib.check(L.sk_sync())

    def background(K):
        _lib.check(L.sk_motifseq_background_dev_i16(C.c_void_p(d_sig), stride, C.c_void_p(d_len), R, _lib.ptr(motif),
                                                    _lib.ptr(moff), 1, 0, 0, 1200, K, float("inf"), C.c_void_p(d_out),
                                                    C.c_void_p(d_cnt), C.c_void_p(d_bg)))
        _lib.check(L.sk_sync())

    def fetch(K):
        got = np.zeros(R * K, dtype=_lib.HIT_DTYPE)
        cnt = np.zeros(R, dtype=np.int32)
        _lib.check(L.sk_dev_download(_lib.ptr(got), C.c_void_p(d_out), got.nbytes))
        _lib.check(L.sk_dev_download(_lib.ptr(cnt), C.c_void_p(d_cnt), cnt.nbytes))
        return got.tobytes(), cnt.tobytes()

    calls = {"hits_k1": lambda: hits(1), "bg_k1": lambda: background(1), "hits_k8": lambda: hits(8),
             "bg_k8": lambda: background(8)}
    calls = {k: calls[k] for k in a.calls.split(",")}
    for f in calls.values():                          # warm-up
        f()
    out = {"reads": R, "samples": M, "motif": a.motif, "reps": a.reps,
           "timing": "wall clock per call, ends in a stream sync"}
    for K in (1, 8):                                  # the check: the twin's hit lists, byte for byte
        hits(K)
        want = fetch(K)
        background(K)
        assert fetch(K) == want, "the background call's hit lists differ from the hit-list call's (K = %d)" % K
    bg = np.zeros(R, dtype=_lib.BG_DTYPE)
    _lib.check(L.sk_dev_download(_lib.ptr(bg), C.c_void_p(d_bg), bg.nbytes))
    out["usable_share"] = float(np.mean((bg["below"] >= 0) & (bg["std"] > 0) & (bg["mad"] > 0)))
    out["median_row_mean"], out["median_row_std"] = float(np.median(bg["mean"])), float(np.median(bg["std"]))
    times = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, f in calls.items():
            t = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t)
    for k in calls:
        out[k] = stats(times[k], R)
    for K in (1, 8):
        if "bg_k%d" % K in out and "hits_k%d" % K in out:
            out["bg_over_hits_k%d" % K] = out["bg_k%d" % K]["median_s"] / out["hits_k%d" % K]["median_s"]
    for p in (d_sig, d_len, d_out, d_cnt, d_bg):
        L.sk_dev_free(C.c_void_p(p))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
