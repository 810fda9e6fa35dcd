#!/usr/bin/env python3
"""MotifSeq hit-list throughput (csrc/sk_hits.hip, MODE_ROWS of csrc/sk_sdtw.hip): one JSON line.

    python tools/hits_throughput.py [--reads 200000] [--samples 4000] [--motif 200] [--reps 5] [--calls LIST]
                                    [--out FILE]

Device-resident int16 rows (sk_synth_squiggles_dev, seeded; the C4 shape by default).  Alternated `reps` times after a
warm-up, over the same buffers: sk_motifseq_hits_dev_i16 with K = 1 and K = 8, sk_motifseq_dev_i16 under
SK_DTW_SCHEME=full (the exact single pass) and under the default scheme (screening + certified window).  Seconds per
call (median, min, max; wall clock around each call, which ends in a stream synchronisation), reads per second, and
the K = 8 rate over the FULL rate.  `non_sweep_share_est` = 1 - FULL / (K = 8): the share of the K = 8 call that the
exact sweep alone does not account for (the row stores inside the sweep, the prep kernels, k_hits_select), from the
medians.  The time of k_hits_select itself comes from a kernel trace of the K = 8 call alone:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/hits_throughput.py --calls hits_k8 --reps 3
Hit 1 of the K = 8 call is checked against the FULL call's records on the way."""
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
    ap.add_argument("--calls", default="hits_k1,hits_k8,full,default", help="which calls to time (comma list)")
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
    d_one = L.sk_dev_alloc(R * 24)
    _lib.check(L.sk_synth_squiggles_dev(C.c_void_p(d_sig), stride, R, M, 2025, _lib.ptr(motif), motif.size))
    lens = np.full(R, M, dtype=np.int32)
    _lib.check(L.sk_dev_upload(C.c_void_p(d_len), _lib.ptr(lens), lens.nbytes))
    _lib.check(L.sk_sync())

    def hits(K):
        _lib.check(L.sk_motifseq_hits_dev_i16(C.c_void_p(d_sig), stride, C.c_void_p(d_len), R, _lib.ptr(motif),
                                              _lib.ptr(moff), 1, 0, 0, 1200, K, float("inf"), C.c_void_p(d_out),
                                              C.c_void_p(d_cnt)))
        _lib.check(L.sk_sync())

    def single(scheme):
        if scheme:
            os.environ["SK_DTW_SCHEME"] = scheme
        try:
            _lib.check(L.sk_motifseq_dev_i16(C.c_void_p(d_sig), stride, C.c_void_p(d_len), R, _lib.ptr(motif),
                                             motif.size, 0, 0, 1200, C.c_void_p(d_one)))
            _lib.check(L.sk_sync())
        finally:
            os.environ.pop("SK_DTW_SCHEME", None)

    calls = {"hits_k1": lambda: hits(1), "hits_k8": lambda: hits(8), "full": lambda: single("full"),
             "default": lambda: single(None)}
    calls = {k: calls[k] for k in a.calls.split(",")}
    for f in calls.values():                          # warm-up
        f()
    hits(8)                                           # the check: hit 1 = the exact pass's record
    got = np.zeros(R * 8, dtype=_lib.HIT_DTYPE)
    _lib.check(L.sk_dev_download(_lib.ptr(got), C.c_void_p(d_out), got.nbytes))
    single("full")
    want = np.zeros(R, dtype=_lib.HIT_DTYPE)
    _lib.check(L.sk_dev_download(_lib.ptr(want), C.c_void_p(d_one), want.nbytes))
    assert got.reshape(R, 8)[:, 0].tobytes() == want.tobytes(), "hit 1 differs from the exact pass"
    times = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, f in calls.items():
            t = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t)
    out = {"reads": R, "samples": M, "motif": a.motif, "reps": a.reps,
           "timing": "wall clock per call, ends in a stream sync"}
    for k in calls:
        out[k] = stats(times[k], R)
    if "hits_k8" in out and "full" in out:
        k8, full = out["hits_k8"]["median_s"], out["full"]["median_s"]
        out["k8_over_full_rate"] = full / k8
        out["non_sweep_share_est"] = 1.0 - full / k8
    for p in (d_sig, d_len, d_out, d_cnt, d_one):
        L.sk_dev_free(C.c_void_p(p))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
