#!/usr/bin/env python3
"""Segment-levels throughput (csrc/sk_seglev.hip behind the segmenter's int16 route): one JSON line.

    python tools/levels_throughput.py [--reads 200000] [--samples 4000] [--max-segs 64] [--reps 5] [--out FILE]

Device-resident int16 rows (sk_synth_squiggles_dev, seeded).  Alternated `reps` times after a warm-up, over the same
buffers: sk_segment_levels_dev_i16 and sk_segment_dev_i16 -- the yardstick, the call the levels ride on.  Seconds per
call (median, min, max; wall clock around each call, which ends in a stream synchronisation), reads per second and the
ratio levels / segment of the medians.  The segments of the levels call are checked against the segmenter call's on the
way.  Default --out: profiles/levels_throughput.json.
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
    ap.add_argument("--max-segs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "levels_throughput.json"))
    a = ap.parse_args()
    L = _lib.ensure_init()
    R, M, K = a.reads, a.samples, a.max_segs
    stride = (M + 7) // 8 * 8
    motif = synth.synthetic_motif(200)
    p = _lib.SegParams()
    d_sig, d_len = L.sk_dev_alloc(R * stride * 2), L.sk_dev_alloc(R * 4)
    d_segs, d_nsegs = L.sk_dev_alloc(R * K * 8), L.sk_dev_alloc(R * 4)
    d_lev, d_rl = L.sk_dev_alloc(R * K * 64), L.sk_dev_alloc(R * 64)
    bufs = (d_sig, d_len, d_segs, d_nsegs, d_lev, d_rl)
    assert all(bufs), "device allocation failed"
    _lib.check(L.sk_synth_squiggles_dev(C.c_void_p(d_sig), stride, R, M, 2025, _lib.ptr(motif), motif.size))
    lens = np.full(R, M, dtype=np.int32)
    _lib.check(L.sk_dev_upload(C.c_void_p(d_len), _lib.ptr(lens), lens.nbytes))
    _lib.check(L.sk_sync())

    def segment():
        _lib.check(L.sk_segment_dev_i16(C.c_void_p(d_sig), stride, C.c_void_p(d_len), R, C.byref(p), C.c_void_p(d_segs),
                                        C.c_void_p(d_nsegs), K))
        _lib.check(L.sk_sync())

    def levels():
        _lib.check(L.sk_segment_levels_dev_i16(C.c_void_p(d_sig), stride, C.c_void_p(d_len), R, C.byref(p),
                                               C.c_void_p(d_segs), C.c_void_p(d_nsegs), K, C.c_void_p(d_lev), C.c_void_p(d_rl)))
        _lib.check(L.sk_sync())

    def fetch():
        segs, nsegs = np.zeros((R, K, 2), dtype=np.int32), np.zeros(R, dtype=np.int32)
        _lib.check(L.sk_dev_download(_lib.ptr(segs), C.c_void_p(d_segs), segs.nbytes))
        _lib.check(L.sk_dev_download(_lib.ptr(nsegs), C.c_void_p(d_nsegs), nsegs.nbytes))
        return segs, nsegs

    calls = {"segment": segment, "levels": levels}
    for f in calls.values():                          # warm-up
        f()
    segment()
    want = fetch()
    levels()
    got = fetch()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "the levels call's segments differ"
    lev = np.zeros((R, K), dtype=_lib.LEVEL_DTYPE)
    _lib.check(L.sk_dev_download(_lib.ptr(lev), C.c_void_p(d_lev), lev.nbytes))
    out = {"reads": R, "samples": M, "max_segs": K, "reps": a.reps, "timing": "wall clock per call, ends in a stream sync",
           "segments": int(want[1].sum()), "records_with_a_span": int((lev["n"] > 0).sum()),
           "median_segment_length": float(np.median(lev["n"][lev["n"] > 0])) if (lev["n"] > 0).any() else 0.0}
    times = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, f in calls.items():
            t = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t)
    for k in calls:
        out[k] = stats(times[k], R)
    out["levels_over_segment"] = out["levels"]["median_s"] / out["segment"]["median_s"]
    for b in bufs:
        L.sk_dev_free(C.c_void_p(b))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
