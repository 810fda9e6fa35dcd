#!/usr/bin/env python3
"""MotifSeq events and pooling throughput (csrc/sk_events.hip beside the path kernel): one JSON line.

    python tools/events_throughput.py [--reads 200000] [--samples 4000] [--motif 200] [--reps 5] [--calls LIST]
                                      [--out FILE]

Device-resident int16 rows (sk_synth_squiggles_dev, seeded; the shape of tools/background_throughput.py).  Alternated
`reps` times after a warm-up, over the same buffers: sk_motifseq_events_dev_i16 and sk_motifseq_paths_dev_i16 -- the
yardstick, code the events do not touch -- with K = 1 and K = 8.  Seconds per call (median, min, max; wall clock around
each call, which ends in a stream synchronisation), reads per second, and per K the ratio events / paths of the
medians.  The hit lists of the events call are checked against the paths call's on the way (K = 8 and K = 1), and at
K = 1 its events against the spans, `--check_reads` reads at a time.  Then the K = 1 events are pooled:
sk_events_pool_dev on the device-resident records against numpy on the same records on the host (the reductions of the
contract, column by column), `pool_reps` times each.  Host memory: the K = 1 records (reads x motif x 32 bytes: 1.3 GB at
the default size) plus one chunk of spans; the K = 8 records (10 GB) never leave the device.  No time is gated.
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
from squigglekit_amd import _lib, api, synth          # noqa: E402


def stats(xs, reads):
    med = statistics.median(xs)
    return {"median_s": med, "min_s": min(xs), "max_s": max(xs), "reads_per_s": reads / med}


def numpy_pool(ev):
    """The contract's reductions on the host: events [H, N] -> POOL_DTYPE[N]."""
    sel = ev["dwell"][:, 0] > 0
    out = np.zeros(ev.shape[1], dtype=_lib.POOL_DTYPE)
    for i in range(ev.shape[1]):
        col = ev[sel, i]
        s, d = np.ascontiguousarray(col["sum"]), np.ascontiguousarray(col["dwell"])
        total = int(d.astype(np.int64).sum())
        out[i] = (np.sum(s) / total, np.std(s / d), np.mean(np.ascontiguousarray(col["std"])), total / col.size,
                  np.std(d.astype(np.float64)), np.mean(np.ascontiguousarray(col["cost"])), col.size)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200000)
    ap.add_argument("--samples", type=int, default=4000)
    ap.add_argument("--motif", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pool_reps", type=int, default=2)
    ap.add_argument("--check_reads", type=int, default=20000, help="reads per chunk of the events-against-spans check")
    ap.add_argument("--calls", default="paths_k1,events_k1,paths_k8,events_k8", help="which calls to time (comma list)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.ensure_init()
    R, M, N = a.reads, a.samples, a.motif
    stride = (M + 7) // 8 * 8
    motif = synth.synthetic_motif(N)
    moff = np.array([0, N], dtype=np.int32)
    vp = C.c_void_p
    d_sig, d_len = L.sk_dev_alloc(R * stride * 2), L.sk_dev_alloc(R * 4)
    d_out, d_cnt = L.sk_dev_alloc(R * 8 * 24), L.sk_dev_alloc(R * 4)
    d_spans, d_ev, d_pool = L.sk_dev_alloc(R * 8 * N * 8), L.sk_dev_alloc(R * 8 * N * 32), L.sk_dev_alloc(N * 56)
    bufs = (d_sig, d_len, d_out, d_cnt, d_spans, d_ev, d_pool)
    assert all(bufs), "device allocation failed"
    _lib.check(L.sk_synth_squiggles_dev(vp(d_sig), stride, R, M, 2025, _lib.ptr(motif), N))
    lens = np.full(R, M, dtype=np.int32)
    _lib.check(L.sk_dev_upload(vp(d_len), _lib.ptr(lens), lens.nbytes))
    _lib.check(L.sk_sync())

    def run(entry, K, d_res):
        _lib.check(entry(vp(d_sig), stride, vp(d_len), R, _lib.ptr(motif), _lib.ptr(moff), 1, 0, 0, 1200, K,
                         float("inf"), vp(d_out), vp(d_cnt), vp(d_res)))
        _lib.check(L.sk_sync())

    def fetch(K):
        got = np.zeros(R * K, dtype=_lib.HIT_DTYPE)
        cnt = np.zeros(R, dtype=np.int32)
        _lib.check(L.sk_dev_download(_lib.ptr(got), vp(d_out), got.nbytes))
        _lib.check(L.sk_dev_download(_lib.ptr(cnt), vp(d_cnt), cnt.nbytes))
        return got.tobytes(), cnt.tobytes()

    calls = {"paths_k1": lambda: run(L.sk_motifseq_paths_dev_i16, 1, d_spans),
             "events_k1": lambda: run(L.sk_motifseq_events_dev_i16, 1, d_ev),
             "paths_k8": lambda: run(L.sk_motifseq_paths_dev_i16, 8, d_spans),
             "events_k8": lambda: run(L.sk_motifseq_events_dev_i16, 8, d_ev)}
    calls = {k: calls[k] for k in a.calls.split(",")}
    for f in calls.values():                          # warm-up
        f()
    out = {"reads": R, "samples": M, "motif": N, "reps": a.reps, "timing": "wall clock per call, ends in a stream sync"}
    for K in (8, 1):                                  # the check: the twin's hit lists, byte for byte
        run(L.sk_motifseq_paths_dev_i16, K, d_spans)
        want = fetch(K)
        run(L.sk_motifseq_events_dev_i16, K, d_ev)
        assert fetch(K) == want, "the events call's hit lists differ from the paths call's (K = %d)" % K
        assert L.sk_last_path_mismatches() == 0
    ev = np.zeros((R, N), dtype=_lib.EVENT_DTYPE)     # K = 1 (the last pair of calls): its events against its spans
    _lib.check(L.sk_dev_download(_lib.ptr(ev), vp(d_ev), ev.nbytes))
    for lo in range(0, R, a.check_reads):
        n = min(a.check_reads, R - lo)
        spans = np.zeros((n, N, 2), dtype=np.int32)
        _lib.check(L.sk_dev_download(_lib.ptr(spans), vp(d_spans + lo * N * 8), spans.nbytes))
        assert np.array_equal(api.spans_of_events(ev[lo:lo + n]), spans), "events and spans disagree (reads %d..)" % lo
    dw = ev["dwell"][ev["dwell"] > 0]
    out["dwell_k1"] = {"median": float(np.median(dw)), "p99": float(np.percentile(dw, 99)), "max": int(dw.max()),
                       "above_128": int((dw > 128).sum())}
    times = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, f in calls.items():
            t = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t)
    for k in calls:
        out[k] = stats(times[k], R)
    for K in (1, 8):
        if "events_k%d" % K in out and "paths_k%d" % K in out:
            out["events_over_paths_k%d" % K] = out["events_k%d" % K]["median_s"] / out["paths_k%d" % K]["median_s"]
    # pooling: the K = 1 events as they lie on the device (made again: the timed calls wrote over them) against numpy on
    # the host copy
    run(L.sk_motifseq_events_dev_i16, 1, d_ev)
    flat = ev
    tg, tn = [], []
    pool = np.zeros(N, dtype=_lib.POOL_DTYPE)
    for _ in range(a.pool_reps):
        t = time.perf_counter()
        _lib.check(L.sk_events_pool_dev(vp(d_ev), None, flat.shape[0], N, vp(d_pool)))
        _lib.check(L.sk_dev_download(_lib.ptr(pool), vp(d_pool), pool.nbytes))
        tg.append(time.perf_counter() - t)
        t = time.perf_counter()
        want = numpy_pool(flat)
        tn.append(time.perf_counter() - t)
    assert pool.tobytes() == want.tobytes(), "the pooled model differs from numpy's"
    out["pool_hits"] = int(pool["hits"][0])
    out["pool_gpu"], out["pool_numpy"] = stats(tg, flat.shape[0]), stats(tn, flat.shape[0])
    out["pool_numpy_over_gpu"] = out["pool_numpy"]["median_s"] / out["pool_gpu"]["median_s"]
    for p in bufs:
        L.sk_dev_free(vp(p))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
