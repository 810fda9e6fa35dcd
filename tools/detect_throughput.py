#!/usr/bin/env python3
"""Event-detection throughput (csrc/sk_detect.hip): one JSON line.

    python tools/detect_throughput.py [--reads 200000] [--samples 4000] [--reps 5] [--ref-reads 200] [--out FILE]

Device-resident int16 rows (sk_synth_squiggles_dev, seeded).  After a warm-up and a counting call that sizes the records,
alternated `reps` times over the same buffers: sk_detect_events_dev_i16 with the dna and with the rna preset, and
sk_segment_dev_i16 -- the yardstick, a kernel that streams the same bytes.  Seconds per call (median, min, max; wall
clock around each call, which ends in a stream synchronisation), events per read, and per preset the share of the HBM
peak (8 TB/s) that 2 bytes per sample in plus 24 bytes per event out amount to at the median -- what the call has to
move, not what it does move: the samples are read twice and the mark words once written and twice read -- and the ratio
detect / segment of the medians.  The numpy statement (tests/detect_ref.py) is timed on --ref-reads of the same reads on
one host core, its records compared with the device's on the way; ref_over_detect is per read.
Default --out: profiles/detect_throughput.json.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["SK_TUNING"] = "1"
from squigglekit_amd import _lib, api, synth     # noqa: E402
import detect_ref                                # noqa: E402

HBM_PEAK = 8.0e12                                # bytes per second, MI355X


def stats(xs, reads):
    med = statistics.median(xs)
    return {"median_s": med, "ms_per_call": med * 1e3, "min_s": min(xs), "max_s": max(xs), "reads_per_s": reads / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200000)
    ap.add_argument("--samples", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-reads", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_throughput.json"))
    a = ap.parse_args()
    L = _lib.ensure_init()
    R, M, K = a.reads, a.samples, 64
    stride = (M + 7) // 8 * 8
    motif = synth.synthetic_motif(200)
    seg = _lib.SegParams()
    presets = {"dna": api.det_params("dna"), "rna": api.det_params("rna")}
    d_sig, d_len, d_off = L.sk_dev_alloc(R * stride * 2), L.sk_dev_alloc(R * 4), L.sk_dev_alloc((R + 1) * 8)
    d_segs, d_nsegs = L.sk_dev_alloc(R * K * 8), L.sk_dev_alloc(R * 4)
    bufs = [d_sig, d_len, d_off, d_segs, d_nsegs]
    assert all(bufs), "device allocation failed"
    _lib.check(L.sk_synth_squiggles_dev(C.c_void_p(d_sig), stride, R, M, 2025, _lib.ptr(motif), motif.size))
    lens = np.full(R, M, dtype=np.int32)
    _lib.check(L.sk_dev_upload(C.c_void_p(d_len), _lib.ptr(lens), lens.nbytes))
    _lib.check(L.sk_sync())

    def detect(p, d_rec, cap):
        _lib.check(L.sk_detect_events_dev_i16(C.c_void_p(d_sig), stride, C.c_void_p(d_len), R, C.byref(p), C.c_void_p(d_off),
                                              C.c_void_p(d_rec) if cap else None, cap))
        _lib.check(L.sk_sync())

    def offsets():
        off = np.zeros(R + 1, dtype=np.int64)
        _lib.check(L.sk_dev_download(_lib.ptr(off), C.c_void_p(d_off), off.nbytes))
        return off

    events = {}
    for name, p in presets.items():                  # the counting calls
        detect(p, None, 0)
        events[name] = int(offsets()[R])
    cap = max(events.values())
    d_rec = L.sk_dev_alloc(max(cap, 1) * 24)
    assert d_rec, "device allocation failed"
    bufs.append(d_rec)

    def segment():
        _lib.check(L.sk_segment_dev_i16(C.c_void_p(d_sig), stride, C.c_void_p(d_len), R, C.byref(seg), C.c_void_p(d_segs),
                                        C.c_void_p(d_nsegs), K))
        _lib.check(L.sk_sync())

    calls = {"segment": segment}
    for name, p in presets.items():
        calls[name] = lambda p=p: detect(p, d_rec, cap)
    for f in calls.values():                          # warm-up
        f()
    times = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, f in calls.items():
            t = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t)
    out = {"reads": R, "samples": M, "reps": a.reps, "timing": "wall clock per call, ends in a stream sync",
           "hbm_peak_bytes_per_s": HBM_PEAK, "segment": stats(times["segment"], R)}
    for name in presets:
        s = stats(times[name], R)
        s["events"] = events[name]
        s["events_per_read"] = events[name] / max(R, 1)
        s["bytes_min"] = 2 * R * M + 24 * events[name]
        s["hbm_share"] = s["bytes_min"] / s["median_s"] / HBM_PEAK
        s["detect_over_segment"] = s["median_s"] / out["segment"]["median_s"]
        out[name] = s

    # the numpy statement on one host core, on the first reads of the same batch (and a check of the device's records)
    n = min(a.ref_reads, R)
    if n > 0:
        rows = np.zeros((n, stride), dtype=np.int16)
        _lib.check(L.sk_dev_download(_lib.ptr(rows), C.c_void_p(d_sig), rows.nbytes))
        reads = [rows[r, :M] for r in range(n)]
        for name, p in presets.items():
            t = time.perf_counter()
            woff, wrec = detect_ref.detect(reads, detect_ref.PRESETS[name])
            ref_s = time.perf_counter() - t
            detect(p, d_rec, cap)
            off = offsets()
            rec = np.zeros(int(off[n]), dtype=api.DET_EVENT_DTYPE)
            if rec.size:
                _lib.check(L.sk_dev_download(_lib.ptr(rec), C.c_void_p(d_rec), rec.nbytes))
            assert np.array_equal(off[:n + 1], woff) and rec.tobytes() == wrec.tobytes(), "the device differs from detect_ref"
            out[name]["ref_reads"] = n
            out[name]["ref_s_per_read_one_core"] = ref_s / n
            out[name]["ref_over_detect"] = (ref_s / n) / (out[name]["median_s"] / R)
    for b in bufs:
        L.sk_dev_free(C.c_void_p(b))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
