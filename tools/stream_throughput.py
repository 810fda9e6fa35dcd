#!/usr/bin/env python3
"""MotifSeq session throughput (csrc/sk_stream.hip): one JSON line, and profiles/stream_throughput.json with --out.

    python tools/stream_throughput.py [--slots 512,3000] [--motifs 1,4] [--motif 200] [--chunk 2000] [--pushes 10]
                                      [--calib 2000] [--reps 5] [--out FILE]

Device-resident int16 rows (sk_synth_squiggles_dev, seeded): `slots` reads of pushes x chunk samples.  Per (slots, K),
`reps` times after a warm-up, in the same run:
  chunked    the read pushed in `pushes` chunks through sk_stream_push_dev_i16 (wall clock per push, each ends in a
             stream synchronisation; the slots are reset before every read) -- `push_ms` is the median over all pushes of
             all repetitions, `read_ms` the median sum of a read's pushes;
  whole      the same samples in ONE push (`whole_ms`): `chunking_cost` = read_ms / whole_ms;
  one_shot   sk_motifseq_multi_dev_i16 on the whole rows, the existing route (`one_shot_ms`);
  realtime_fraction = push_ms / 400: a 2 000-sample chunk at 5 kHz arrives every 0.4 s.
The final records of the chunked and the whole route are compared byte for byte on the way."""
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


def spread(xs):
    return {"median_ms": 1e3 * statistics.median(xs), "min_ms": 1e3 * min(xs), "max_ms": 1e3 * max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="512,3000")
    ap.add_argument("--motifs", default="1,4")
    ap.add_argument("--motif", type=int, default=200)
    ap.add_argument("--chunk", type=int, default=2000)
    ap.add_argument("--pushes", type=int, default=10)
    ap.add_argument("--calib", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.ensure_init()
    vp = C.c_void_p
    M = a.chunk * a.pushes
    out = {"motif": a.motif, "chunk": a.chunk, "pushes": a.pushes, "calib": a.calib, "reps": a.reps,
           "timing": "wall clock per call, each ends in a stream sync", "cases": []}
    for S in [int(v) for v in a.slots.split(",")]:
        d_sig, d_len, d_one = L.sk_dev_alloc(S * M * 2), L.sk_dev_alloc(S * 4), L.sk_dev_alloc(S * 4)
        d_slots = L.sk_dev_alloc(S * 4)
        motif0 = synth.synthetic_motif(a.motif)
        _lib.check(L.sk_synth_squiggles_dev(vp(d_sig), M, S, M, 2026, _lib.ptr(motif0), motif0.size))
        for d, v in ((d_len, np.full(S, a.chunk, dtype=np.int32)), (d_one, np.full(S, M, dtype=np.int32)),
                     (d_slots, np.arange(S, dtype=np.int32))):
            _lib.check(L.sk_dev_upload(vp(d), _lib.ptr(v), v.nbytes))
        for K in [int(v) for v in a.motifs.split(",")]:
            motifs = [synth.synthetic_motif(a.motif, seed=7 + k) for k in range(K)]
            _, flat, moff = api._flat_motifs(motifs)
            d_rec, d_hit = L.sk_dev_alloc(K * S * 40), L.sk_dev_alloc(K * S * 24)
            slots = np.arange(S, dtype=np.int32)
            with api.MotifStream(motifs, S, "medmad", 0, 1200, calib=a.calib) as ms:
                def chunked():
                    ms.reset(slots)
                    ts = []
                    for p in range(a.pushes):
                        t = time.perf_counter()
                        _lib.check(L.sk_stream_push_dev_i16(ms.handle, vp(d_slots), S, vp(d_sig + 2 * p * a.chunk), M, vp(d_len),
                                                            vp(d_rec)))
                        _lib.check(L.sk_sync())
                        ts.append(time.perf_counter() - t)
                    return ts

                def whole():
                    ms.reset(slots)
                    t = time.perf_counter()
                    _lib.check(L.sk_stream_push_dev_i16(ms.handle, vp(d_slots), S, vp(d_sig), M, vp(d_one), vp(d_rec)))
                    _lib.check(L.sk_sync())
                    return time.perf_counter() - t

                def one_shot():
                    t = time.perf_counter()
                    _lib.check(L.sk_motifseq_multi_dev_i16(vp(d_sig), M, vp(d_one), S, _lib.ptr(flat), _lib.ptr(moff), K, 0, 0,
                                                           1200, vp(d_hit)))
                    _lib.check(L.sk_sync())
                    return time.perf_counter() - t

                def records():
                    r = np.zeros((K, S), dtype=_lib.STREAM_DTYPE)
                    _lib.check(L.sk_dev_download(_lib.ptr(r), vp(d_rec), r.nbytes))
                    return r
                chunked()
                ra = records()
                whole()
                rb = records()
                one_shot()
                for f in ("dist", "tail", "start", "end", "n", "seen", "flags"):
                    assert ra[f].tobytes() == rb[f].tobytes(), "chunked and whole pushes differ in " + f
                pushes, reads, wholes, ones = [], [], [], []
                for _ in range(a.reps):
                    ts = chunked()
                    pushes += ts
                    reads.append(sum(ts))
                    wholes.append(whole())
                    ones.append(one_shot())
            case = {"slots": S, "K": K, "push": spread(pushes), "read": spread(reads), "whole": spread(wholes),
                    "one_shot": spread(ones)}
            case["push_ms"] = case["push"]["median_ms"]
            case["chunking_cost"] = case["read"]["median_ms"] / case["whole"]["median_ms"]
            case["realtime_fraction"] = case["push_ms"] / 400.0
            out["cases"].append(case)
            for p in (d_rec, d_hit):
                L.sk_dev_free(vp(p))
        for p in (d_sig, d_len, d_one, d_slots):
            L.sk_dev_free(vp(p))
    last = [c for c in out["cases"] if c["slots"] == 3000 and c["K"] == 4]
    if last:
        out["push_within_chunk_period"] = bool(last[0]["push_ms"] < 400.0)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    if last and not out["push_within_chunk_period"]:
        sys.exit("a push of 3 000 slots x 4 motifs takes longer than the 400 ms chunk period")


if __name__ == "__main__":
    main()
