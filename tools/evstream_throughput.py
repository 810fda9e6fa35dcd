#!/usr/bin/env python3
"""Latency of an event session's pushes (csrc/sk_evstream.hip): one JSON line, also written to --out
(profiles/evstream_throughput.json).  Recorded, not gated.

    python tools/evstream_throughput.py [--slots 512,3000] [--chunk 2000] [--pushes 10] [--reads 5] [--out FILE]

The sequencer's shape: --slots channels, every one pushed --chunk int16 samples at a time, --pushes pushes per read, the
dna preset, END with the last push.  Device resident on both sides (sk_evs_push_dev_i16; sk_detect_events_dev_i16), timed
with HIP events around the launches (sk_last_kernel_ms: walk + scan + gather; mark + count + scan + fill).

per_push_ms   one push of all slots: median, min and max over the pushes of --reads reads after a warm-up read, and the
              median by push index (the first push of a read is fresh, the last one ends it)
read_ms       the --pushes pushes of a read, summed (median over the reads)
one_shot_ms   ONE sk_detect_events_dev_i16 call on the same slots x (chunk x pushes)-sample reads, in the same run
arrival_ms    what a chunk takes to arrive at 5 kHz: the yardstick of a push
state_bytes   the session's slot state (sk_last_evs_plan), with the staging rows of a push and its guard hits

One lane per slot: 512 slots are 8 wavefronts on a device of 256 compute units.  per_push_ms is a LATENCY figure -- how
long a decision waits for its events -- not a throughput figure."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["SK_TUNING"] = "1"
from squigglekit_amd import _lib, api, synth     # noqa: E402


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def main_ms(L):
    a, b = C.c_float(0), C.c_float(0)
    _lib.check(L.sk_last_kernel_ms(C.byref(a), C.byref(b)))
    return float(b.value)


def shape(L, S, E, P, reads):
    n = E * P
    sig = synth.squiggle_batch(S, n, 20261020 + S)                      # int16 [S, n]
    params = api.det_params("dna")
    vp = C.c_void_p
    d_sig, d_chunk = L.sk_dev_alloc(S * n * 2), L.sk_dev_alloc(S * E * 2)
    d_slots, d_len, d_end, d_full = (L.sk_dev_alloc(S * 4) for _ in range(4))
    cap = S * (n // 2 + 8)
    d_off, d_rec = L.sk_dev_alloc((S + 1) * 8), L.sk_dev_alloc(cap * 24)
    slots = np.arange(S, dtype=np.int32)
    for d, a in ((d_sig, sig), (d_slots, slots), (d_len, np.full(S, E, dtype=np.int32)), (d_full, np.full(S, n, dtype=np.int32))):
        _lib.check(L.sk_dev_upload(vp(d), _lib.ptr(a), a.nbytes))
    flags = [np.zeros(S, dtype=np.int32), np.ones(S, dtype=np.int32)]
    per_push, by_index, per_read = [], [[] for _ in range(P)], []
    got = []
    with api.EventStream(params, S) as es:
        for r in range(reads + 1):                                      # read 0 is the warm-up
            es.reset(slots)
            total, parts = 0.0, []
            for p in range(P):
                chunk = np.ascontiguousarray(sig[:, p * E:(p + 1) * E])
                _lib.check(L.sk_dev_upload(vp(d_chunk), _lib.ptr(chunk), chunk.nbytes))
                _lib.check(L.sk_dev_upload(vp(d_end), _lib.ptr(flags[p == P - 1]), 4 * S))
                _lib.check(L.sk_evs_push_dev_i16(es.handle, vp(d_slots), S, vp(d_chunk), E, vp(d_len), vp(d_end), vp(d_off),
                                                 vp(d_rec), cap))
                dt = main_ms(L)
                total += dt
                if r > 0:
                    per_push.append(dt)
                    by_index[p].append(dt)
                if r == reads:                                          # the last read's records, for the comparison below
                    off = np.zeros(S + 1, dtype=np.int64)
                    _lib.check(L.sk_dev_download(_lib.ptr(off), vp(d_off), off.nbytes))
                    rec = np.zeros(max(int(off[S]), 1), dtype=api.DET_EVENT_DTYPE)
                    _lib.check(L.sk_dev_download(_lib.ptr(rec), vp(d_rec), rec.nbytes))
                    parts.append((off, rec))
            if r > 0:
                per_read.append(total)
            got = parts
        plan = api.last_event_plan()
    one = []
    for k in range(reads + 1):
        _lib.check(L.sk_detect_events_dev_i16(vp(d_sig), n, vp(d_full), S, C.byref(params), vp(d_off), vp(d_rec), cap))
        dt = main_ms(L)
        if k > 0:
            one.append(dt)
    off = np.zeros(S + 1, dtype=np.int64)
    _lib.check(L.sk_dev_download(_lib.ptr(off), vp(d_off), off.nbytes))
    rec = np.zeros(int(off[S]), dtype=api.DET_EVENT_DTYPE)
    _lib.check(L.sk_dev_download(_lib.ptr(rec), vp(d_rec), rec.nbytes))
    same = all(np.concatenate([r_[o[s]:o[s + 1]] for o, r_ in got]).tobytes() == rec[off[s]:off[s + 1]].tobytes()
               for s in range(S))
    for p in (d_sig, d_chunk, d_slots, d_len, d_end, d_full, d_off, d_rec):
        L.sk_dev_free(vp(p))
    return {"slots": S, "wavefronts": (S + 63) // 64, "events": int(off[S]),
            "per_push_ms": spread(per_push), "per_push_ms_by_index": [statistics.median(v) for v in by_index],
            "read_ms": spread(per_read), "one_shot_ms": spread(one),
            "read_over_one_shot": statistics.median(per_read) / statistics.median(one),
            "arrival_ms": 1e3 * E / 5000.0, "same_records_as_one_shot": bool(same), "plan": plan}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="512,3000")
    ap.add_argument("--chunk", type=int, default=2000)
    ap.add_argument("--pushes", type=int, default=10)
    ap.add_argument("--reads", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.ensure_init()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernels_sha import kernels_sha
    res = {"tool": "evstream_throughput", "kernels_sha": kernels_sha(ROOT), "note": "one run on one MI355X",
           "preset": "dna", "chunk": a.chunk, "pushes": a.pushes, "reads": a.reads,
           "shapes": [shape(L, int(s), a.chunk, a.pushes, a.reads) for s in a.slots.split(",")]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
