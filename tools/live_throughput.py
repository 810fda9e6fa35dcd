#!/usr/bin/env python3
"""Latency of a live mapping session's pushes (csrc/sk_live.hip) beside the unfused route squiggle_map_stream --live takes:
one JSON line, also written to --out (profiles/live_throughput.json).  Recorded, not gated.

    python tools/live_throughput.py [--slots 512,3000] [--chunk 2000] [--pushes 10] [--reads 5] [--calib 200]
                                    [--target 100000] [--out FILE]

The sequencer's shape: --slots channels, every one pushed --chunk int16 samples at a time, --pushes pushes per read, the
dna preset, END with the last push, --calib calibration events, a --target-point reference and its reversal as targets.
Measured in the same run, per push of all slots (medians over the pushes of --reads reads after a warm-up read, with min
and max):

fused_wall_ms     (a) wall time of one host-form api.LiveMap.push with the device rule: samples up, records, info and
                  decisions down
unfused_wall_ms   (b) wall time of the same push as replay_live makes it: EventStream.push, event_levels, the per-slot
                  numpy loop (concatenate, hold back, mean / std, normalise), MapStream.push, map_decide
fused_kernel_ms   (c) sk_last_kernel_ms of the fused push (event cutting to summary, the read-back and the host-side plan
                  of the sweep included), with bridge_ms (count, scan, fill) and summary_ms from HIP events of their own
fused_over_unfused  median (a) / median (b)

The records of the two routes are compared push by push (same_records)."""
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
from squigglekit_amd import _lib, api, synth     # noqa: E402

RULE = (100, 0.5, 0.05, 400)                      # squiggle_map_stream's defaults


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


class _Read:
    def __init__(self):
        self.levels, self.mean, self.sd, self.ended = np.zeros(0), None, None, False


def unfused_push(es, ms, chan, slots, chunks, end, Cal):
    """one push of replay_live (squigglekit_amd/mapstream_cli.py), without the output lines"""
    off, rec = es.push(slots, chunks, end=end)
    values, _ = api.event_levels(off, rec)
    mslots, mchunks = [], []
    for i, s in enumerate(slots):
        r = chan[s]
        r.ended = bool(end[i])
        had = len(r.levels)
        r.levels = np.concatenate([r.levels, values[int(off[i]):int(off[i + 1])]])
        if r.sd is None:
            if len(r.levels) < Cal and not r.ended:
                continue
            head = r.levels[:Cal]
            sd = head.std() if head.size >= 2 else 0.0
            if not sd > 0:
                continue
            r.mean, r.sd = head.mean(), sd
            had = 0
        new = (r.levels[had:] - r.mean) / r.sd
        if new.size == 0 and not r.ended:
            continue
        mslots.append(s)
        mchunks.append(new)
    if not mslots:
        return mslots, None, None
    mrec = ms.push(mslots, mchunks)
    return mslots, mrec, api.map_decide(mrec, *RULE)[1]


def shape(L, S, E, P, reads, Cal, targets):
    n = E * P
    sig = synth.squiggle_batch(S, n, 20261020 + S)                      # int16 [S, n]
    params = api.det_params("dna")
    slots = np.arange(S, dtype=np.int32)
    rule = api.live_rule(*RULE)
    flags = [np.zeros(S, dtype=np.int32), np.ones(S, dtype=np.int32)]
    fused, unfused, kernel, bridge, summary = [], [], [], [], []
    by_index = [[] for _ in range(P)]
    same, levels, decided = True, 0, 0
    a, b = C.c_float(0), C.c_float(0)
    with api.LiveMap(params, Cal, targets, S) as lm, api.EventStream(params, S) as es, api.MapStream(targets, S) as ms:
        for r in range(reads + 1):                                      # read 0 is the warm-up
            lm.reset(slots)
            es.reset(slots)
            ms.reset(slots)
            chan = [_Read() for _ in range(S)]
            for p in range(P):
                chunk = np.ascontiguousarray(sig[:, p * E:(p + 1) * E])
                end = flags[p == P - 1]
                chunks = [chunk[i] for i in range(S)]                  # both routes get the list replay_live builds
                t0 = time.perf_counter()
                rec, info, best = lm.push(slots, chunks, end=end, rule=rule)
                t1 = time.perf_counter()
                _lib.check(L.sk_last_kernel_ms(C.byref(a), C.byref(b)))
                k_ms = float(b.value)
                _lib.check(L.sk_live_last_ms(lm.handle, C.byref(a), C.byref(b)))
                t2 = time.perf_counter()
                mslots, mrec, dec = unfused_push(es, ms, chan, slots, chunks, end, Cal)
                t3 = time.perf_counter()
                if mrec is not None:
                    same = same and rec[:, mslots].tobytes() == mrec.tobytes() and \
                        np.array_equal(best["decision"][mslots], dec)
                if r > 0:
                    fused.append(1e3 * (t1 - t0))
                    unfused.append(1e3 * (t3 - t2))
                    kernel.append(k_ms)
                    bridge.append(float(a.value))
                    summary.append(float(b.value))
                    by_index[p].append(1e3 * (t1 - t0))
                if r == reads and p == P - 1:
                    levels, decided = int(info["mapped"].sum()), int(np.count_nonzero(best["decision"]))
        plan = api.last_live_plan()
    return {"slots": S, "levels_mapped_at_end": levels, "decided_at_end": decided,
            "fused_wall_ms": spread(fused), "fused_wall_ms_by_index": [statistics.median(v) for v in by_index],
            "unfused_wall_ms": spread(unfused), "fused_kernel_ms": spread(kernel), "bridge_ms": spread(bridge),
            "summary_ms": spread(summary), "fused_over_unfused": statistics.median(fused) / statistics.median(unfused),
            "arrival_ms": 1e3 * E / 5000.0, "same_records": bool(same), "plan": plan}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="512,3000")
    ap.add_argument("--chunk", type=int, default=2000)
    ap.add_argument("--pushes", type=int, default=10)
    ap.add_argument("--reads", type=int, default=5)
    ap.add_argument("--calib", type=int, default=200)
    ap.add_argument("--target", type=int, default=100000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.ensure_init()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernels_sha import kernels_sha
    ref = np.random.default_rng(20261020).normal(size=a.target)
    targets = [ref, ref[::-1].copy()]
    res = {"tool": "live_throughput", "kernels_sha": kernels_sha(ROOT), "note": "one run on one MI355X",
           "preset": "dna", "chunk": a.chunk, "pushes": a.pushes, "reads": a.reads, "calib": a.calib, "target": a.target,
           "rule": list(RULE),
           "shapes": [shape(L, int(s), a.chunk, a.pushes, a.reads, a.calib, targets) for s in a.slots.split(",")]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
