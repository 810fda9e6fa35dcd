#!/usr/bin/env python3
"""Latency of a GATED live mapping session's pushes (csrc/sk_livegate.hip) beside an ungated one on the same samples: one
JSON line, also written to --out (profiles/livegate_throughput.json).  Recorded, not gated: nothing here is a criterion.

    python tools/livegate_throughput.py [--slots 512,3000] [--chunk 2000] [--pushes 10] [--reads 5] [--calib 200]
                                        [--target 100000] [--hold 1024] [--out FILE]

tools/live_throughput.py's shape on direct-RNA-like reads (synth.drna_reads, --chunk * --pushes samples of each): --slots
channels, every one pushed --chunk int16 samples at a time, the rna preset, END with the last push, the synth_raw poly(A)
model with min_body 2 000 and margin 20.  The gated and the ungated push alternate in one run, per push of all slots
(medians over the pushes of --reads reads after a warm-up read, with min and max):

gated_wall_ms / ungated_wall_ms   wall time of one host-form api.LiveMap.push with the device rule
gated_kernel_ms / ungated_kernel_ms   sk_last_kernel_ms of the push (event cutting to summary)
hmm_ms      the HMM side of the gated push by HIP events of its own: the chunk lengths and k_hmms_push -- it shrinks as
            slots leave GATING (by_index shows it per push of a read)
gate_ms     k_live_gate and the scan of the released counts, likewise
gated_over_ungated   median wall / median wall"""
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
GATE = (2000, 20.0)                               # min_body, min_margin


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def shape(L, S, E, P, reads, Cal, hold, targets):
    n = E * P
    raw = synth.drna_reads(S, 20261021 + S, min_len=n, max_len=n + 1)
    sig = np.stack([r[:n] for r in raw])                                # int16 [S, n]
    params = api.det_params("rna")
    slots = np.arange(S, dtype=np.int32)
    rule = api.live_rule(*RULE)
    gate = api.live_gate(api.polya_model("synth_raw"), GATE[0], GATE[1], hold=hold)
    flags = [np.zeros(S, dtype=np.int32), np.ones(S, dtype=np.int32)]
    wall = {"gated": [], "ungated": []}
    kern = {"gated": [], "ungated": []}
    hmm, gms = [], []
    hmm_by, gating_by = [[] for _ in range(P)], [0] * P
    a, b = C.c_float(0), C.c_float(0)
    opened = mapped = 0
    with api.LiveMap(params, Cal, targets, S, gate=gate) as lg, api.LiveMap(params, Cal, targets, S) as lu:
        for r in range(reads + 1):                                      # read 0 is the warm-up
            lg.reset(slots)
            lu.reset(slots)
            for p in range(P):
                chunk = np.ascontiguousarray(sig[:, p * E:(p + 1) * E])
                end = flags[p == P - 1]
                lens = np.full(S, E, dtype=np.int32)
                for name, lm in (("gated", lg), ("ungated", lu)) if (r + p) % 2 == 0 else (("ungated", lu), ("gated", lg)):
                    t0 = time.perf_counter()
                    res = lm.push(slots, (chunk, lens), end=end, rule=rule)
                    t1 = time.perf_counter()
                    _lib.check(L.sk_last_kernel_ms(C.byref(a), C.byref(b)))
                    if r > 0:
                        wall[name].append(1e3 * (t1 - t0))
                        kern[name].append(float(b.value))
                    if name == "gated":
                        _lib.check(L.sk_live_gate_last_ms(lm.handle, C.byref(a), C.byref(b)))
                        if r > 0:
                            hmm.append(float(a.value))
                            gms.append(float(b.value))
                            hmm_by[p].append(float(a.value))
                        if r == reads:
                            g = lm.gate()[0]
                            gating_by[p] = int(np.count_nonzero(g["state"] == _lib.SK_LIVE_GATE_GATING))
                            if p == P - 1:
                                opened, mapped = int(np.count_nonzero(g["state"] == _lib.SK_LIVE_GATE_OPEN)), int(res[1]["mapped"].sum())
        plan = api.last_live_plan()
    return {"slots": S, "gates_open_at_end": opened, "levels_mapped_at_end": mapped, "gating_after_push": gating_by,
            "gated_wall_ms": spread(wall["gated"]), "ungated_wall_ms": spread(wall["ungated"]),
            "gated_kernel_ms": spread(kern["gated"]), "ungated_kernel_ms": spread(kern["ungated"]),
            "hmm_ms": spread(hmm), "hmm_ms_by_index": [statistics.median(v) for v in hmm_by], "gate_ms": spread(gms),
            "gated_over_ungated": statistics.median(wall["gated"]) / statistics.median(wall["ungated"]),
            "arrival_ms": 1e3 * E / 5000.0, "plan_of_the_last_push": plan}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="512,3000")
    ap.add_argument("--chunk", type=int, default=2000)
    ap.add_argument("--pushes", type=int, default=10)
    ap.add_argument("--reads", type=int, default=5)
    ap.add_argument("--calib", type=int, default=200)
    ap.add_argument("--target", type=int, default=100000)
    ap.add_argument("--hold", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.ensure_init()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernels_sha import kernels_sha
    ref = np.random.default_rng(20261021).normal(size=a.target)
    targets = [ref, ref[::-1].copy()]
    res = {"tool": "livegate_throughput", "kernels_sha": kernels_sha(ROOT), "note": "one run on one MI355X",
           "preset": "rna", "model": "synth_raw", "gate": list(GATE), "hold": a.hold, "chunk": a.chunk, "pushes": a.pushes,
           "reads": a.reads, "calib": a.calib, "target": a.target, "rule": list(RULE),
           "shapes": [shape(L, int(s), a.chunk, a.pushes, a.reads, a.calib, a.hold, targets) for s in a.slots.split(",")]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
