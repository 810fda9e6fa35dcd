#!/usr/bin/env python3
"""Latency of an HMM session's pushes (csrc/sk_hmmstream.hip): one JSON line, also written to --out
(profiles/hmmstream_throughput.json).  Recorded, not gated.

    python tools/hmmstream_throughput.py [--slots 512,3000] [--chunk 2000] [--pushes 10] [--reads 5] [--out FILE] [--filter]

The sequencer's shape: --slots channels, every one pushed --chunk int16 samples at a time, --pushes pushes per read:
synth.drna_reads of chunk x pushes samples under the synth_raw poly(A) model.  Device resident on both sides
(sk_hmms_push_dev_i16; sk_hmm_viterbi_dev_i16), timed with HIP events around the launches (sk_last_kernel_ms).

per_push_ms   one push of all slots: median, min and max over the pushes of --reads reads after a warm-up read, and the
              median by push index (the first push of a read is fresh: its first sample takes the t == 0 branch)
read_ms       the --pushes pushes of a read, summed (median over the reads)
one_shot_ms   ONE sk_hmm_viterbi_dev_i16 call on the same slots x (chunk x pushes)-sample reads, in the same run
arrival_ms    what a chunk takes to arrive at 5 kHz: the yardstick of a push
plan          the session's slot state in bytes and its guard hits (sk_last_hmms_plan)

--filter      the cost of the filter (SK_HMMS_FILTER) instead, written to profiles/hmmfilter_throughput.json:
              a plain and a filtered session of the same slots in ONE run, pushed alternately with the same chunks (which
              of the two goes first alternates too); per push median [min - max] of both, their ratio, and the
              sk_hmms_filter_dev call over all slots alone.  The filtered session's last filter is checked against ONE
              sk_hmm_posterior_dev_i16 call's loglik and final_post.  Recorded, not gated.

One lane per slot: 512 slots are 8 wavefronts on a device of 256 compute units.  per_push_ms is a LATENCY figure -- how
long a decision waits for its record -- not a throughput figure."""
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
    sig = np.stack(synth.drna_reads(S, 20261020 + S, min_len=n, max_len=n + 1))      # int16 [S, n]
    model = api.polya_model("synth_raw")
    vp = C.c_void_p
    d_sig, d_chunk = L.sk_dev_alloc(S * n * 2), L.sk_dev_alloc(S * E * 2)
    d_slots, d_len, d_full = (L.sk_dev_alloc(S * 4) for _ in range(3))
    d_out, d_rec = L.sk_dev_alloc(S * 96), L.sk_dev_alloc(S * 40)
    slots = np.arange(S, dtype=np.int32)
    for d, a in ((d_sig, sig), (d_slots, slots), (d_len, np.full(S, E, dtype=np.int32)), (d_full, np.full(S, n, dtype=np.int32))):
        _lib.check(L.sk_dev_upload(vp(d), _lib.ptr(a), a.nbytes))
    per_push, by_index, per_read = [], [[] for _ in range(P)], []
    last = np.zeros(S, dtype=api.HMMS_DTYPE)
    with api.HmmStream(model, S) as hs:
        for r in range(reads + 1):                                      # read 0 is the warm-up
            hs.reset(slots)
            total = 0.0
            for p in range(P):
                chunk = np.ascontiguousarray(sig[:, p * E:(p + 1) * E])
                _lib.check(L.sk_dev_upload(vp(d_chunk), _lib.ptr(chunk), chunk.nbytes))
                _lib.check(L.sk_hmms_push_dev_i16(hs.handle, vp(d_slots), S, vp(d_chunk), E, vp(d_len), vp(d_out)))
                dt = main_ms(L)
                total += dt
                if r > 0:
                    per_push.append(dt)
                    by_index[p].append(dt)
            if r > 0:
                per_read.append(total)
        _lib.check(L.sk_dev_download(_lib.ptr(last), vp(d_out), last.nbytes))
        plan = api.last_hmm_stream_plan()
    one = []
    for k in range(reads + 1):
        _lib.check(L.sk_hmm_viterbi_dev_i16(vp(d_sig), n, vp(d_full), S, None, C.byref(model), 0, vp(d_rec)))
        dt = main_ms(L)
        if k > 0:
            one.append(dt)
    rec = np.zeros(S, dtype=api.HMM_DTYPE)
    _lib.check(L.sk_dev_download(_lib.ptr(rec), vp(d_rec), rec.nbytes))
    same = all(last[name].tobytes() == rec[name].tobytes() for name in api.HMM_DTYPE.names)
    found = int(api.polya_segments(rec)["found"].sum())
    for p in (d_sig, d_chunk, d_slots, d_len, d_full, d_out, d_rec):
        L.sk_dev_free(vp(p))
    return {"slots": S, "wavefronts": (S + 63) // 64, "tails_found": found,
            "per_push_ms": spread(per_push), "per_push_ms_by_index": [statistics.median(v) for v in by_index],
            "read_ms": spread(per_read), "one_shot_ms": spread(one),
            "read_over_one_shot": statistics.median(per_read) / statistics.median(one),
            "arrival_ms": 1e3 * E / 5000.0, "same_records_as_one_shot": bool(same), "plan": plan}


def filter_shape(L, S, E, P, reads):
    """a plain and a filtered session side by side: see --filter"""
    n = E * P
    sig = np.stack(synth.drna_reads(S, 20261020 + S, min_len=n, max_len=n + 1))      # int16 [S, n]
    model = api.polya_model("synth_raw")
    vp = C.c_void_p
    d_chunk, d_slots, d_len = L.sk_dev_alloc(S * E * 2), L.sk_dev_alloc(S * 4), L.sk_dev_alloc(S * 4)
    d_out, d_filt = L.sk_dev_alloc(S * 96), L.sk_dev_alloc(S * 64)
    slots = np.arange(S, dtype=np.int32)
    for d, a in ((d_slots, slots), (d_len, np.full(S, E, dtype=np.int32))):
        _lib.check(L.sk_dev_upload(vp(d), _lib.ptr(a), a.nbytes))
    ms = {"plain": [], "filtered": [], "filter_call": []}
    by_index = {"plain": [[] for _ in range(P)], "filtered": [[] for _ in range(P)]}
    rec = {k: np.zeros(S, dtype=api.HMMS_DTYPE) for k in ("plain", "filtered")}
    filt = np.zeros(S, dtype=api.HMMS_FILT_DTYPE)
    with api.HmmStream(model, S) as hp, api.HmmStream(model, S, filter=True) as hf:
        plans = {}
        for r in range(reads + 1):                                      # read 0 is the warm-up
            hp.reset(slots)
            hf.reset(slots)
            for p in range(P):
                chunk = np.ascontiguousarray(sig[:, p * E:(p + 1) * E])
                _lib.check(L.sk_dev_upload(vp(d_chunk), _lib.ptr(chunk), chunk.nbytes))
                order = (("plain", hp), ("filtered", hf)) if (r + p) % 2 == 0 else (("filtered", hf), ("plain", hp))
                for name, hs in order:
                    _lib.check(L.sk_hmms_push_dev_i16(hs.handle, vp(d_slots), S, vp(d_chunk), E, vp(d_len), vp(d_out)))
                    dt = main_ms(L)
                    plans[name] = api.last_hmm_stream_plan()
                    if r > 0:
                        ms[name].append(dt)
                        by_index[name][p].append(dt)
                    if r == reads and p == P - 1:
                        _lib.check(L.sk_dev_download(_lib.ptr(rec[name]), vp(d_out), rec[name].nbytes))
                _lib.check(L.sk_hmms_filter_dev(hf.handle, vp(d_slots), S, vp(d_filt)))
                dt = main_ms(L)
                if r > 0:
                    ms["filter_call"].append(dt)
        _lib.check(L.sk_dev_download(_lib.ptr(filt), vp(d_filt), filt.nbytes))
    post = api.hmm_posterior_batch(sig, None, model)[0]
    same = bool(filt["loglik"].tobytes() == post["loglik"].tobytes() and filt["post"].tobytes() == post["final_post"].tobytes()
                and np.array_equal(filt["n_used"], post["n_used"]) and np.array_equal(filt["flags"], post["flags"]))
    for p in (d_chunk, d_slots, d_len, d_out, d_filt):
        L.sk_dev_free(vp(p))
    mp, mf = statistics.median(ms["plain"]), statistics.median(ms["filtered"])
    return {"slots": S, "wavefronts": (S + 63) // 64,
            "plain_per_push_ms": spread(ms["plain"]), "filtered_per_push_ms": spread(ms["filtered"]),
            "filtered_over_plain": mf / mp, "filter_call_ms": spread(ms["filter_call"]),
            "plain_per_push_ms_by_index": [statistics.median(v) for v in by_index["plain"]],
            "filtered_per_push_ms_by_index": [statistics.median(v) for v in by_index["filtered"]],
            "arrival_ms": 1e3 * E / 5000.0, "filtered_push_over_arrival": mf / (1e3 * E / 5000.0),
            "records_equal_plain": bool(rec["plain"].tobytes() == rec["filtered"].tobytes()),
            "filter_equals_one_shot_posterior": same, "p_transcript_median": float(np.median(filt["post"][:, api.TRANSCRIPT])),
            "plans": plans}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filter", action="store_true", help="a plain and a filtered session side by side (see the head of the file)")
    ap.add_argument("--slots", default="512,3000")
    ap.add_argument("--chunk", type=int, default=2000)
    ap.add_argument("--pushes", type=int, default=10)
    ap.add_argument("--reads", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.ensure_init()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernels_sha import kernels_sha
    one = filter_shape if a.filter else shape
    res = {"tool": "hmmstream_throughput" + (" --filter" if a.filter else ""), "kernels_sha": kernels_sha(ROOT),
           "note": "one run on one MI355X", "preset": "synth_raw", "chunk": a.chunk, "pushes": a.pushes, "reads": a.reads,
           "shapes": [one(L, int(s), a.chunk, a.pushes, a.reads) for s in a.slots.split(",")]}
    line = json.dumps(res)
    print(line)
    if a.filter and not a.out:
        a.out = os.path.join(ROOT, "profiles", "hmmfilter_throughput.json")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
