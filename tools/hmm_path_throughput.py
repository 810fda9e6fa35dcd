#!/usr/bin/env python3
"""Signal-HMM state paths: what the segments call costs beside the record-only call (csrc/sk_hmm.hip): one JSON line.

    python tools/hmm_path_throughput.py [--reads 250000] [--distinct 1000] [--limit 0] [--reps 3] [--ref-reads 2] [--out FILE]

The workload of tools/hmm_throughput.py: device-resident int16 rows, --distinct reads of synth.drna_reads (6 000 .. 30 000
samples) tiled to --reads rows, the "synth_raw" poly(A) model.  After a warm-up, alternated `reps` times over the same
buffers: sk_hmm_viterbi_dev_i16 and sk_hmm_segments_dev_i16.  Seconds per call (median, min, max; wall clock around each
call, which ends in a stream synchronisation), their ratio, the back-pointer scratch the call reserved and its slices, the
segment total and the most segments of a read.  The records of both calls must agree byte for byte, and the segments of
--ref-reads reads are compared with the numpy statement (tests/hmm_path_ref.py).  For the time of each kernel run this
tool under a kernel trace (a run of its own).  Default --out: profiles/hmm_path_throughput.json.
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
import hmm_path_ref                              # noqa: E402

BUDGET_MB = 16384                                # sk_hmm.hip: hmm_bp_budget()


def stats(xs, reads):
    med = statistics.median(xs)
    return {"median_s": med, "ms_per_call": med * 1e3, "min_s": min(xs), "max_s": max(xs), "reads_per_s": reads / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=250000)
    ap.add_argument("--distinct", type=int, default=1000)
    ap.add_argument("--limit", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-reads", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hmm_path_throughput.json"))
    a = ap.parse_args()
    L = _lib.ensure_init()
    NB = max(1, min(a.distinct, a.reads))
    R = a.reads // NB * NB
    M = 30000
    base = synth.drna_reads(NB, synth.SEED_C5 + 7, min_len=6000, max_len=M)
    host = np.zeros((NB, M), dtype=np.int16)
    lens_b = np.zeros(NB, dtype=np.int32)
    for r, x in enumerate(base):
        host[r, :x.size] = x
        lens_b[r] = x.size
    lens = np.tile(lens_b, R // NB)
    cap = 64 * R
    d_sig, d_len, d_rec, d_rec2 = L.sk_dev_alloc(R * M * 2), L.sk_dev_alloc(R * 4), L.sk_dev_alloc(R * 40), L.sk_dev_alloc(R * 40)
    d_off, d_seg = L.sk_dev_alloc((R + 1) * 8), L.sk_dev_alloc(cap * 48)
    bufs = [d_sig, d_len, d_rec, d_rec2, d_off, d_seg]
    assert all(bufs), "device allocation failed"
    _lib.check(L.sk_dev_upload(C.c_void_p(d_len), _lib.ptr(lens), lens.nbytes))
    for k in range(R // NB):
        _lib.check(L.sk_dev_upload(C.c_void_p(d_sig + k * NB * M * 2), _lib.ptr(host), host.nbytes))
    _lib.check(L.sk_sync())
    model = api.polya_model("synth_raw")

    def viterbi():
        _lib.check(L.sk_hmm_viterbi_dev_i16(C.c_void_p(d_sig), M, C.c_void_p(d_len), R, None, C.byref(model), a.limit,
                                            C.c_void_p(d_rec)))
        _lib.check(L.sk_sync())

    def segments():
        _lib.check(L.sk_hmm_segments_dev_i16(C.c_void_p(d_sig), M, C.c_void_p(d_len), R, None, C.byref(model), a.limit,
                                             C.c_void_p(d_rec2), C.c_void_p(d_off), C.c_void_p(d_seg), cap))
        _lib.check(L.sk_sync())

    calls = {"viterbi": viterbi, "segments": segments}
    for f in calls.values():                          # warm-up
        f()
    times = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, f in calls.items():
            t = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t)
    used = np.minimum(lens, a.limit) if a.limit > 0 else lens
    npad = min(M, a.limit) if a.limit > 0 else M
    budget_mb = int(os.environ.get("SK_HMM_SCRATCH_MB", BUDGET_MB))
    groups = (R + 63) // 64
    per_slice = max(1, min(groups, (budget_mb << 20) // (npad * 256)))
    out = {"reads": R, "distinct": NB, "limit": a.limit, "reps": a.reps, "samples_used": int(used.sum()),
           "timing": "wall clock per call, ends in a stream sync",
           "scratch_budget_mb": budget_mb, "scratch_reserved_mb": per_slice * npad * 256 / 2 ** 20,
           "groups": groups, "groups_per_slice": per_slice, "slices": (groups + per_slice - 1) // per_slice}
    for k in calls:
        out[k] = stats(times[k], R)
    out["segments_over_viterbi"] = out["segments"]["median_s"] / out["viterbi"]["median_s"]
    out["segments"]["samples_per_s"] = int(used.sum()) / out["segments"]["median_s"]
    rec, rec2, off = np.zeros(R, dtype=api.HMM_DTYPE), np.zeros(R, dtype=api.HMM_DTYPE), np.zeros(R + 1, dtype=np.int64)
    _lib.check(L.sk_dev_download(_lib.ptr(rec), C.c_void_p(d_rec), rec.nbytes))
    _lib.check(L.sk_dev_download(_lib.ptr(rec2), C.c_void_p(d_rec2), rec2.nbytes))
    _lib.check(L.sk_dev_download(_lib.ptr(off), C.c_void_p(d_off), off.nbytes))
    assert rec.tobytes() == rec2.tobytes(), "the two calls' records differ"
    total = int(off[R])
    assert total <= cap, "more segments than the room of 64 per read"
    out["segments_total"] = total
    out["segments_per_read_max"] = int(np.diff(off).max())
    n = min(a.ref_reads, NB)
    if n > 0:                                         # the numpy statement on the first reads of the same batch
        seg = np.zeros(int(off[n]), dtype=api.HMM_SEG_DTYPE)
        _lib.check(L.sk_dev_download(_lib.ptr(seg), C.c_void_p(d_seg), seg.nbytes))
        want = hmm_path_ref.segments_batch(model, host[:n], lens_b[:n], None, a.limit)
        assert off[:n + 1].tolist() == want[1].tolist() and seg.tobytes() == want[2].tobytes(), "the device differs from hmm_path_ref"
        out["ref_reads"] = n
    for b in bufs:
        L.sk_dev_free(C.c_void_p(b))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
