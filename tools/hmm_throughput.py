#!/usr/bin/env python3
"""Signal-HMM throughput (csrc/sk_hmm.hip): one JSON line.

    python tools/hmm_throughput.py [--reads 250000] [--distinct 1000] [--limit 0] [--reps 3] [--ref-reads 4] [--out FILE]

Device-resident int16 rows: --distinct reads of synth.drna_reads (6 000 .. 30 000 samples: adapter, poly(A), body),
tiled to --reads rows.  After a warm-up, alternated `reps` times over the same buffers: sk_hmm_viterbi_dev_i16 with the
"synth_raw" poly(A) model, and both dRNA_segmenter branches (sk_drna_segment_dev_i16, sk_drna_roll_dev_i16) -- the tools
that approximate the adapter end with thresholds.  Seconds per call (median, min, max; wall clock around each call,
which ends in a stream synchronisation), reads and samples per second, the share of reads with a tail found, and the
ratio hmm / branch of the medians.  The numpy statement (tests/hmm_ref.py) is timed on --ref-reads of the same reads on
one host core, its records compared with the device's on the way; ref_over_hmm is per sample.
Default --out: profiles/hmm_throughput.json.
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
import hmm_ref                                   # noqa: E402


def stats(xs, reads):
    med = statistics.median(xs)
    return {"median_s": med, "ms_per_call": med * 1e3, "min_s": min(xs), "max_s": max(xs), "reads_per_s": reads / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=250000)
    ap.add_argument("--distinct", type=int, default=1000)
    ap.add_argument("--limit", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-reads", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hmm_throughput.json"))
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
    d_sig, d_len, d_rec = L.sk_dev_alloc(R * M * 2), L.sk_dev_alloc(R * 4), L.sk_dev_alloc(R * 40)
    d_segs, d_n, d_xy, d_found = L.sk_dev_alloc(R * 32 * 2 * 4), L.sk_dev_alloc(R * 4), L.sk_dev_alloc(R * 2 * 4), L.sk_dev_alloc(R * 4)
    bufs = [d_sig, d_len, d_rec, d_segs, d_n, d_xy, d_found]
    assert all(bufs), "device allocation failed"
    _lib.check(L.sk_dev_upload(C.c_void_p(d_len), _lib.ptr(lens), lens.nbytes))
    for k in range(R // NB):
        _lib.check(L.sk_dev_upload(C.c_void_p(d_sig + k * NB * M * 2), _lib.ptr(host), host.nbytes))
    _lib.check(L.sk_sync())
    model = api.polya_model("synth_raw")
    dp, rp = _lib.DrnaParams(), _lib.RollParams()

    def hmm():
        _lib.check(L.sk_hmm_viterbi_dev_i16(C.c_void_p(d_sig), M, C.c_void_p(d_len), R, None, C.byref(model), a.limit,
                                            C.c_void_p(d_rec)))
        _lib.check(L.sk_sync())

    def drna_slow5():
        _lib.check(L.sk_drna_segment_dev_i16(C.c_void_p(d_sig), M, C.c_void_p(d_len), R, C.byref(dp), C.c_void_p(d_segs),
                                             C.c_void_p(d_n), 32))
        _lib.check(L.sk_sync())

    def drna_roll():
        _lib.check(L.sk_drna_roll_dev_i16(C.c_void_p(d_sig), M, C.c_void_p(d_len), R, C.byref(rp), C.c_void_p(d_xy),
                                          C.c_void_p(d_found)))
        _lib.check(L.sk_sync())

    calls = {"hmm": hmm, "drna_slow5": drna_slow5, "drna_roll": drna_roll}
    for f in calls.values():                          # warm-up
        f()
    times = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, f in calls.items():
            t = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t)
    used = np.minimum(lens, a.limit) if a.limit > 0 else lens
    out = {"reads": R, "distinct": NB, "limit": a.limit, "reps": a.reps, "samples_used": int(used.sum()),
           "timing": "wall clock per call, ends in a stream sync"}
    for k in calls:
        out[k] = stats(times[k], R)
    out["hmm"]["samples_per_s"] = int(used.sum()) / out["hmm"]["median_s"]
    for k in ("drna_slow5", "drna_roll"):
        out["hmm"]["over_" + k] = out["hmm"]["median_s"] / out[k]["median_s"]
    rec = np.zeros(R, dtype=api.HMM_DTYPE)
    _lib.check(L.sk_dev_download(_lib.ptr(rec), C.c_void_p(d_rec), rec.nbytes))
    out["hmm"]["found_share"] = float(api.polya_segments(rec)["found"].mean())

    # the numpy statement on one host core, on the first reads of the same batch (and a check of the device's records)
    n = min(a.ref_reads, NB)
    if n > 0:
        t = time.perf_counter()
        want = hmm_ref.viterbi_batch(model, host[:n], lens_b[:n], None, a.limit)
        ref_s = time.perf_counter() - t
        assert rec[:n].tobytes() == want.tobytes(), "the device differs from hmm_ref"
        out["hmm"]["ref_reads"] = n
        out["hmm"]["ref_s_per_sample_one_core"] = ref_s / max(1, int(want["n_used"].sum()))
        out["hmm"]["ref_over_hmm"] = out["hmm"]["ref_s_per_sample_one_core"] * out["hmm"]["samples_per_s"]
    for b in bufs:
        L.sk_dev_free(C.c_void_p(b))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
