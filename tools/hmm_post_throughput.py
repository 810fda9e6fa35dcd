#!/usr/bin/env python3
"""Signal-HMM posteriors: what forward-backward costs beside the Viterbi call (csrc/sk_hmm_post.hip): one JSON line.

    python tools/hmm_post_throughput.py [--reads 250000] [--distinct 1000] [--limit 0] [--reps 3] [--ref-reads 2] [--out FILE]

The workload of tools/hmm_throughput.py: device-resident int16 rows, --distinct reads of synth.drna_reads (6 000 .. 30 000
samples) tiled to --reads rows, the "synth_raw" poly(A) model.  After a warm-up, alternated `reps` times over the same
buffers: sk_hmm_viterbi_dev_i16, sk_hmm_posterior_dev_i16 without counts and with counts (no dense rows: at 48 bytes a
sample they are for small calls).  Seconds per call (median, min, max; wall clock around each call, which ends in a
stream synchronisation), the ratios to the Viterbi call, the scratch the call reserved and its slices.  The records of
the two posterior calls must agree byte for byte, and records and counts of --ref-reads reads (cut to --ref-limit samples
in a call of their own) are compared with the numpy statement (tests/hmm_post_ref.py).  Default --out:
profiles/hmm_post_throughput.json.
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
import hmm_post_ref                              # noqa: E402

BUDGET_MB = 16384                                # sk_hmm_post.hip: post_budget()


def stats(xs, reads, samples):
    med = statistics.median(xs)
    return {"median_s": med, "ms_per_call": med * 1e3, "min_s": min(xs), "max_s": max(xs), "reads_per_s": reads / med,
            "samples_per_s": samples / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=250000)
    ap.add_argument("--distinct", type=int, default=1000)
    ap.add_argument("--limit", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-reads", type=int, default=2)
    ap.add_argument("--ref-limit", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hmm_post_throughput.json"))
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
    sizes = (R * M * 2, R * 4, R * 40, R * 112, R * 112, R * 624)
    bufs = [L.sk_dev_alloc(n) for n in sizes]
    assert all(bufs), "device allocation failed"
    d_sig, d_len, d_rec, d_post, d_post2, d_cnt = bufs
    _lib.check(L.sk_dev_upload(C.c_void_p(d_len), _lib.ptr(lens), lens.nbytes))
    for k in range(R // NB):
        _lib.check(L.sk_dev_upload(C.c_void_p(d_sig + k * NB * M * 2), _lib.ptr(host), host.nbytes))
    _lib.check(L.sk_sync())
    model = api.polya_model("synth_raw")

    def viterbi():
        _lib.check(L.sk_hmm_viterbi_dev_i16(C.c_void_p(d_sig), M, C.c_void_p(d_len), R, None, C.byref(model), a.limit,
                                            C.c_void_p(d_rec)))
        _lib.check(L.sk_sync())

    def posterior(d_out, d_counts):
        _lib.check(L.sk_hmm_posterior_dev_i16(C.c_void_p(d_sig), M, C.c_void_p(d_len), R, None, C.byref(model), a.limit,
                                              C.c_void_p(d_out), C.c_void_p(d_counts) if d_counts else None, None, None))
        _lib.check(L.sk_sync())

    calls = {"viterbi": viterbi, "posterior": lambda: posterior(d_post, None), "posterior_counts": lambda: posterior(d_post2, d_cnt)}
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
    block = int(os.environ.get("SK_HMM_POST_BLOCK", 128))
    groups = (R + 63) // 64
    per_group = 512 + (-(-npad // block) + block) * 3072
    per_slice = max(1, min(groups, (budget_mb << 20) // per_group))
    out = {"reads": R, "distinct": NB, "limit": a.limit, "reps": a.reps, "samples_used": int(used.sum()),
           "timing": "wall clock per call, ends in a stream sync", "block": block,
           "scratch_budget_mb": budget_mb, "scratch_reserved_mb": per_slice * per_group / 2 ** 20,
           "groups": groups, "groups_per_slice": per_slice, "slices": (groups + per_slice - 1) // per_slice}
    for k in calls:
        out[k] = stats(times[k], R, int(used.sum()))
    out["posterior_over_viterbi"] = out["posterior"]["median_s"] / out["viterbi"]["median_s"]
    out["posterior_counts_over_viterbi"] = out["posterior_counts"]["median_s"] / out["viterbi"]["median_s"]
    post, post2 = np.zeros(R, dtype=api.HMM_POST_DTYPE), np.zeros(R, dtype=api.HMM_POST_DTYPE)
    cnt = np.zeros(R, dtype=api.HMM_COUNTS_DTYPE)
    for dst, src in ((post, d_post), (post2, d_post2), (cnt, d_cnt)):
        _lib.check(L.sk_dev_download(_lib.ptr(dst), C.c_void_p(src), dst.nbytes))
    assert post.tobytes() == post2.tobytes(), "the records with and without counts differ"
    assert (post["flags"] == 0).all() and not np.isnan(post["occ"]).any() and not np.isnan(cnt["xi"]).any()
    out["occ_minus_n_max"] = float(np.abs(post["occ"].sum(axis=1) - used).max())
    out["p_transcript_above_half_share"] = float((post["final_post"][:, api.TRANSCRIPT] > 0.5).mean())
    out["loglik_per_sample_mean"] = float((post["loglik"] / np.maximum(used, 1)).mean())
    n = min(a.ref_reads, NB)
    if n > 0:                                         # the numpy statement on the first reads, cut to --ref-limit samples
        lim = a.ref_limit if a.limit == 0 else min(a.limit, a.ref_limit)
        _lib.check(L.sk_hmm_posterior_dev_i16(C.c_void_p(d_sig), M, C.c_void_p(d_len), n, None, C.byref(model), lim,
                                              C.c_void_p(d_post), C.c_void_p(d_cnt), None, None))
        _lib.check(L.sk_sync())
        _lib.check(L.sk_dev_download(_lib.ptr(post[:n]), C.c_void_p(d_post), n * 112))
        _lib.check(L.sk_dev_download(_lib.ptr(cnt[:n]), C.c_void_p(d_cnt), n * 624))
        want = hmm_post_ref.posterior_batch(model, host[:n], lens_b[:n], None, lim, dense=False)
        assert post[:n].tobytes() == want[0].tobytes() and cnt[:n].tobytes() == want[1].tobytes(), "the device differs from hmm_post_ref"
        out["ref_reads"], out["ref_limit"] = n, lim
    for b in bufs:
        L.sk_dev_free(C.c_void_p(b))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
