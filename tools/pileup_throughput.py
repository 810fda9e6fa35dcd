#!/usr/bin/env python3
"""Throughput of the reference pile-up (csrc/sk_pileup.hip) against the paths call that feeds it and against numpy, in one
run: one JSON line, also written to --out (profiles/pileup_throughput.json).  Recorded, not gated.

    python tools/pileup_throughput.py [--part mapping|locus|both] [--queries 100000] [--target 100000] [--locus 2000]
                                      [--reps 5] [--numpy_reps 5] [--out FILE]

mapping   the mapping workload of tools/pairs_throughput.py: --queries queries of 300 .. 500 points (windows of the
          reference, each point once or twice, with noise) against a --target-point reference and its reversal, best
          target only.  Timed: sk_dtw_pairs_paths_dev on the best pairs (records, then paths), sk_pileup_dev on the spans it
          left on the device, and the numpy statement of the pile-up done with lexsort + reduceat on one host core.
locus     the same queries drawn from one --locus-point target and aligned to it: every list is thousands of entries long,
          so every point takes the merge tier of the ordering step.
Device times are medians of --reps after a warm-up, from the HIP events the library records around its launches
(sk_last_kernel_ms: the main interval); the numpy time is the median of --numpy_reps wall-clock runs after a warm-up.
The job that runs this tool gives each part a time limit of its own."""
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
from squigglekit_amd import _lib, api     # noqa: E402


def main_s(L):
    ms = C.c_float()
    _lib.check(L.sk_last_kernel_ms(None, C.byref(ms)))
    return float(ms.value) / 1e3


def summary(xs):
    return {"median_s": statistics.median(xs), "min_s": min(xs), "max_s": max(xs), "reps": len(xs)}


def numpy_pileup(span_off, spans, value, dwell, target, toff):
    """the pile-up with lexsort + reduceat (the workload of the statement, not its bits)"""
    P = span_off.size - 1
    pair = np.repeat(np.arange(P), np.diff(span_off))
    on = (spans[:, 0] >= 0) & (target[pair] >= 0)
    rows = np.flatnonzero(on)
    lens = (spans[rows, 1] - spans[rows, 0] + 1).astype(np.int64)
    total = int(lens.sum())
    first = np.cumsum(lens) - lens
    ent_row = np.repeat(rows, lens)
    pts = np.repeat(toff[target[pair[rows]]] + spans[rows, 0], lens) + (np.arange(total) - np.repeat(first, lens))
    order = np.lexsort((ent_row, pts))
    pts, ent_row = pts[order], ent_row[order]
    starts = np.flatnonzero(np.concatenate([[True], pts[1:] != pts[:-1]]))
    n = np.diff(np.concatenate([starts, [total]]))
    out = {}
    for name, x in (("level", value[ent_row]), ("dwell", dwell[ent_row].astype(np.float64))):
        mean = np.add.reduceat(x, starts) / n
        out[name] = mean
        out[name + "_sd"] = np.sqrt(np.add.reduceat((x - np.repeat(mean, n)) ** 2, starts) / n)
    out["vmin"], out["vmax"] = np.minimum.reduceat(value[ent_row], starts), np.maximum.reduceat(value[ent_row], starts)
    p = pair[ent_row]
    change = np.concatenate([[True], (p[1:] != p[:-1]) | (pts[1:] != pts[:-1])])
    out["depth"] = np.add.reduceat(change.astype(np.int64), starts)
    out["shared"] = np.add.reduceat((spans[ent_row, 1] > spans[ent_row, 0]).astype(np.int64), starts)
    return total, out


def queries_from(rng, targets, Q):
    lens = rng.integers(300, 501, size=Q)
    out = []
    for n in lens:
        src = targets[int(rng.integers(0, len(targets)))]
        w = int(n) * 2 // 3
        a = int(rng.integers(0, len(src) - w))
        q = np.repeat(src[a:a + w], rng.integers(1, 3, size=w))[:int(n)]
        out.append(q + rng.normal(scale=0.05, size=q.size))
    return out


def part(L, name, targets, Q, reps, numpy_reps):
    rng = np.random.default_rng(5)
    queries = queries_from(rng, targets, Q)
    if len(targets) > 1:
        rec, best = api.map_queries(queries, targets)
    else:
        best = np.zeros(Q, dtype=np.int64)
    values, off = api._as_pool(queries + targets)
    pairs = api._as_pairs(np.stack([np.arange(Q), Q + best], axis=1))
    span_off = api.pair_span_off(off, pairs)
    E = int(span_off[-1])
    dwell = rng.integers(2, 60, size=E).astype(np.int32)
    target = best.astype(np.int32)
    tlen = np.array([len(t) for t in targets], dtype=np.int64)
    toff = np.concatenate([[0], np.cumsum(tlen)])
    mtot = int(toff[-1])
    alloc = lambda n: C.c_void_p(L.sk_dev_alloc(max(int(n), 8)))                                  # noqa: E731
    d_val, d_rec, d_sp = alloc(values.nbytes), alloc(Q * 24), alloc(E * 8)
    d_so, d_dw, d_tg, d_out = alloc(span_off.nbytes), alloc(dwell.nbytes), alloc(target.nbytes), alloc(mtot * 64)
    for d, a in ((d_val, values), (d_so, span_off), (d_dw, dwell), (d_tg, target)):
        _lib.check(L.sk_dev_upload(d, _lib.ptr(a), a.nbytes))

    def paths():
        _lib.check(L.sk_dtw_pairs_paths_dev(d_val, _lib.ptr(off), off.size - 1, _lib.ptr(pairs), Q, 0, d_rec, 0, d_sp))
        _lib.check(L.sk_sync())

    def pile():                                                     # value: the queries lie first in the pool, in pair order
        _lib.check(L.sk_pileup_dev(d_so, d_sp, d_val, d_dw, d_tg, None, None, Q, E, _lib.ptr(tlen), tlen.size, d_out,
                                   None, None, 0))
        _lib.check(L.sk_sync())

    times = {"paths": [], "pileup": []}
    paths(), pile()
    for _ in range(reps):
        paths()
        times["paths"].append(main_s(L))
        pile()
        times["pileup"].append(main_s(L))
    plan = api.last_pileup_plan()
    spans = np.zeros((E, 2), dtype=np.int32)
    _lib.check(L.sk_dev_download(_lib.ptr(spans), d_sp, spans.nbytes))
    got = np.zeros(mtot, dtype=api.PILE_DTYPE)
    _lib.check(L.sk_dev_download(_lib.ptr(got), d_out, got.nbytes))
    for d in (d_val, d_rec, d_sp, d_so, d_dw, d_tg, d_out):
        L.sk_dev_free(d)
    numpy_s = []
    for k in range(numpy_reps + 1):                                 # (the first run warms the allocator up)
        t0 = time.perf_counter()
        total, ref = numpy_pileup(span_off, spans, values[:E], dwell, target, toff)
        if k:
            numpy_s.append(time.perf_counter() - t0)
    covered = got["n"] > 0
    assert total == plan["entries"] and np.array_equal(got["depth"][covered], ref["depth"])
    assert np.allclose(got["level"][covered], ref["level"], rtol=1e-9, atol=1e-12)
    res = {"queries": Q, "targets": [int(x) for x in tlen], "rows": E, "plan": plan,
           "depth_median": float(np.median(got["depth"][covered])), "depth_max": int(got["depth"].max()),
           "paths_dev": summary(times["paths"]), "pileup_dev": summary(times["pileup"]), "numpy_one_core": summary(numpy_s)}
    res["pileup_over_paths"] = res["pileup_dev"]["median_s"] / res["paths_dev"]["median_s"]
    res["numpy_over_pileup"] = res["numpy_one_core"]["median_s"] / res["pileup_dev"]["median_s"]
    res["entries_per_s"] = plan["entries"] / res["pileup_dev"]["median_s"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("mapping", "locus", "both"), default="both")
    ap.add_argument("--queries", type=int, default=100000)
    ap.add_argument("--target", type=int, default=100000)
    ap.add_argument("--locus", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--numpy_reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.ensure_init()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernels_sha import kernels_sha
    res = {"tool": "pileup_throughput", "kernels_sha": kernels_sha(ROOT)}
    if a.out and os.path.exists(a.out):                             # the parts may be run one at a time into one file
        try:
            old = json.loads(open(a.out).read())
            if old.get("kernels_sha") == res["kernels_sha"]:
                res.update({k: old[k] for k in ("mapping", "locus") if k in old})
        except ValueError:
            pass
    rng = np.random.default_rng(4)
    if a.part in ("mapping", "both"):
        ref = rng.normal(size=a.target)
        res["mapping"] = part(L, "mapping", [ref, np.ascontiguousarray(ref[::-1])], a.queries, a.reps, a.numpy_reps)
    if a.part in ("locus", "both"):
        res["locus"] = part(L, "locus", [np.random.default_rng(6).normal(size=a.locus)], a.queries, a.reps, a.numpy_reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
