#!/usr/bin/env python3
"""MotifSeq panel throughput (csrc/sk_panel.hip): writes profiles/panel_throughput.json and prints it as one JSON line.

    python tools/panel_throughput.py [--reads 100000] [--samples 4000] [--region 0:2000] [--motifs 12,96] [--points 163]
                                     [--reps 5] [--out FILE]

Device-resident int16 rows (sk_synth_squiggles_dev, seeded), K motifs of `points` points each.  Three calls, alternated
`reps` times after one warm-up round of each, wall clock around each call ending in sk_sync():
    panel     sk_motifseq_panel_dev_i16 over the region (gather, statistics over the window, one grid per shape group,
              ranking on the device)
    whole     baseline (a): sk_motifseq_multi_dev_i16 over the whole reads, records brought home, ranked in numpy
    windows   baseline (b): the same entry point over window rows gathered beforehand (not timed), ranked in numpy
Per call: median / min / max seconds, the spread (max - min) / median, reads per second.  `panel_vs_whole` and
`panel_vs_windows` are ratios of medians; `windows_gain_exceeds_spread` says whether the panel's gain over (b) is larger
than the larger of the two run-to-run spreads.  The panel's records are compared with (b)'s on the way (same slice, so
the same bits)."""
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
from squigglekit_amd import _lib, synth          # noqa: E402


def summary(xs, reads):
    med = statistics.median(xs)
    return {"median_s": med, "min_s": min(xs), "max_s": max(xs), "spread": (max(xs) - min(xs)) / med,
            "reads_per_s": reads / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--samples", type=int, default=4000)
    ap.add_argument("--region", default="0:2000")
    ap.add_argument("--motifs", default="12,96")
    ap.add_argument("--points", type=int, default=163)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panel_throughput.json"))
    a = ap.parse_args()
    begin, end = (int(x) for x in a.region.split(":"))
    R, M, W = a.reads, a.samples, end - begin
    _lib.init()
    L = _lib.load()
    check, ptr = _lib.check, _lib.ptr
    name = C.create_string_buffer(128)
    L.sk_device_name(name, 128)

    d_sig = L.sk_dev_alloc(R * M * 2)
    d_len = L.sk_dev_alloc(R * 4)
    d_win = L.sk_dev_alloc(R * W * 2)
    d_wlen = L.sk_dev_alloc(R * 4)
    base = synth.synthetic_motif(a.points)
    check(L.sk_synth_squiggles_dev(d_sig, M, R, M, 20260, ptr(base), base.size))
    lens = np.full(R, M, dtype=np.int32)
    check(L.sk_dev_upload(d_len, ptr(lens), lens.nbytes))
    # window rows for baseline (b): gathered on the host once, outside the timed calls
    sig = np.empty((R, M), dtype=np.int16)
    check(L.sk_dev_download(ptr(sig), d_sig, sig.nbytes))
    wrows = np.ascontiguousarray(sig[:, begin:end])
    wlens = np.full(R, W, dtype=np.int32)
    check(L.sk_dev_upload(d_win, ptr(wrows), wrows.nbytes))
    check(L.sk_dev_upload(d_wlen, ptr(wlens), wlens.nbytes))
    del sig, wrows

    result = {"tool": "panel_throughput", "device": name.value.decode(), "reads": R, "samples": M, "region": [begin, end],
              "points": a.points, "reps": a.reps, "cases": []}
    for K in [int(x) for x in a.motifs.split(",")]:
        motifs = [base] + [synth.synthetic_motif(a.points, seed=100 + k) for k in range(1, K)]
        flat = np.ascontiguousarray(np.concatenate(motifs))
        moff = (np.arange(K + 1) * a.points).astype(np.int32)
        mean = np.full(K, 2.90 * a.points - 9.6)
        sd = mean * 0.08468
        d_out = L.sk_dev_alloc(R * 48)
        d_all = L.sk_dev_alloc(K * R * 24)
        rec = np.zeros((K, R), dtype=_lib.HIT_DTYPE)
        pan = np.zeros(R, dtype=_lib.PANEL_DTYPE)

        def rank_host():
            check(L.sk_dev_download(ptr(rec), d_all, rec.nbytes))
            z = (rec["dist"] - mean[:, None]) / sd[:, None]
            return np.argmin(z, axis=0)

        def panel():
            check(L.sk_motifseq_panel_dev_i16(d_sig, M, d_len, R, begin, end, None, ptr(flat), ptr(moff), K, ptr(mean),
                                              ptr(sd), 0, 0, 1200, d_out, None, d_all))
            check(L.sk_sync())
            check(L.sk_dev_download(ptr(pan), d_out, pan.nbytes))

        def whole():
            check(L.sk_motifseq_multi_dev_i16(d_sig, M, d_len, R, ptr(flat), ptr(moff), K, 0, 0, 1200, d_all))
            check(L.sk_sync())
            return rank_host()

        def windows():
            check(L.sk_motifseq_multi_dev_i16(d_win, W, d_wlen, R, ptr(flat), ptr(moff), K, 0, 0, 1200, d_all))
            check(L.sk_sync())
            return rank_host()

        calls = {"panel": panel, "whole": whole, "windows": windows}
        times = {n: [] for n in calls}
        for n, f in calls.items():                                    # warm-up: every shape the timed window uses
            f()
        best_b = windows()
        rec_b = rec.copy()
        panel()
        check(L.sk_dev_download(ptr(rec), d_all, rec.nbytes))
        same = bool(rec.tobytes() == rec_b.tobytes() and np.array_equal(pan["best"], best_b))
        for _ in range(a.reps):
            for n, f in calls.items():
                t0 = time.perf_counter()
                f()
                times[n].append(time.perf_counter() - t0)
        case = {"motifs": K, "panel_equals_windows_baseline": same}
        for n in calls:
            case[n] = summary(times[n], R)
        case["panel_vs_whole"] = case["whole"]["median_s"] / case["panel"]["median_s"]
        case["panel_vs_windows"] = case["windows"]["median_s"] / case["panel"]["median_s"]
        case["windows_gain_exceeds_spread"] = bool(
            case["windows"]["median_s"] - case["panel"]["median_s"] >
            max(case["panel"]["max_s"] - case["panel"]["min_s"], case["windows"]["max_s"] - case["windows"]["min_s"]))
        result["cases"].append(case)
        L.sk_dev_free(d_out)
        L.sk_dev_free(d_all)
    for p in (d_sig, d_len, d_win, d_wlen):
        L.sk_dev_free(p)
    text = json.dumps(result)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")
    print(text)


if __name__ == "__main__":
    main()
