#!/usr/bin/env python3
"""SquigglePull drop-in throughput (csrc/sk_pull.hip, squigglekit_amd/squigglepull_cli.py): one JSON line.

    python tools/pull_throughput.py [--reads 100000] [--samples 4000] [--out FILE]

kernel      sk_pull_text_dev on R x N device-resident int16 rows (synthetic, seeded), pA and raw: seconds per call
            (median of 5, wall clock around the call, which synchronises twice -- the size read-back and the end),
            GB/s of text, samples/s, and the share of the 8 TB/s HBM peak from the bytes moved (the rows are read by
            both passes, the text written once).
end_to_end  `SquigglePull.py --blow5 FILE` on an R-read BLOW5 file, stdout to /dev/null and to a file in a temporary
            directory: reads/s and GB/s of text, process start to exit.
reference   the reference's per-read work (convert_to_pA_numpy, np.round, map(str), join: SquigglePull.py:185-189,
            238-253) on 1 000 of the reads, scaled to per-read seconds, for the ratio."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from squigglekit_amd import _lib, api, fastio          # noqa: E402

HBM = 8.0e12


def kernel(L, rows, mode):
    R, N = rows.shape
    lens = np.full(R, N, dtype=np.int32)
    calib = np.tile([8192.0, 10.0, 1400.0], (R, 1))
    cal2 = np.zeros((R, 2))
    _lib.check(L.sk_pa_calib(_lib.ptr(calib), R, _lib.ptr(cal2)))
    blob, poff = api.pack_prefixes([b"reads.blow5\tread%d\t" % i for i in range(R)])
    pre = np.frombuffer(blob, dtype=np.uint8)
    cap = len(blob) + 10 * R * N
    d = [L.sk_dev_alloc(n) for n in (rows.nbytes, lens.nbytes, cal2.nbytes, pre.nbytes, poff.nbytes, poff.nbytes, cap)]
    try:
        for p, a in zip(d, (rows, lens, cal2, pre, poff)):
            _lib.check(L.sk_dev_upload(p, _lib.ptr(a), a.nbytes))
        total = C.c_int64(0)
        ts = []
        for _ in range(6):
            _lib.check(L.sk_sync())
            t0 = time.perf_counter()
            _lib.check(L.sk_pull_text_dev(d[0], N, d[1], R, d[2] if mode == _lib.SK_PULL_PA else None, mode, d[3], d[4],
                                          d[6], cap, C.byref(total), d[5]))
            _lib.check(L.sk_sync())
            ts.append(time.perf_counter() - t0)
        t = statistics.median(ts[1:])
    finally:
        for p in d:
            L.sk_dev_free(p)
    moved = 2 * rows.nbytes + total.value
    return {"seconds": t, "text_bytes": total.value, "text_GB_per_s": total.value / t / 1e9, "samples_per_s": R * N / t,
            "bytes_moved": moved, "hbm_share": moved / t / HBM, "calls_s": ts}


def end_to_end(path, R, tmp):
    out = {}
    for name, dest in (("dev_null", os.devnull), ("file", os.path.join(tmp, "out.tsv"))):
        with open(dest, "wb") as fh:
            t0 = time.perf_counter()
            r = subprocess.run([sys.executable, os.path.join(ROOT, "SquigglePull.py"), "--blow5", path], stdout=fh,
                               stderr=subprocess.PIPE, timeout=600)
            t = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError("SquigglePull.py failed: %s" % r.stderr.decode()[-800:])
        size = os.path.getsize(dest) if dest != os.devnull else None
        out[name] = {"seconds": t, "reads_per_s": R / t}
        if size is not None:
            out[name].update({"text_bytes": size, "text_GB_per_s": size / t / 1e9})
            os.unlink(dest)
    return out


def reference(rows, n=1000):
    t0 = time.perf_counter()
    for r in range(n):
        d = np.array([int(v) for v in rows[r]], dtype=int)          # SquigglePull.py:178-179, 185-189
        pa = np.round((d + 10.0) * (1400.0 / 8192.0), 2)
        "reads.blow5\tread\t" + "\t".join(map(str, pa))
    return (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--samples", type=int, default=4000)
    ap.add_argument("--out")
    ap.add_argument("--kernel-only", action="store_true", help="the two kernel measurements only (profiler runs)")
    a = ap.parse_args()
    L = _lib.ensure_init()
    rng = np.random.default_rng(424242)
    rows = (rng.standard_normal((a.reads, a.samples)) * 60 + 480).astype(np.int16)
    rec = {"tool": "pull_throughput", "reads": a.reads, "samples": a.samples,
           "kernel_pA": kernel(L, rows, _lib.SK_PULL_PA), "kernel_raw": kernel(L, rows, _lib.SK_PULL_RAW)}
    if a.kernel_only:
        print(json.dumps(rec))
        return
    with tempfile.TemporaryDirectory() as tmp:
        path = fastio.write_blow5(os.path.join(tmp, "reads.blow5"), rows)
        rec["end_to_end"] = end_to_end(path, a.reads, tmp)
    per_read = reference(rows)
    rec["reference_s_per_read"] = per_read
    rec["reference_reads_per_s"] = 1.0 / per_read
    rec["speedup_end_to_end_file"] = rec["end_to_end"]["file"]["reads_per_s"] * per_read
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
