"""CPU: bench.py's lean default and --dump-outputs.  The records of a "step" come from a host buffer standing in for
device memory (the download is a memmove), so what is written can be checked without a GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_full_is_off_by_default_and_implied_by_the_extra_only_options():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert bench.parse(["--full"]).full
    assert bench.parse(["--only-other-paths"]).full and bench.parse(["--sweep-reads"]).full
    assert bench.parse(["--dump-outputs", "out"]).dump_outputs == "out"


class _HostLib:
    """sk_dev_download over host buffers: a 'device pointer' is the address of a numpy array."""

    def sk_dev_download(self, dst, src, nbytes):
        C.memmove(dst, src, nbytes)
        return 0


class _Step:
    def __init__(self, kind, R, records, segs=None):
        self.L, self.kind, self.R, self.comm = _HostLib(), kind, R, None
        self.rec_bytes = bench.HIT_BYTES if kind == "motifseq" else 4
        self._keep = [records, segs]
        self.d_out = records.ctypes.data
        self.d_segs = segs.ctypes.data if segs is not None else None


def test_motifseq_records_are_dumped_whole_in_float64(tmp_path):
    from squigglekit_amd._lib import HIT_DTYPE
    R = 1000
    rng = np.random.default_rng(1)
    hits = np.zeros(R, dtype=HIT_DTYPE)
    hits["dist"] = rng.random(R) * 100
    hits["start"] = rng.integers(0, 4000, R)
    hits["end"] = hits["start"] + 200
    hits["n"] = 3990
    hits["flags"][::7] = 2
    outs = bench.step_outputs(_Step("motifseq", R, hits), [R])
    names = bench.write_outputs(str(tmp_path), outs)
    assert names == sorted(HIT_DTYPE.names)
    for name in HIT_DTYPE.names:
        got = np.load(tmp_path / (name + ".npy"))
        assert got.dtype == np.float64 and got.shape == (R,)
        assert np.array_equal(got, hits[name].astype(np.float64))
    assert not (tmp_path / "rows.npy").exists()


def test_segmenter_boundaries_past_the_count_are_masked_and_a_large_output_is_sampled(tmp_path):
    R = 5000
    rng = np.random.default_rng(2)
    nsegs = rng.integers(0, bench.MAX_SEGS + 3, R).astype(np.int32)          # counts beyond MAX_SEGS occur too
    segs = rng.integers(-2 ** 31, 2 ** 31 - 1, (R, bench.MAX_SEGS, 2)).astype(np.int32)   # past nsegs: anything
    outs = bench.step_outputs(_Step("segmenter", R, nsegs, segs), [R])
    assert np.array_equal(outs["nsegs"], nsegs)
    for r in range(0, R, 97):
        k = min(int(nsegs[r]), bench.MAX_SEGS)
        assert np.array_equal(outs["segs"][r, :k], segs[r, :k]) and (outs["segs"][r, k:] == -1).all()

    limit = 200_000                                                            # far below the 5000 x 264 B of it
    a, b = tmp_path / "a", tmp_path / "b"
    assert bench.write_outputs(str(a), outs, limit=limit) == ["nsegs", "rows", "segs"]
    bench.write_outputs(str(b), outs, limit=limit)
    assert sum(os.path.getsize(p) for p in a.iterdir()) <= limit
    rows = np.load(a / "rows.npy").astype(np.int64)
    assert len(rows) > 100 and np.all(np.diff(rows) > 0) and rows[-1] < R
    assert np.array_equal(rows, np.load(b / "rows.npy"))                       # the sample is fixed
    assert np.array_equal(np.load(a / "segs.npy"), outs["segs"][rows].astype(np.float64))
    assert np.array_equal(np.load(a / "nsegs.npy"), outs["nsegs"][rows].astype(np.float64))


def test_the_default_c4_outputs_fit_whole():
    """1 M MotifSeq records, five fields in float64: 40 MB, under the 64 MB cap -- no sampling on the headline."""
    assert 1_000_000 * 5 * 8 <= bench.DUMP_BYTES


@pytest.mark.gpu
def test_plain_bench_run_is_lean_and_its_outputs_repeat(gpu, ora, tmp_path):
    """`bench.py --steps K --warmup W --dump-outputs DIR` without --full: the headline line only (no oracle, CPU baseline,
    roofline or extras), exactly K timed steps, and the last step's records -- the same on a second run, and equal to
    the oracle on the generator's reads."""
    import json
    import subprocess
    from squigglekit_amd._lib import HIT_DTYPE
    R = 20000
    runs = []
    for k in range(2):
        out = tmp_path / ("run%d" % k)
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--reads", str(R), "--steps", "3",
               "--warmup", "1", "--dump-outputs", str(out)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = p.stdout.strip().splitlines()
        assert not [ln for ln in lines if ln.startswith('{"extra"')], "extras belong to --full"
        line = json.loads(lines[-1])
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(R / (line["ms_per_step"] * 1e-3), rel=1e-9)
        assert line["unit"] == "reads/s" and line["higher_is_better"] is True and line["dtype"]
        assert not {"roofline", "cpu_baseline", "parity", "extras", "secondary"} & set(line)
        runs.append({name: np.load(out / (name + ".npy")) for name in HIT_DTYPE.names})
    for name in HIT_DTYPE.names:
        assert runs[0][name].dtype == np.float64 and runs[0][name].shape == (R,)
        assert np.array_equal(runs[0][name], runs[1][name], equal_nan=True), name
    # the dumped records are the path's answer: a strided sample of reads, regenerated, against the oracle
    a = bench.parse(["--reads", str(R)])
    w = bench.Workload(a, gpu.load(), 0, 1, R)
    try:
        rows = bench.strided_rows(R, 64)
        sample = bench.download_rows(w.L, w.d_sig, w.stride * 2, rows, np.int16, w.stride)
        want = ora.motifseq_batch_i16(sample, w.lens[rows], w.motif, scale_mode=w.mode)
    finally:
        w.free()
    assert np.array_equal(runs[0]["dist"][rows], want["dist"])
    assert np.array_equal(runs[0]["start"][rows], want["start"]) and np.array_equal(runs[0]["end"][rows], want["end"])
