"""CPU: the segmenter parameter sweep's host side -- struct layouts, exported symbols, the refusal without a device, the
grid order and range parsing of segmenter_sweep.py, and its table against the reference's golden line counts with
api.segment_sweep answered by the oracle (a loop over get_segs + test_segs, as test_cli.py fakes the GPU calls)."""
import contextlib
import ctypes
import hashlib
import io
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import GOLD, ROOT, load_golden


# ------------------------------------------------------------------ layouts and symbols
def test_sweep_struct_layouts():
    from squigglekit_amd import _lib
    assert ctypes.sizeof(_lib.SweepSet) == 48 and ctypes.sizeof(_lib.SweepRec) == 24 and ctypes.sizeof(_lib.SweepSum) == 64
    assert _lib.SweepSet.seg.offset == 0 and _lib.SweepSet.stall_start.offset == 40 and _lib.SweepSet.gap_dist.offset == 44
    for cls, dt in ((_lib.SweepRec, _lib.SWEEP_REC_DTYPE), (_lib.SweepSum, _lib.SWEEP_SUM_DTYPE)):
        assert ctypes.sizeof(cls) == dt.itemsize
        for name, _ in cls._fields_:
            assert getattr(cls, name).offset == dt.fields[name][1], name
    s = _lib.SweepSet()
    assert (s.seg.window, s.stall_start, s.gap_dist) == (150, 300, 3000)


def test_sweep_symbols_exported():
    from squigglekit_amd import _lib
    _lib.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in ("sk_segment_sweep_i16", "sk_segment_sweep_dev_i16", "sk_segment_sweep_f64"):
        assert hasattr(lib, name) and name in _lib.ABI


def test_sweep_refused_without_a_device():
    """A fresh process that never bound a GPU: the entry point answers SK_ERR_NO_DEVICE, it computes nothing."""
    code = r"""
import sys, ctypes, numpy as np
sys.path.insert(0, %r)
from squigglekit_amd import _lib, api
L = _lib.load()
sig = np.full((2, 64), 500, dtype=np.int16); lens = np.full(2, 64, dtype=np.int32)
sets = (_lib.SweepSet * 1)(api.sweep_set())
sums = np.zeros(1, dtype=_lib.SWEEP_SUM_DTYPE)
print(L.sk_segment_sweep_i16(_lib.ptr(sig), 64, _lib.ptr(lens), 2, sets, 1, _lib.ptr(sums), None))
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert int(out.stdout.strip().splitlines()[-1]) == -2            # SK_ERR_NO_DEVICE


def test_negative_corrector_is_named():
    from squigglekit_amd import api
    sets = api.sweep_grid(corrector=[5, -1])
    with pytest.raises(ValueError, match="set 1"):
        api.segment_sweep(np.zeros((1, 64), dtype=np.int16), sets)


# ------------------------------------------------------------------ grid order and parsing
def test_sweep_grid_order():
    from squigglekit_amd import api
    g = api.sweep_grid(error=[1, 2], window=[100, 200], gap_dist=[5, 6])
    vals = [api.sweep_values(s) for s in g]
    assert len(vals) == 8
    assert [(v[0], v[2], v[9]) for v in vals] == [(e, w, b) for e in (1, 2) for w in (100, 200) for b in (5, 6)]
    assert vals[0][1] == 50 and vals[0][4] == 0.75 and vals[0][8] == 300           # the rest: segmenter.py's defaults


def test_range_parsing():
    from squigglekit_amd.sweep_cli import parse_values
    assert parse_values("0.5:1.0:0.1", "std_scale") == [0.5, 0.6, 0.7, 0.8, 0.9, 1.0]
    assert parse_values("100:150:25,7", "window") == [100, 125, 150, 7]
    assert parse_values("10:0:-5", "error") == [10, 5, 0]
    assert parse_values("3", "seg_dist") == [3]
    for bad in ("1:2", "a", "1:5:0", "5:1:1", "1.5"):
        with pytest.raises(ValueError):
            parse_values(bad, "window")


def test_grid_file_partial_columns(tmp_path):
    from squigglekit_amd import api
    from squigglekit_amd.sweep_cli import build_parser, build_sets
    f = tmp_path / "grid.tsv"
    f.write_text("window\tstd_scale\n100\t0.5\n200\t1.25\n")
    args = build_parser().parse_args(["-s", "x", "--grid", str(f), "-e", "3,4"])
    vals = [api.sweep_values(s) for s in build_sets(args)]
    assert [(v[0], v[2], v[4]) for v in vals] == [(3, 100, 0.5), (4, 100, 0.5), (3, 200, 1.25), (4, 200, 1.25)]
    assert all(v[1] == 50 and v[9] == 3000 for v in vals)


def _run(main, argv):
    so, se = io.StringIO(), io.StringIO()
    code = 0
    with contextlib.redirect_stdout(so), contextlib.redirect_stderr(se):
        try:
            main(argv)
        except SystemExit as e:
            code = e.code
    return so.getvalue(), se.getvalue(), code


@pytest.mark.parametrize("argv", [["-s", "x", "-w", "1:"], ["-s", "x", "-e", "x"], ["-s", "x", "-w", "5:1:1"],
                                  ["-s", "x", "-c", "-1"], []])
def test_cli_errors_exit_2(argv, tmp_path):
    from squigglekit_amd.sweep_cli import main
    so, se, code = _run(main, argv)
    assert code == 2 and se.startswith("error: ")


def test_cli_empty_grid_file(tmp_path):
    from squigglekit_amd.sweep_cli import main
    f = tmp_path / "g.tsv"
    f.write_text("window\n")
    so, se, code = _run(main, ["-s", "x", "--grid", str(f)])
    assert code == 2 and "empty grid" in se


# ------------------------------------------------------------------ the table against the golden runs
@pytest.fixture
def oracle_sweep(monkeypatch, ora):
    """api.segment_sweep answered by the oracle's get_segs and api.test_segs, read by read and set by set."""
    from squigglekit_amd import _lib, api

    def sweep(reads, sets, lens=None, records=False, devices=None):
        sums = np.zeros(len(sets), dtype=_lib.SWEEP_SUM_DTYPE)
        recs = np.zeros((len(sets), len(reads)), dtype=_lib.SWEEP_REC_DTYPE)
        for k, s in enumerate(sets):
            g = s.seg
            op = ora.SegParams(g.error, g.corrector, g.window, g.seg_dist, g.std_scale, g.stall_len)
            for r, sig in enumerate(reads):
                segs = ora.get_segs(ora.scale_outliers(np.asarray(sig, float), g.lim_low, g.lim_hi), op) or []
                rec = recs[k, r]
                rec["nsegs"] = len(segs)
                rec["s0_start"], rec["s0_end"] = segs[0] if segs else (-1, -1)
                rec["s1_start"], rec["s1_end"] = segs[1] if len(segs) > 1 else (-1, -1)
                m = sums[k]
                m["reads"] += 1
                m["segs"] += len(segs)
                if not segs:
                    continue
                m["with_segs"] += 1
                m["seg0_end_sum"] += segs[0][1]
                ok = {}
                for name, stall, gap in (("stall_ok", True, False), ("gap_ok", False, True), ("stall_gap_ok", True, True)):
                    a = types.SimpleNamespace(stall=stall, gap=gap, stall_start=s.stall_start, gap_dist=s.gap_dist)
                    ok[name] = bool(api.test_segs([list(x) for x in segs], a, err=io.StringIO()))
                    m[name] += ok[name]
        return sums, (recs if records else None)
    monkeypatch.setattr(api, "segment_sweep", sweep)
    monkeypatch.setattr(_lib, "init", lambda device=None: 0)
    monkeypatch.setattr(_lib, "warm_start", lambda device=None, also=(): None)


@pytest.fixture(scope="module")
def golden_tsvs(tmp_path_factory, example_read):
    """The golden runs' TSV inputs, rebuilt the way tools/gen_golden.py made them."""
    from squigglekit_amd import synth
    from squigglekit_amd.blow5 import to_pA
    d = tmp_path_factory.mktemp("sweep_tsv")
    rec = example_read
    raw = rec["signal"]
    pa = to_pA(raw, rec["digitisation"], rec["offset"], rec["range"])
    texts = {"pA_noinfo": "\t".join(["test.fast5", rec["read_id"]] + [str(v) for v in pa]) + "\n",
             "raw_noinfo": "\t".join(["test.fast5", rec["read_id"]] + [str(v) for v in raw]) + "\n"}
    syn = synth.squiggle_batch(256, 4000, synth.SEED_C2)
    assert hashlib.sha256(syn[:8].tobytes()).hexdigest() == load_golden("segmenter_cli.json.gz")["synthetic8_sha256"]
    lines = []
    for r in range(8):
        vals = syn[r]
        if r == 3:
            vals = np.zeros(50, dtype=np.int16)
        if r == 5:
            vals = np.full(800, 500, dtype=np.int16)
        lines.append("\t".join(["read%d.fast5" % r, "id%d" % r, "x", "y"] + [str(int(v)) for v in vals]) + "\n")
    texts["synthetic8"] = "".join(lines)
    out = {}
    for k, t in texts.items():
        p = d / (k + ".tsv")
        p.write_text(t)
        out[k] = str(p)
    return out


def _table(text):
    lines = text.strip("\n").split("\n")
    head = lines[0].split("\t")
    return [dict(zip(head, ln.split("\t"))) for ln in lines[1:]]


def _golden_lines(tsv, flags):
    for run in load_golden("segmenter_cli.json.gz")["runs"]:
        if run["tsv"] == tsv and run["flags"] == flags:
            return len(run["stdout"].splitlines())
    raise KeyError((tsv, flags))


@pytest.mark.parametrize("tsv", ["pA_noinfo", "raw_noinfo", "synthetic8"])
def test_cli_table_matches_golden_line_counts(oracle_sweep, golden_tsvs, tsv, tmp_path):
    from squigglekit_amd.sweep_cli import main
    names = tmp_path / "names.txt"
    recs = tmp_path / "recs.npy"
    so, se, code = _run(main, ["-s", golden_tsvs[tsv], "-j", "100,300", "-b", "100,3000", "--records", str(recs),
                               "--names", str(names)])
    assert code in (0, None), se
    rows = _table(so)
    assert len(rows) == 4
    by = {(r["stall_start"], r["gap_dist"]): r for r in rows}
    assert int(by[("300", "3000")]["with_segs"]) == _golden_lines(tsv, [])
    assert int(by[("100", "3000")]["stall_ok"]) == _golden_lines(tsv, ["-ku", "-j", "100"])
    assert int(by[("300", "100")]["stall_gap_ok"]) == _golden_lines(tsv, ["-k", "-g", "-u", "-b", "100"])
    nreads = len(names.read_text().splitlines())
    assert all(int(r["reads"]) == nreads for r in rows)
    assert np.load(recs).shape == (4, nreads)
    # error >= corrector: the per-sample walk's set
    so, se, code = _run(main, ["-s", golden_tsvs[tsv], "-e", "10", "-c", "0", "-w", "100"])
    (row,) = _table(so)
    assert int(row["with_segs"]) == _golden_lines(tsv, ["-e", "10", "-c", "0", "-w", "100"])
    m = row["seg0_end_mean"]
    assert m == "nan" if int(row["with_segs"]) == 0 else float(m) >= 0
