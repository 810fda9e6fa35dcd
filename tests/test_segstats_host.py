"""CPU: the host side of segment levels -- the record layout, thresholds_of, the --levels writer, and the segmenter
command line with --levels on the CLI goldens' inputs (GPU calls answered by the oracle and numpy)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden
from test_cli import _strip_path, oracle_backend, run_cli, tsv_files   # noqa: F401  (fixtures)

FIELDS = ("mean", "std", "median", "mad", "min", "max", "raw_start", "raw_end", "n", "pad")


def test_level_dtype_matches_the_header():
    from squigglekit_amd import _lib, api
    assert api.LEVEL_DTYPE is _lib.LEVEL_DTYPE
    assert api.LEVEL_DTYPE.itemsize == 64 and ctypes.sizeof(_lib.SegLevel) == 64
    assert api.LEVEL_DTYPE.names == FIELDS == tuple(n for n, _ in _lib.SegLevel._fields_)
    for name in FIELDS:
        assert api.LEVEL_DTYPE.fields[name][1] == getattr(_lib.SegLevel, name).offset
    # the header's own words: the struct, field by field in this order, and the four entry points
    text = open(os.path.join(ROOT, "include", "squigglekit_hip.h")).read()
    body = re.search(r"typedef struct sk_seg_level \{(.*?)\} sk_seg_level;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = re.findall(r"(double|int32_t)\s+(\w+);", body)
    assert [n for _, n in decl] == list(FIELDS)
    assert [t for t, _ in decl] == ["double"] * 6 + ["int32_t"] * 4
    for sym in ("sk_segment_levels_i16", "sk_segment_levels_f64_len", "sk_segment_levels_centi_len",
                "sk_segment_levels_dev_i16"):
        assert sym in _lib.ABI and re.search(r"\b%s\s*\(" % sym, text)
        tail = re.search(r"\b%s\s*\((.*?)\);" % sym, text, flags=re.S).group(1)
        assert re.search(r"sk_seg_level \*\w*levels, sk_seg_level \*\w*read_level$", " ".join(tail.split()))
    lib = ctypes.CDLL(_lib.build())
    assert all(hasattr(lib, s) for s in _lib.ABI if s.startswith("sk_segment_levels_"))


def test_no_levels_and_thresholds_of():
    from squigglekit_amd import _lib, api
    e = api.no_levels((2, 3))
    assert e.shape == (2, 3) and np.all(np.isnan(e["mean"])) and np.all(np.isnan(e["max"]))
    assert np.all(e["raw_start"] == -1) and np.all(e["raw_end"] == -1) and not e["n"].any() and not e["pad"].any()
    rl = api.no_levels(3)
    rl["median"][:2], rl["std"][:2] = [100.0, 0.1], [2.0, 0.3]
    top, bot = api.thresholds_of(rl, _lib.SegParams(std_scale=0.75))
    assert top[0] == 101.5 and bot[0] == 98.5
    # two float64 operations, in the order of segmenter.py:413-414: the product first, then the sum / the difference
    assert top[1] == 0.1 + 0.3 * 0.75 and bot[1] == 0.1 - 0.3 * 0.75
    assert np.isnan(top[2]) and np.isnan(bot[2])
    top, bot = api.thresholds_of(rl[0])                       # one record, default parameters
    assert (float(top), float(bot)) == (101.5, 98.5)


def test_levels_writer_text(tmp_path):
    from squigglekit_amd import _lib, api
    from squigglekit_amd.segmenter_cli import LevelsWriter
    lv = api.no_levels(2)
    lv[0] = (500.25, 1.5, 500.0, 1.0, 498.0, 503.0, 12, 120, 100, 0)
    lv[1] = (1e-05, 0.0, 7.0, 0.0, 7.0, 7.0, 130, 131, 1, 0)
    rl = api.no_levels(1)[0]
    rl["median"], rl["std"] = 480.0, 40.0
    path = str(tmp_path / "levels.tsv")
    w = LevelsWriter(path, _lib.SegParams(std_scale=0.5))
    w.read("a.fast5", [[10, 110], [118, 119]], lv, rl)
    w.read("b.fast5", [], lv, rl)
    w.close()
    assert open(path).read() == (
        "fast5\tseg\tstart\tend\traw_start\traw_end\tlength\tmean\tstdev\tmedian\tmad\tmin\tmax\tread_median\tread_stdev\ttop\tbot\n"
        "a.fast5\t0\t10\t110\t12\t120\t100\t500.25\t1.5\t500.0\t1.0\t498.0\t503.0\t480.0\t40.0\t500.0\t460.0\n"
        "a.fast5\t1\t118\t119\t130\t131\t1\t1e-05\t0.0\t7.0\t0.0\t7.0\t7.0\t480.0\t40.0\t500.0\t460.0\n")


@pytest.fixture
def numpy_levels_backend(oracle_backend, monkeypatch):
    """the levels calls answered by the segmenter fakes of oracle_backend plus plain numpy"""
    from squigglekit_amd import _lib, api

    def records(reads, segs, nsegs, params):
        params = params or _lib.SegParams()
        lv, rl = api.no_levels(segs.shape[:2]), api.no_levels(len(reads))

        def one(w, kept, s):
            m = np.median(w)
            return (np.mean(w), np.std(w), m, np.median(np.abs(w - m)), w.min(), w.max(), kept[s], kept[s + len(w) - 1] + 1,
                    len(w), 0)
        for r, a in enumerate(reads):
            kept = np.flatnonzero((a > params.lim_low) & (a < params.lim_hi))
            y = a[kept]
            if y.size:
                rl[r] = one(y, kept, 0)
            for k in range(nsegs[r]):
                s, e = segs[r, k]
                if len(y[s:e]):
                    lv[r, k] = one(y[s:e], kept, s)
        return lv, rl

    def lev_batch(sig, lens=None, params=None, max_segs=64, devices=None):
        segs, nsegs = api.segment_batch(sig, lens, params, max_segs)
        lens = np.full(len(sig), sig.shape[1]) if lens is None else lens
        return (segs, nsegs) + records([np.asarray(sig[r, :lens[r]]).astype(np.int64) for r in range(len(sig))], segs, nsegs, params)

    def lev_ragged(values, off, lens=None, params=None, max_segs=64, devices=None):
        segs, nsegs = api.segment_ragged_f64(values, off, lens, params, max_segs)
        v = np.asarray(values)
        v = v / 100.0 if v.dtype == np.int32 else v
        reads = [v[off[r]:off[r] + (int(lens[r]) if lens is not None else off[r + 1] - off[r])] for r in range(len(off) - 1)]
        return (segs, nsegs) + records(reads, segs, nsegs, params)

    def lev_any(reads, params=None):
        flat, off = api.pack_f64(reads)
        return lev_ragged(flat, off, None, params)

    monkeypatch.setattr(api, "segment_levels_batch", lev_batch)
    monkeypatch.setattr(api, "segment_levels_ragged_f64", lev_ragged)
    monkeypatch.setattr(api, "segment_levels", lev_any)


def test_segmenter_cli_levels_flag_leaves_the_output_alone(numpy_levels_backend, tsv_files, tmp_path):
    """--levels FILE on every run of the CLI goldens: stdout, stderr and the exit code stay the reference's, byte for
    byte, and FILE holds the header and one well-formed line per printed segment"""
    from squigglekit_amd import api
    from squigglekit_amd.segmenter_cli import build_parser, main
    assert build_parser().parse_args(["-s", "x", "--levels", "out.tsv"]).levels == "out.tsv"
    assert build_parser().parse_args(["-s", "x"]).levels is None
    gold = load_golden("segmenter_cli.json.gz")
    n = lines_seen = 0
    for i, run in enumerate(gold["runs"]):
        if run["tsv"] is None:
            continue
        path = str(tmp_path / ("levels%d.tsv" % i))
        so, se, code = run_cli(main, ["-s", tsv_files[run["tsv"]]] + run["flags"] + ["--levels", path])
        assert so == run["stdout"], (run["tsv"], run["flags"])
        assert code == run["exit"]
        assert _strip_path(se) == _strip_path(run["stderr"]), (run["tsv"], run["flags"])
        n += 1
        if code != 0 and not os.path.exists(path):
            continue
        text = open(path).read().split("\n")
        assert text[0].split("\t") == list(api.LEVELS_HEADER) and text[-1] == ""
        want = []
        for line in so.split("\n"):
            if "\t" in line:
                name, pairs = line.split("\t")
                v = pairs.split(",")
                want += [(name, str(k), v[2 * k], v[2 * k + 1]) for k in range(len(v) // 2)]
        got = [tuple(row.split("\t")[:4]) for row in text[1:-1]]
        assert got == want, (run["tsv"], run["flags"])
        for row in text[1:-1]:
            c = row.split("\t")
            assert len(c) == len(api.LEVELS_HEADER)
            s, e, rs, re_, ln = (int(x) for x in c[2:7])
            assert ln == e - s and rs >= s and re_ - rs >= ln
            mean, sd, med, mad, mn, mx, rmed, rsd, top, bot = (float(x) for x in c[7:])
            assert mn <= med <= mx and mn <= mean <= mx and sd >= 0 and mad >= 0 and bot <= top
            assert bot < med < top or ln <= 2            # a segment lies in the band it was found with
            lines_seen += 1
    assert n >= 20 and lines_seen >= 20
