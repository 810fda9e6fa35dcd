"""squiggle_map --whole: the alignment of the whole read against the matched locus by the adaptive-band DTW.  CPU: the
arguments.  GPU: the table on the golden BLOW5 read and the example model against tests/band_ref.py fed with the same
events, and stdout / --align unchanged by the option."""
import math
import os

import numpy as np
import pytest

import band_ref as br
from conftest import GOLD
from test_cli import run_cli

MODEL = os.path.join(GOLD, "CATCTATCCAGGGTTAAATT.model")
BLOW5 = os.path.join(GOLD, "example_0.blow5")


def test_argument_errors():
    from squigglekit_amd.map_cli import build_parser, main, whole_span
    for argv, msg in ((["--i16", "x.npy", "-m", MODEL, "--whole", "w.tsv", "--band", "100"], "--band must be 64, 128 or 256"),
                      (["--i16", "x.npy", "-m", MODEL, "--whole", "w.tsv", "--band", "0"], "--band must be 64, 128 or 256"),
                      (["--i16", "x.npy", "-m", MODEL, "--band", "64"], "--band needs --whole"),
                      (["--i16", "x.npy", "-m", MODEL, "--whole"], "expected one argument"),
                      (["--i16", "x.npy", "-m", MODEL, "--whole", "w.tsv", "--band", "wide"], "invalid int value")):
        so, se, code = run_cli(main, argv)
        assert code == 2 and msg in se and (so == "" or so.startswith("usage")), (argv, se)
    args = build_parser().parse_args(["--i16", "x.npy", "-m", MODEL, "--whole", "w.tsv"])
    assert args.whole == "w.tsv" and args.band == 128
    # the window: the prefix's points per event scaled to the whole read, half as much again, plus the band; cut at the end
    assert whole_span(10000, 100, 149, 100, 1000, 128) == 750 + 128
    assert whole_span(10000, 100, 149, 30, 1000, 64) == math.ceil(1000 * 50 / 30 * 1.5) + 64 == 2564
    assert whole_span(500, 100, 149, 100, 1000, 128) == 400


@pytest.mark.gpu
@pytest.mark.parametrize("band", (None, 64))
def test_whole_read_table_on_the_golden_read(gpu, tmp_path, band):
    from squigglekit_amd import api
    from squigglekit_amd.blow5 import read_slow5
    from squigglekit_amd.map_cli import ALIGN_HEADER, load_targets, main, zscore
    W = band or 128
    argv = ["--blow5", BLOW5, "-m", MODEL, "--both"]
    plain, se, code = run_cli(main, argv)
    assert code == 0, se
    a0, a1, wt = tmp_path / "a0.tsv", tmp_path / "a1.tsv", tmp_path / "whole.tsv"
    so0, se, code = run_cli(main, argv + ["--align", str(a0)])
    assert code == 0, se
    so1, se1, code = run_cli(main, argv + ["--align", str(a1), "--whole", str(wt)] + (["--band", str(band)] if band else []))
    assert code == 0, se1
    assert so0 == plain and so1 == plain and open(a0).read() == open(a1).read()     # stdout and --align do not change

    targets = load_targets(MODEL, True)
    reads = {r["read_id"]: np.asarray(r["signal"]) for r in read_slow5(BLOW5)}
    lines, notes = ["\t".join(ALIGN_HEADER) + "\n"], 0
    for ln in plain.split("\n")[1:-1]:
        rid, name, strand, start, end, nprefix = ln.split("\t")[:6]
        if name == ".":
            continue
        off, rec = api.detect_events([reads[rid]], api.det_params("dna"))            # the same events the tool sees
        lev = api.event_levels(off, rec)[0]
        assert len(lev) > 1024                                                       # a whole read: past the old limit
        z = zscore(lev)
        y = [t[2] for t in targets if (t[0], t[1]) == (name, strand)][0]
        start, end, nprefix = int(start), int(end), int(nprefix)
        span = min(len(y) - start, int(math.ceil(len(z) * (end - start + 1) / nprefix * 1.5)) + W)
        r = br.band(z, y[start:start + span], W, "free")
        if r["lost"] or r["spans"][0, 0] < 0:
            notes += 1
            continue
        sp = r["spans"] + start
        assert sp[0, 0] == start and sp[-1, 1] == start + r["end"]
        for e in range(len(z)):
            lines.append("{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\n".format(
                rid, name, strand, e, int(rec["start"][e]), int(rec["length"][e]), float(lev[e]), float(z[e]),
                int(sp[e, 0]), int(sp[e, 1])))
    assert open(wt).read() == "".join(lines)
    assert se1.count("whole read:") == notes
    assert len(lines) > 1 or notes
