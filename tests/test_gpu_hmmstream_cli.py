"""GPU: dRNA_polya_stream.py (squigglekit_amd/polya_stream_cli.py), the replay of a file through an HMM session, against
dRNA_polya.py on the same input and against the numpy replay of tests/hmmstream_ref.py."""
import os

import numpy as np
import pytest

import hmmstream_ref as HR
from test_gpu_mapstream import run_cli

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    """(reads.npy, reads int16 [6, 2400]): six shrunk direct-RNA reads in the synth_raw preset's units"""
    rng = np.random.default_rng(20261021)
    reads = np.stack([HR.small_drna_read(rng, 2400) for _ in range(6)])
    path = tmp_path_factory.mktemp("hmmstream") / "reads.npy"
    np.save(path, reads)
    return str(path), reads


def table(text):
    lines = text.split("\n")
    assert lines[-1] == ""
    rows = [ln.split("\t") for ln in lines[:-1]]
    assert len({r[0] for r in rows}) == len(rows)
    return {r[0]: r for r in rows}


@pytest.mark.parametrize("source, chunk", [("blow5", 2000), ("i16", 2000), ("i16", 777)])
def test_reads_that_run_to_their_end_print_the_lines_of_the_one_shot_tool(gpu, synthetic, source, chunk):
    """--give_up 0 (never) and a --min_body above any read length: every read prints `end`, its first seven columns are
    dRNA_polya.py's line byte for byte, samples_seen is its length and pushes ceil(length / sample_chunk)"""
    from squigglekit_amd.polya_cli import main as polya_main
    from squigglekit_amd.polya_stream_cli import main as stream_main
    base = ["-f", os.path.join(GOLD, "example_0.blow5")] if source == "blow5" else ["--i16", synthetic[0], "--preset", "synth_raw"]
    want, err, code = run_cli(polya_main, base)
    assert code == 0, err[-300:]
    got, err, code = run_cli(stream_main, base + ["--sample_chunk", str(chunk), "--channels", "4", "--give_up", "0",
                                                  "--min_body", "1000000000"])
    assert code == 0, err[-300:]
    want, got = table(want), table(got)
    assert sorted(got) == sorted(want) and len(got) >= 1
    for rid, cols in got.items():
        assert len(cols) == 10 and cols[:7] == want[rid], (rid, cols, want[rid])
        n = int(cols[9])
        assert cols[7] == "end" and n > 0 and int(cols[8]) == -(-n // chunk), (rid, cols)
    if source == "i16":
        assert all(int(got[str(r)][9]) == synthetic[1].shape[1] for r in range(6))
        assert all(c[3] != "." for c in got.values())                   # a tail was found in every synthetic read
    else:
        from squigglekit_amd.blow5 import read_slow5
        assert [int(got[r["read_id"]][9]) for r in read_slow5(base[1])] == [len(r["signal"]) for r in read_slow5(base[1])]


def test_reads_are_accepted_before_their_end(gpu, synthetic):
    """a small --min_body: the numpy replay accepts every synthetic read, at least one before its samples run out, and
    the tool prints the replay's lines"""
    from squigglekit_amd import api
    from squigglekit_amd.polya_cli import polya_lines
    from squigglekit_amd.polya_stream_cli import main as stream_main
    path, reads = synthetic
    chunk, body, margin = 300, 150, 10.0
    model = api.polya_model("synth_raw")
    want = {}
    for r, x in enumerate(reads):                                        # the replay in numpy: one slot per read
        ref = HR.Session(model, 1)
        for at in range(0, len(x), chunk):
            rec = ref.push([0], [x[at:at + chunk]], "i16")
            if api.polya_decide(rec, body, margin, 0)[0] == 1:
                break
        assert api.polya_decide(rec, body, margin, 0)[0] == 1, (r, rec)   # the reads were chosen so: all accepted
        want[str(r)] = polya_lines([str(r)], rec)[0].rstrip("\n").split("\t") + ["accept", str(int(rec["pushes"][0])),
                                                                                  str(int(rec["n_used"][0]))]
    assert any(int(w[9]) < reads.shape[1] for w in want.values())        # ... and before the end
    got, err, code = run_cli(stream_main, ["--i16", path, "--preset", "synth_raw", "--sample_chunk", str(chunk), "--channels", "4",
                                           "--min_body", str(body), "--min_margin", str(margin)])
    assert code == 0, err[-300:]
    assert table(got) == want
