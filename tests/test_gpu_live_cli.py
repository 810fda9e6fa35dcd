"""GPU: squiggle_map_stream --live --fused against --live: the same stdout and the same stderr, byte for byte -- the lines,
their order, the `.` lines of undecidable reads and their notes -- whether the decision is made on the device (whole
targets) or on the host from the fused session's records and hit lists (--piece, --locus_margin)."""
import pytest

pytestmark = pytest.mark.gpu

NEVER = ["--min_events", "1000000", "--give_up", "1000000"]
CASES = {
    "never, 2000": ["--sample_chunk", "2000"] + NEVER,
    "never, 777": ["--sample_chunk", "777"] + NEVER,
    "accept at once": ["--min_events", "0", "--max_dist_per_event", "1e30", "--min_margin=-1e30"],
    "give up at 74": ["--min_events", "1000000", "--give_up", "74"],
    "pieces": ["--piece", "400", "--overlap", "100"] + NEVER,
    "pieces, deciding": ["--piece", "400", "--overlap", "100", "--min_events", "20", "--max_dist_per_event", "5", "--min_margin", "0"],
    "locus margin": ["--locus_margin", "--hits", "3", "--min_events", "20", "--max_dist_per_event", "5", "--min_margin", "0.001"],
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_prints_what_live_prints(gpu, tmp_path, case):
    from squigglekit_amd import api
    from squigglekit_amd.mapstream_cli import HEADER, main
    from test_gpu_mapstream import run_cli, synthetic_input
    path, model, reads, _ = synthetic_input(tmp_path)
    base = ["--i16", str(path), "-m", str(model), "--both", "--prefix", str(reads.shape[1]), "--calib", "40", "--channels", "3",
            "--live"] + CASES[case]
    want_out, want_err, want_code = run_cli(main, base)
    assert want_code == 0, want_err
    got_out, got_err, got_code = run_cli(main, base + ["--fused"])
    assert got_code == 0, got_err
    assert got_out == want_out and got_err == want_err
    lines = got_out.split("\n")
    assert lines[0] == "\t".join(HEADER) and len(lines) == 10 and lines[-1] == ""
    assert "fewer than 2 events in read 6" in got_err
    words = {ln.split("\t")[10] for ln in lines[1:-1]}
    if case.startswith("never") or case == "pieces":
        assert words == {"end", "."}
    elif case == "accept at once":
        assert words == {"accept", "."}
    elif case == "give up at 74":
        assert "reject" in words and "accept" not in words            # (the read of 1 200 events; the short ones end)
    assert api.last_live_plan()["launches"] >= 2
