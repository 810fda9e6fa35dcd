"""GPU: squiggle_map_stream --live --polya_gate.  With --fused (one gated api.LiveMap) it prints what the host gate prints
(HmmStream, polya_decide, EventStream, the ring, MapStream): the same stdout and stderr, byte for byte.  Without
--polya_gate nothing changes: the ungated runs on the same file print the 13 columns they always did."""
import numpy as np
import pytest

import hmmstream_ref as HR

pytestmark = pytest.mark.gpu

NEVER = ["--min_events", "1000000", "--give_up", "1000000"]
GATE = ["--polya_gate", "--gate_preset", "synth_raw", "--min_body", "200", "--gate_margin", "20"]
CASES = {
    "never, 200": ["--sample_chunk", "200"] + NEVER,
    "never, 333, small ring": ["--sample_chunk", "333", "--gate_hold", "4"] + NEVER,
    "accept at once": ["--sample_chunk", "200", "--min_events", "0", "--max_dist_per_event", "1e30", "--min_margin=-1e30"],
    "gate gives up": ["--sample_chunk", "200", "--gate_give_up", "600"] + NEVER,
    "reads end while gating": ["--sample_chunk", "200", "--prefix", "900"] + NEVER,
    "pieces": ["--sample_chunk", "250", "--piece", "60", "--overlap", "20"] + NEVER,
    "locus margin": ["--sample_chunk", "250", "--locus_margin", "--hits", "3", "--min_events", "20", "--max_dist_per_event", "5",
                     "--min_margin", "0.001"],
}


def drna_input(tmp_path):
    from test_gpu_mapstream import synthetic_input
    _, model, _, _ = synthetic_input(tmp_path)
    reads = np.stack([HR.small_drna_read(np.random.default_rng(seed), 1500) for seed in range(6)] +
                     [np.clip(np.rint(np.random.default_rng(6).normal(560, 8, 1500)), 0, 32767).astype(np.int16)])
    path = tmp_path / "drna.npy"
    np.save(path, reads)
    return path, model, reads


@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_prints_what_the_host_gate_prints(gpu, tmp_path, case):
    from squigglekit_amd.mapstream_cli import HEADER, main
    from test_gpu_mapstream import run_cli
    path, model, reads = drna_input(tmp_path)
    base = ["--i16", str(path), "-m", str(model), "--both", "--prefix", "1500", "--calib", "8", "--channels", "3", "--rna",
            "--live"] + GATE + CASES[case]
    want_out, want_err, want_code = run_cli(main, base)
    assert want_code == 0, want_err
    got_out, got_err, got_code = run_cli(main, base + ["--fused"])
    assert got_code == 0, got_err
    assert got_out == want_out and got_err == want_err
    lines = got_out.split("\n")
    assert lines[0] == "\t".join(HEADER + ("transcript_start",)) and len(lines) == 9 and lines[-1] == ""
    rows = [ln.split("\t") for ln in lines[1:-1]]
    assert all(len(r) == 14 for r in rows) and sorted(r[0] for r in rows) == [str(i) for i in range(7)]
    by = {r[0]: r for r in rows}
    assert by["6"][10] == "gate_reject" and by["6"][13] == "-1"        # poly(A)-like noise to the end: the gate never opens
    words = {by[str(i)][10] for i in range(6)}
    starts = [int(by[str(i)][13]) for i in range(6)]
    if case in ("gate gives up", "reads end while gating"):
        assert words == {"gate_reject"} and starts == [-1] * 6
    else:
        assert words == ({"accept"} if case == "accept at once" else {"end"} if "never" in case or case == "pieces" else words)
        assert all(abs(t - 841) <= 35 for t in starts) and "gate_reject" not in words
        assert all(int(by[str(i)][12]) >= 8 for i in range(6))         # events_seen: from the start on, at least --calib


def test_without_the_gate_nothing_changes(gpu, tmp_path):
    from squigglekit_amd.mapstream_cli import HEADER, main
    from test_gpu_mapstream import run_cli
    path, model, reads = drna_input(tmp_path)
    base = ["--i16", str(path), "-m", str(model), "--both", "--prefix", "1500", "--calib", "8", "--channels", "3", "--rna",
            "--live", "--sample_chunk", "200"] + NEVER
    plain_out, plain_err, code = run_cli(main, base)
    assert code == 0, plain_err
    fused_out, fused_err, code = run_cli(main, base + ["--fused"])
    assert code == 0 and fused_out == plain_out and fused_err == plain_err
    lines = plain_out.split("\n")
    assert lines[0] == "\t".join(HEADER) and len(lines) == 9 and all(len(ln.split("\t")) == 13 for ln in lines[:-1])
    # the gated run on the same file maps fewer events per read: the ones before the transcript start are gone
    gated_out, _, code = run_cli(main, base + GATE)
    assert code == 0
    seen = {r.split("\t")[0]: int(r.split("\t")[12]) for r in lines[1:-1]}
    gseen = {r.split("\t")[0]: int(r.split("\t")[12]) for r in gated_out.split("\n")[1:-1]}
    assert all(0 < gseen[str(i)] < seen[str(i)] for i in range(6))


@pytest.mark.parametrize("with_model", [True, False])
def test_a_blow5_files_calibration_pairs_reach_the_gate_under_a_pa_preset(gpu, tmp_path, with_model):
    """The records of a BLOW5 file carry offset 10, range 1400, digitisation 8192: under a pA preset (rna_pa, the default)
    the gate's model sees (raw + 10) * 1400 / 8192, with --gate_model or without.  The reads are small_drna_reads taken
    the other way through that pair, so a model file with the synth_raw numbers finds the planted start only if the pairs
    arrive (under a raw preset they do not, and no gate opens).  Without --gate_model the preset's own pA numbers are far
    off these samples and no gate opens either: that case only shows that the route runs and that both routes agree."""
    from squigglekit_amd import api, fastio
    from squigglekit_amd.mapstream_cli import main
    from test_gpu_mapstream import run_cli, synthetic_input
    _, model, _, _ = synthetic_input(tmp_path)
    unit = 1400.0 / 8192.0
    reads = [np.rint(HR.small_drna_read(np.random.default_rng(seed), 1500) / unit - 10.0).astype(np.int16) for seed in range(4)]
    path = fastio.write_blow5(str(tmp_path / "drna.blow5"), reads, ["r%d" % i for i in range(4)])
    spec = tmp_path / "synth_as_pa.json"
    spec.write_text(api.hmm_spec_to_json(api.polya_spec("synth_raw")))
    base = ["--blow5", path, "-m", str(model), "--both", "--prefix", "1500", "--calib", "8", "--channels", "3", "--rna", "--live",
            "--sample_chunk", "200", "--polya_gate", "--min_body", "200", "--gate_margin", "20"] + NEVER
    if with_model:
        base += ["--gate_model", str(spec)]
    want_out, want_err, code = run_cli(main, base)
    assert code == 0, want_err
    got_out, got_err, code = run_cli(main, base + ["--fused"])
    assert code == 0 and got_out == want_out and got_err == want_err
    rows = {r.split("\t")[0]: r.split("\t") for r in got_out.split("\n")[1:-1]}
    assert sorted(rows) == ["r0", "r1", "r2", "r3"]
    if with_model:
        assert all(abs(int(r[13]) - 841) <= 35 and r[10] == "end" and int(r[12]) >= 8 for r in rows.values()), rows
        # the same file under a raw preset: the pairs stay in the file, the model sees raw values in the thousands
        raw_out, _, code = run_cli(main, base + ["--gate_preset", "synth_raw"])
        assert code == 0 and all(r.split("\t")[10] == "gate_reject" for r in raw_out.split("\n")[1:-1])
    else:
        assert all(r[10] == "gate_reject" and r[13] == "-1" for r in rows.values()), rows
