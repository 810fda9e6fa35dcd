"""GPU leg of the seeded random cases (tests/randcases.py): every committed seed -- segmenter sweep (sk_sweep.hip),
MotifSeq hit lists (sk_hits.hip + k_sdtw's row output), alignment paths (sk_path.hip), SquigglePull text (sk_pull.hip),
the region + motif panel (sk_panel.hip), event detection (sk_detect.hip), the signal HMM and its state paths
(sk_hmm.hip), segment levels (sk_seglev.hip), the read background (sk_bg.hip) and events (sk_events.hip) twins of the
hit family, and the switches of the screening scheme (sk_sdtwq.hip) -- through the public api call, against its reference, exactly; and two interleaved sequences of calls over
the shared grow-only context buffers.  tests/test_random_cases.py (CPU) asserts what the seeds
reach; tests/RANDOM_CASES.md lists the one-line kernel mutants these tests catch.  A failure names family, seed, the
drawn parameters and switches, and the first differing (read, hit / set / line): `randcases.case_of(family, seed)`
rebuilds the case on any machine."""
import numpy as np
import pytest

import randcases as rc
import test_gpu_hits
import test_gpu_panel
import test_gpu_paths

pytestmark = pytest.mark.gpu


def run_case(monkeypatch, ora, case):
    """One case through the GPU and its reference; returns (result, expectation).  Fails with the case's description."""
    from squigglekit_amd import api
    for key in rc.SWITCHES:
        if key in case["env"]:
            monkeypatch.setenv(key, case["env"][key])
        else:
            monkeypatch.delenv(key, raising=False)
    fam = case["family"]
    exp = rc.EXPECT[fam](ora, case)
    got = rc.CALL[fam](api, case, exp)
    msg = rc.DIFF[fam](case, got, exp)
    assert msg is None, "%s\n  first difference: %s" % (rc.describe(case), msg)
    if fam in ("hits", "paths", "motifseq", "background", "events", "screen"):
        guard = api.last_dtw_guard()
        assert guard["premise_violations"] == 0 and guard["audit_mismatches"] == 0, (rc.describe(case), guard)
    if fam == "screen":                                      # every motif of the call took the screening scheme, no alarm
        import ctypes as C
        from squigglekit_amd import _lib
        launches = C.c_int32()
        _lib.load().sk_last_dtw_profile(None, C.byref(launches), None, None, None)
        assert launches.value >= 1 and guard["alarm"] == 0 and guard["exact_fallback"] == 0, (rc.describe(case), guard)
    if fam == "paths":
        assert api.last_path_mismatches() == 0, rc.describe(case)
    return got, exp


@pytest.mark.parametrize("seed", rc.SEEDS["sweep"])
def test_sweep_seed_matches_the_oracle(gpu, ora, monkeypatch, seed):
    case = rc.case_of("sweep", seed)
    (sums, recs), exp = run_case(monkeypatch, ora, case)
    assert recs.tobytes() == exp["recs"].tobytes() and sums.tobytes() == exp["sums"].tobytes(), rc.describe(case)
    from squigglekit_amd import api                          # without records: the same summaries
    sums_only, none = (api.segment_sweep(case["sig"], [api.sweep_set(**s) for s in case["sets"]], case["lens"])
                       if case["form"] == "batch" else
                       api.segment_sweep(case["reads"], [api.sweep_set(**s) for s in case["sets"]]))
    assert none is None and sums_only.tobytes() == exp["sums"].tobytes(), rc.describe(case)


@pytest.mark.parametrize("seed", rc.SEEDS["hits"])
def test_hits_seed_matches_the_reference(gpu, ora, monkeypatch, seed):
    case = rc.case_of("hits", seed)
    got, exp = run_case(monkeypatch, ora, case)
    for m, want in enumerate(exp["want"]):                  # the existing helper's comparison, as it stands
        test_gpu_hits.same(got[m], want, "%s motif %d" % (rc.describe(case), m))


@pytest.mark.parametrize("seed", rc.SEEDS["paths"])
def test_paths_seed_matches_the_reference(gpu, ora, monkeypatch, seed):
    from squigglekit_amd import api
    case = rc.case_of("paths", seed)
    got, exp = run_case(monkeypatch, ora, case)
    for m, want in enumerate(exp["want"]):
        test_gpu_paths.same(got[m], want, "%s motif %d" % (rc.describe(case), m))
    plain = rc.call_hits(api, dict(case, family="hits"), exp)      # the records are the hit-list call's, byte for byte
    test_gpu_paths.same_as_hit_lists(got, plain)


@pytest.mark.parametrize("seed", rc.SEEDS["pull"])
def test_pull_seed_matches_numpy(gpu, ora, monkeypatch, seed):
    case = rc.case_of("pull", seed)
    text, exp = run_case(monkeypatch, ora, case)
    assert bytes(text) == exp["text"], rc.describe(case)
    other = dict(case, entry="dev" if case["entry"] == "host" else "host")      # the other entry point: the same bytes
    run_case(monkeypatch, ora, other)


@pytest.mark.parametrize("seed", rc.SEEDS["panel"])
def test_panel_seed_matches_the_reference(gpu, ora, monkeypatch, seed):
    import ctypes as C
    from squigglekit_amd import api
    case = rc.case_of("panel", seed)
    got, exp = run_case(monkeypatch, ora, case)
    if rc.panel_screened(case):                              # the long windows over 256 reads went to the screening path
        launches = C.c_int32()
        gpu.load().sk_last_dtw_profile(None, C.byref(launches), None, None, None)
        assert launches.value >= 1, rc.describe(case)
    test_gpu_panel.same(got, exp["ref"], rc.describe(case))  # the existing helper's comparison, as it stands
    if rc.panel_screened(case):                              # ... and the one-grid exact kernel gives the same bytes
        monkeypatch.setenv("SK_PANEL_EXACT", "1")
        exact = rc.call_panel(api, case, exp)
        assert rc.result_bytes(exact) == rc.result_bytes(got), rc.describe(case)
        test_gpu_panel.same(exact, exp["ref"], rc.describe(case) + " SK_PANEL_EXACT=1")


@pytest.mark.parametrize("seed", rc.SEEDS["detect"])
def test_detect_seed_matches_the_definition(gpu, ora, monkeypatch, seed):
    case = rc.case_of("detect", seed)
    (off, rec), exp = run_case(monkeypatch, ora, case)
    assert off.tobytes() == exp["off"].tobytes() and rec.tobytes() == exp["rec"].tobytes(), rc.describe(case)


@pytest.mark.parametrize("seed", rc.SEEDS["hmm"])
def test_hmm_seed_matches_the_definition(gpu, ora, monkeypatch, seed):
    """The record call and the segments call on the same case: records and segments byte for byte, the segments call's
    records the record call's, and the definition's invariants on what the GPU returned."""
    import hmm_path_ref
    case = rc.case_of("hmm", seed)
    (rec, prec, segs), exp = run_case(monkeypatch, ora, case)
    assert rec.tobytes() == exp["rec"].tobytes() and prec.tobytes() == rec.tobytes(), rc.describe(case)
    for idx, _, woff, wseg in exp["parts"]:
        off = np.concatenate([[0], np.cumsum([len(segs[r]) for r in idx])]).astype(np.int64)
        seg = np.concatenate([segs[r] for r in idx]) if idx else wseg
        assert off.tobytes() == woff.tobytes() and seg.tobytes() == wseg.tobytes(), rc.describe(case)
        hmm_path_ref.invariants(case["model"], prec[idx], off, seg)


@pytest.mark.parametrize("seed", rc.SEEDS["levels"])
def test_levels_seed_matches_numpy(gpu, ora, monkeypatch, seed):
    from squigglekit_amd import api
    from squigglekit_amd._lib import SegParams
    case = rc.case_of("levels", seed)
    (segs, nsegs, levels, read_level), exp = run_case(monkeypatch, ora, case)
    assert [segs[r, :nsegs[r]].tolist() for r in range(case["R"])] == exp["segs"], rc.describe(case)
    p = SegParams(**case["seg"])                             # the segments are the plain segmenter call's, on every route
    if case["route"] == "list":
        plain = [list(map(list, g or [])) for g in api.segment_any(case["reads"], p)]
    else:
        if case["route"] == "batch":
            sg, n = api.segment_batch(case["sig"], case["lens"], p, max_segs=segs.shape[1])
        elif case["route"] == "batch_pa":
            sg, n = api.segment_batch_pa(case["sig"], case["lens"], case["calib"], p, max_segs=segs.shape[1])
        else:
            sg, n = api.segment_ragged_f64(*api.pack_f64(case["reads"]), None, p, max_segs=segs.shape[1])
        plain = [sg[r, :n[r]].tolist() for r in range(case["R"])]
    assert plain == [segs[r, :nsegs[r]].tolist() for r in range(case["R"])], rc.describe(case)
    if "max_segs" in case:                                   # the call began with the drawn number of columns and grew
        assert segs.shape[1] >= max(case["max_segs"], int(nsegs.max())), rc.describe(case)


@pytest.mark.parametrize("seed", rc.SEEDS["screen"])
def test_screen_seed_matches_the_oracle(gpu, ora, monkeypatch, seed):
    """One int16 first-match call through the screening scheme under drawn switches (lane layout, hint, checkpoint
    distance, sorted order, chunks, fused or separate statistics, siblings, early retry, scaling, limits, stride, one to
    three motifs): every record the oracle's, byte for byte; chunks and retries as the case's plan says."""
    import ctypes as C
    case = rc.case_of("screen", seed)
    got, exp = run_case(monkeypatch, ora, case)
    L = gpu.load()
    launches, per = C.c_int32(), C.c_int32()
    L.sk_last_dtw_profile(None, C.byref(launches), None, None, C.byref(per))
    assert launches.value == rc.screen_plan(case)[-1]["chunks"], (rc.describe(case), launches.value, per.value)
    # (the counters of a call add up over its motifs) fewer than a quarter of the (read, motif) pairs took the exact retry
    assert 4 * L.sk_last_dtw_retries() < case["R"] * len(case["Ns"]), (rc.describe(case), L.sk_last_dtw_retries())
    for g, want in zip(got, exp["want"]):
        ok = rc.screen_compared(g, want)
        assert np.array_equal(g["n"], want["n"]) and 10 * int((~ok).sum()) < case["R"], rc.describe(case)
    if any(p["hinted"] for p in rc.screen_plan(case)):       # the hint changes which columns a window computes, never a record
        from squigglekit_amd import api
        monkeypatch.setenv("SK_DTW_NOHINT", "1")
        assert rc.result_bytes(rc.call_screen(api, case)) == rc.result_bytes(got), rc.describe(case) + " SK_DTW_NOHINT=1"


@pytest.mark.parametrize("seed", rc.SEEDS["hits"])
def test_background_twin_of_the_hits_seed(gpu, ora, monkeypatch, seed):
    """Every committed hit-list case through api.motifseq_background: the records against numpy on the oracle's last row,
    the hit lists the hit-list call's bytes."""
    run_case(monkeypatch, ora, rc.interleave_case("background", seed))


@pytest.mark.parametrize("seed", rc.SEEDS["paths"])
def test_events_twin_of_the_paths_seed(gpu, ora, monkeypatch, seed):
    """Every committed paths case through api.motifseq_events and api.pool_events (a drawn `use` mask): records and pooled
    model against the numpy statement, the hit lists the hit-list call's bytes."""
    run_case(monkeypatch, ora, rc.interleave_case("events", seed))


def run_sequence(monkeypatch, ora, seq):
    seen = {}
    for step, (fam, seed) in enumerate(seq):
        case = rc.interleave_case(fam, seed)
        try:
            got, _ = run_case(monkeypatch, ora, case)
        except AssertionError as e:
            raise AssertionError("step %d of the interleaved sequence (after %s): %s" % (step, seq[:step][-3:], e))
        b = rc.result_bytes(got)
        if (fam, seed) in seen:
            assert b == seen[fam, seed][1], "step %d: %s differs from the same call at step %d" % (
                step, rc.describe(case), seen[fam, seed][0])
        else:
            seen[fam, seed] = (step, b)
    assert len(seen) < len(seq)


def test_interleaved_calls_share_the_context_buffers(gpu, ora, monkeypatch):
    """The context's buffers are grow-only and shared between routes (sk_reserve): a fixed sequence of calls that mixes the
    four families with segment_batch, motifseq_batch and segment_batch_pa, sizes going up and down.  Every call is checked
    against its reference, and a call that occurs twice returns the same bytes both times."""
    run_sequence(monkeypatch, ora, rc.INTERLEAVE)


def test_newer_calls_interleaved_with_the_older_ones(gpu, ora, monkeypatch):
    """The same for the panel, event detection, the signal HMM, segment levels and the two twins, between calls of the
    older families (c->sig / len / off / out / out2 / misc / comp / prep are shared through sk_reserve); at the end three
    screening calls, whose checkpoint, last-row and state buffers are used again after calls of other families."""
    run_sequence(monkeypatch, ora, rc.INTERLEAVE2)
