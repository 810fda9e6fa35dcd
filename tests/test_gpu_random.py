"""GPU leg of the seeded random cases (tests/randcases.py): every committed seed of the four newest kernel files --
segmenter sweep (sk_sweep.hip), MotifSeq hit lists (sk_hits.hip + k_sdtw's row output), alignment paths (sk_path.hip),
SquigglePull text (sk_pull.hip) -- through the public api call, against its reference, exactly; and one interleaved
sequence of calls over the shared grow-only context buffers.  tests/test_random_cases.py (CPU) asserts what the seeds
reach; tests/RANDOM_CASES.md lists the one-line kernel mutants these tests catch.  A failure names family, seed, the
drawn parameters and switches, and the first differing (read, hit / set / line): `randcases.case_of(family, seed)`
rebuilds the case on any machine."""
import numpy as np
import pytest

import randcases as rc
import test_gpu_hits
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
    if fam in ("hits", "paths", "motifseq"):
        guard = api.last_dtw_guard()
        assert guard["premise_violations"] == 0 and guard["audit_mismatches"] == 0, (rc.describe(case), guard)
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


def test_interleaved_calls_share_the_context_buffers(gpu, ora, monkeypatch):
    """The context's buffers are grow-only and shared between routes (sk_reserve): a fixed sequence of calls that mixes the
    four families with segment_batch, motifseq_batch and segment_batch_pa, sizes going up and down.  Every call is checked
    against its reference, and a call that occurs twice returns the same bytes both times."""
    seen = {}
    for step, (fam, seed) in enumerate(rc.INTERLEAVE):
        case = rc.interleave_case(fam, seed)
        try:
            got, _ = run_case(monkeypatch, ora, case)
        except AssertionError as e:
            raise AssertionError("step %d of the interleaved sequence (after %s): %s" % (step, rc.INTERLEAVE[:step][-3:], e))
        b = rc.result_bytes(got)
        if (fam, seed) in seen:
            assert b == seen[fam, seed][1], "step %d: %s differs from the same call at step %d" % (
                step, rc.describe(case), seen[fam, seed][0])
        else:
            seen[fam, seed] = (step, b)
    assert len(seen) < len(rc.INTERLEAVE)
