"""GPU leg of the seeded random cases (tests/randcases.py): every committed seed -- segmenter sweep (sk_sweep.hip),
MotifSeq hit lists (sk_hits.hip + k_sdtw's row output), alignment paths (sk_path.hip), SquigglePull text (sk_pull.hip),
the region + motif panel (sk_panel.hip), event detection (sk_detect.hip), the signal HMM and its state paths
(sk_hmm.hip), segment levels (sk_seglev.hip), the read background (sk_bg.hip) and events (sk_events.hip) twins of the
hit family, the switches of the screening scheme (sk_sdtwq.hip), and both branches of the dRNA segmenter (sk_drna_walk.hip,
k_drna_stats / k_roll_* of sk_prep.hip; host and device entry points), DTW over a pair list (sk_pairs.hip, k_sdtw's
MODE_PAIRS / MODE_PAIRS_GLOBAL) and its warping paths (sk_pairpath.hip; host and device entry points) -- through the public
api call, against its reference, exactly; the adaptive-band DTW (sk_band.hip; host and device entry points) likewise; the
signal HMM's posteriors (sk_hmm_post.hip; host and device entry points) against tests/hmm_post_ref.py bit for bit, each case
also through a filtered HMM session (sk_hmmstream.hip); and six interleaved sequences of calls over the shared grow-only
context buffers.
tests/test_random_cases.py (CPU) asserts what the seeds
reach; tests/RANDOM_CASES.md (tests/RANDOM_CASES_BAND.md for the band, tests/RANDOM_CASES_HMMPOST.md for the posteriors) lists the one-line kernel mutants these tests
catch.  A failure names family, seed, the
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
    if fam in ("pairs", "pairpaths"):                        # no screening scheme: the counters read zeros, whatever ran before
        guard = api.last_dtw_guard()
        assert not any(guard.values()), (rc.describe(case), guard)
    if fam == "band":
        if case["paths"]:                                    # lost corners and failed walks, no other pair
            assert got[3] == exp["mismatches"] >= exp["lost"], (rc.describe(case), got[3], exp["mismatches"])
        if "SK_BAND_WAVES" in case["env"]:
            assert api.last_band_plan()[1] <= int(case["env"]["SK_BAND_WAVES"]), (rc.describe(case), api.last_band_plan())
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


def same_under(monkeypatch, ora, case, got, switches):
    """The case again under each (switch, value): every record the oracle's still, and the bytes the first call's."""
    for key, val in switches:
        again, _ = run_case(monkeypatch, ora, dict(case, env=dict(case["env"], **{key: val})))
        assert rc.result_bytes(again) == rc.result_bytes(got), "%s %s=%s" % (rc.describe(case), key, val)


@pytest.mark.parametrize("seed", rc.SEEDS["drna"])
def test_drna_seed_matches_the_oracle(gpu, ora, monkeypatch, seed):
    """dRNA_segmenter's slow5 branch on a drawn case (read count, lengths, route and stride, limits, statistics window,
    std_scale, the scan's five parameters; two-level reads whose band mask is a drawn or crafted bit pattern): every segment
    of every read the oracle's.  Then under SK_DRNA_STEP=1 -- k_prep_i16 for the statistics and the per-sample scan
    k_drna_walk whatever w is -- the same bytes."""
    case = rc.case_of("drna", seed)
    got, exp = run_case(monkeypatch, ora, case)
    assert got == exp["segs"], rc.describe(case)
    same_under(monkeypatch, ora, case, got, [("SK_DRNA_STEP", "1")])


@pytest.mark.parametrize("seed", rc.SEEDS["roll"])
def test_roll_seed_matches_the_oracle(gpu, ora, monkeypatch, seed):
    """The --signal branch on a drawn case: (x, y) or None per read as the oracle has them, no read left out; then
    k_roll_one for every read, every read through the redo list, the two-kernel path and the per-sample scan: the same bytes."""
    case = rc.case_of("roll", seed)
    got, exp = run_case(monkeypatch, ora, case)
    assert got == exp["xy"], rc.describe(case)
    same_under(monkeypatch, ora, case, got, [("SK_ROLL_ONE_LOOK", "1"), ("SK_ROLL_DELTA_SCALE", "1e13"),
                                             ("SK_ROLL_TWO_KERNELS", "1"), ("SK_DRNA_STEP", "1")])


def _rows_of(case):
    """(sig [R, stride], lens) as the case's route hands them to the C entry point."""
    from squigglekit_amd import api
    if case["route"] == "list":
        return api.pack_i16(case["reads"])
    return np.ascontiguousarray(case["sig"]), np.ascontiguousarray(case["lens"])


class DevBuffers:
    """Device buffers for one call of a device entry point: uploaded arrays and outputs with a guard area behind them."""
    GUARD = 256

    def __init__(self, L):
        self.L, self.ptrs = L, []

    def up(self, a):
        from squigglekit_amd import _lib
        d = self.L.sk_dev_alloc(max(a.nbytes, 8))
        self.ptrs.append(d)
        _lib.check(self.L.sk_dev_upload(d, _lib.ptr(a), a.nbytes))
        return d

    def out(self, nbytes):
        return self.up(np.full(nbytes + self.GUARD, 0x5A, dtype=np.uint8))

    def inout(self, a):
        """an input the call may also write: its bytes, then the guard area"""
        guard = np.full(self.GUARD, 0x5A, dtype=np.uint8)
        return self.up(np.concatenate([np.frombuffer(a.tobytes(), dtype=np.uint8), guard]))

    def down(self, d, shape, dtype):
        from squigglekit_amd import _lib
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        raw = np.zeros(n + self.GUARD, dtype=np.uint8)
        _lib.check(self.L.sk_dev_download(_lib.ptr(raw), d, raw.nbytes))
        assert np.all(raw[n:] == 0x5A), "bytes written behind the output"
        return raw[:n].view(dtype).reshape(shape)

    def free(self):
        for d in self.ptrs:
            self.L.sk_dev_free(d)


# one-look statistics + scan by runs | k_prep_i16 (LDS need past the gate) | one-look + the per-sample scan (w = 63); and
# the case with 46 segments in a read for the call that is given too few columns
DRNA_DEVICE_SEEDS = (0, 14, 17)
DRNA_OVERFLOW_SEED = 15
# k_roll_stream | k_roll_one for every read (w = 12 001) | the two-kernel path (w = 65 536, a row above 2^17)
ROLL_DEVICE_SEEDS = (31, 16, 0)


@pytest.mark.parametrize("seed", DRNA_DEVICE_SEEDS + (DRNA_OVERFLOW_SEED,))
def test_drna_device_form_gives_the_host_form_bytes(gpu, ora, monkeypatch, seed):
    """sk_drna_segment_dev_i16 -- what the benchmark times -- on device buffers against the host form on the same rows:
    the same segments and counts, nothing written behind either output.  With too few columns the host form returns
    SK_ERR_OVERFLOW and both forms leave the true counts in nsegs and the first max_segs segments in segs."""
    import ctypes as C
    from squigglekit_amd import _lib
    L = _lib.ensure_init()
    case = rc.case_of("drna", seed)
    for key in rc.SWITCHES:
        monkeypatch.delenv(key, raising=False)
    want = rc.expect_drna(ora, case)["segs"]
    counts = np.array([len(s) for s in want], dtype=np.int32)
    sig, lens = _rows_of(case)
    R, stride = sig.shape
    p = _lib.DrnaParams(**case["params"])
    for max_segs in ([int(counts.max()) + 1, 4] if seed == DRNA_OVERFLOW_SEED else [max(case["max_segs"], int(counts.max()))]):
        assert seed != DRNA_OVERFLOW_SEED or counts.max() > 32
        segs, nsegs = np.zeros((R, max_segs, 2), dtype=np.int32), np.zeros(R, dtype=np.int32)
        code = L.sk_drna_segment_batch_i16(_lib.ptr(sig), stride, _lib.ptr(lens), R, C.byref(p), _lib.ptr(segs), _lib.ptr(nsegs),
                                           max_segs)
        assert code == (_lib.SK_ERR_OVERFLOW if counts.max() > max_segs else _lib.SK_OK), rc.describe(case)
        assert np.array_equal(nsegs, counts), rc.describe(case)
        for r in range(R):
            assert segs[r, :min(counts[r], max_segs)].tolist() == want[r][:max_segs], (rc.describe(case), r)
        dev = DevBuffers(L)
        try:
            d_sig, d_len = dev.up(sig), dev.up(lens)
            d_segs, d_n = dev.out(segs.nbytes), dev.out(nsegs.nbytes)
            _lib.check(L.sk_drna_segment_dev_i16(d_sig, stride, d_len, R, C.byref(p), d_segs, d_n, max_segs))
            _lib.check(L.sk_sync())
            assert dev.down(d_n, nsegs.shape, np.int32).tobytes() == nsegs.tobytes(), rc.describe(case)
            assert dev.down(d_segs, segs.shape, np.int32).tobytes() == segs.tobytes(), rc.describe(case)
        finally:
            dev.free()


@pytest.mark.parametrize("seed", ROLL_DEVICE_SEEDS)
def test_roll_device_form_gives_the_host_form_bytes(gpu, ora, monkeypatch, seed):
    """sk_drna_roll_dev_i16 on device buffers against the host form and the oracle on the same rows."""
    import ctypes as C
    from squigglekit_amd import _lib
    L = _lib.ensure_init()
    case = rc.case_of("roll", seed)
    for key in rc.SWITCHES:
        monkeypatch.delenv(key, raising=False)
    want = rc.expect_roll(ora, case)["xy"]
    sig, lens = _rows_of(case)
    R, stride = sig.shape
    p = _lib.RollParams(**case["params"])
    xy, found = np.zeros((R, 2), dtype=np.int32), np.zeros(R, dtype=np.int32)
    _lib.check(L.sk_drna_roll_batch_i16(_lib.ptr(sig), stride, _lib.ptr(lens), R, C.byref(p), _lib.ptr(xy), _lib.ptr(found)))
    assert [(int(xy[r, 0]), int(xy[r, 1])) if found[r] else None for r in range(R)] == want, rc.describe(case)
    dev = DevBuffers(L)
    try:
        d_sig, d_len = dev.up(sig), dev.up(lens)
        d_xy, d_found = dev.out(xy.nbytes), dev.out(found.nbytes)
        _lib.check(L.sk_drna_roll_dev_i16(d_sig, stride, d_len, R, C.byref(p), d_xy, d_found))
        _lib.check(L.sk_sync())
        assert dev.down(d_found, found.shape, np.int32).tobytes() == found.tobytes(), rc.describe(case)
        assert dev.down(d_xy, xy.shape, np.int32).tobytes() == xy.tobytes(), rc.describe(case)
    finally:
        dev.free()


def other_layout(case):
    """the switches that put a pairs case on the other lane layout: without SK_DTW_NO_SMALL where it is set, with it
    where it is not -- and a call above the host threshold, which takes 16 lanes by itself, under a threshold above it"""
    if "SK_DTW_NO_SMALL" in case["env"]:
        return {k: v for k, v in case["env"].items() if k != "SK_DTW_NO_SMALL"}
    if case["npairs"] > rc.PAIRS_SMALL_MAX:
        return dict(case["env"], SK_DTW_SMALL_MAX=str(1 << 20))
    return dict(case["env"], SK_DTW_NO_SMALL="1")


@pytest.mark.parametrize("seed", rc.SEEDS["pairs"])
def test_pairs_seed_matches_the_reference(gpu, ora, monkeypatch, seed):
    """api.dtw_pairs on a drawn pool and pair list (either mode, a list of arrays or (values, off) with off[0] > 0; above
    the host threshold of 2 048 pairs without a switch, below it with and without SK_DTW_NO_SMALL): every record of every
    pair the reference's, the guard counters zero; then on the other lane layout: a different plan, the same bytes."""
    case = rc.case_of("pairs", seed)
    got, exp = run_case(monkeypatch, ora, case)
    assert got.dtype == gpu.HIT_DTYPE and len(got) == case["npairs"], rc.describe(case)
    other = dict(case, env=other_layout(case))
    assert rc.pairs_plan(other)["shape"] != rc.pairs_plan(case)["shape"] or \
        all(len(case["seqs"][q]) < 32 or len(case["seqs"][q]) > 256 for q in case["pairs"][:, 0]), rc.describe(case)
    again, _ = run_case(monkeypatch, ora, other)
    assert rc.result_bytes(again) == rc.result_bytes(got), "%s under %s" % (rc.describe(case), other["env"])


def run_again(monkeypatch, case, exp):
    """the case under its switches through the GPU against an expectation that exists already"""
    from squigglekit_amd import api
    for key in rc.SWITCHES:
        if key in case["env"]:
            monkeypatch.setenv(key, case["env"][key])
        else:
            monkeypatch.delenv(key, raising=False)
    got = rc.CALL[case["family"]](api, case, exp)
    msg = rc.DIFF[case["family"]](case, got, exp)
    assert msg is None, "%s\n  first difference: %s" % (rc.describe(case), msg)
    return got


@pytest.mark.parametrize("seed", rc.SEEDS["pairpaths"])
def test_pairpaths_seed_matches_the_reference(gpu, ora, monkeypatch, seed):
    """api.dtw_pairs_paths on a drawn list: records, span_off and spans of every pair the references', the self-check's
    count the case's (the changed records, no other), listed pairs, slab and wavefronts as randcases.pairpaths_plan
    restates them (all in diff_pairpaths); then under the two other tier settings: the same records and spans."""
    case = rc.case_of("pairpaths", seed)
    (rec, off, spans, counted, tiers), exp = run_case(monkeypatch, ora, case)
    assert counted == exp["mismatches"] and tiers[0] == len(rc.pairpaths_plan(case, exp["records"])["listed"])
    for env in rc.PP_TIERS:
        if env != case["env"]:
            again = run_again(monkeypatch, dict(case, env=dict(env)), exp)
            assert again[2].tobytes() == spans.tobytes() and again[0].tobytes() == rec.tobytes() and again[3] == counted, \
                "%s under %s" % (rc.describe(case), env)


def _padded_pool(case, pad=5):
    """(values, off) of the case's pool with `pad` NaN in front: the pool need not start at off = 0"""
    seqs = case["seqs"]
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate([np.full(pad, np.nan)] + [np.asarray(s, dtype=np.float64) for s in seqs]), off + pad


# the natural L = 16 route (2 049 pairs) | long targets beside short ones, global | SK_DTW_NO_SMALL, six groups and more
PAIRS_DEVICE_SEEDS = (23, 130, 133)
# computed records, the tiers as they fall | changed records, global, one wavefront | merged tile records, every pair listed
PAIRPATHS_DEVICE_SEEDS = (6, 13, 1)


@pytest.mark.parametrize("seed", PAIRS_DEVICE_SEEDS)
def test_pairs_device_form_gives_the_host_form_bytes(gpu, ora, monkeypatch, seed):
    """sk_dtw_pairs_dev on device buffers, the pool at a nonzero offset: the host form's bytes, which are the reference's
    records, and nothing written behind `out`."""
    from squigglekit_amd import _lib, api
    L = _lib.ensure_init()
    case = rc.case_of("pairs", seed)
    exp = rc.expect_pairs(ora, case)
    values, off = _padded_pool(case)
    pr = api._as_pairs(case["pairs"])
    host = run_again(monkeypatch, dict(case, form="list"), exp)
    dev = DevBuffers(L)
    try:
        d_val, d_out = dev.up(values), dev.out(host.nbytes)
        _lib.check(L.sk_dtw_pairs_dev(d_val, _lib.ptr(off), off.size - 1, _lib.ptr(pr), len(pr), api.PAIRS_MODES[case["mode"]],
                                      d_out))
        _lib.check(L.sk_sync())
        assert dev.down(d_out, host.shape, host.dtype).tobytes() == host.tobytes(), rc.describe(case)
    finally:
        dev.free()


@pytest.mark.parametrize("seed", PAIRPATHS_DEVICE_SEEDS)
def test_pairpaths_device_form_gives_the_host_form_bytes(gpu, ora, monkeypatch, seed):
    """sk_dtw_pairs_paths_dev on device buffers, the pool at a nonzero offset, records computed or supplied as the case
    has them: records and spans the host form's bytes (checked against the references), the same mismatch count, nothing
    written behind `records` or `spans`."""
    from squigglekit_amd import _lib, api
    L = _lib.ensure_init()
    case = rc.case_of("pairpaths", seed)
    exp = rc.expect_pairpaths(ora, case)
    rec, _, spans, counted, tiers = run_again(monkeypatch, case, exp)
    values, off = _padded_pool(case)
    pr = api._as_pairs(case["pairs"])
    have = exp["supplied"] is not None
    dev = DevBuffers(L)
    try:
        d_val = dev.up(values)
        d_rec = dev.inout(exp["supplied"].astype(gpu.HIT_DTYPE)) if have else dev.out(rec.nbytes)
        d_sp = dev.out(spans.nbytes)
        _lib.check(L.sk_dtw_pairs_paths_dev(d_val, _lib.ptr(off), off.size - 1, _lib.ptr(pr), len(pr),
                                            api.PAIRS_MODES[case["mode"]], d_rec, int(have), d_sp))
        _lib.check(L.sk_sync())
        assert L.sk_last_path_mismatches() == counted == exp["mismatches"], rc.describe(case)
        assert api.last_pair_paths_tiers() == tiers, rc.describe(case)
        assert dev.down(d_rec, rec.shape, rec.dtype).tobytes() == rec.tobytes(), rc.describe(case)
        assert dev.down(d_sp, spans.shape, np.int32).tobytes() == spans.tobytes(), rc.describe(case)
    finally:
        dev.free()


@pytest.mark.parametrize("seed", rc.SEEDS["band"])
def test_band_seed_matches_the_statement(gpu, ora, monkeypatch, seed):
    """api.dtw_band (or, device form, sk_dtw_band_dev) on a drawn pool and list under a drawn width, end, pool form and
    SK_BAND_WAVES, with paths or records only as drawn: every record of every pair the statement's (bits of dist, two NaNs
    agree), span_off and spans as integers, the mismatch count the statement's pairs without a path, the plan the header's
    slab formula and no more wavefronts than forced (all in diff_band); then the other of the two calls -- records only
    where paths were drawn, paths where they were not: the same record bytes."""
    case = rc.case_of("band", seed)
    got, exp = run_case(monkeypatch, ora, case)
    other = run_again(monkeypatch, dict(case, paths=not case["paths"]), exp)
    assert other[0].tobytes() == got[0].tobytes(), rc.describe(case)
    assert (other if case["paths"] else got)[4][0] == 0 < (got if case["paths"] else other)[4][0], rc.describe(case)


# W = 128 pinned, 35 pairs under 3 wavefronts | W = 256 free, 30 pairs under 3 | W = 64 pinned, three pairs lost by a -inf
BAND_DEVICE_SEEDS = (138, 297, 240)


@pytest.mark.parametrize("seed", BAND_DEVICE_SEEDS)
def test_band_device_form_gives_the_host_form_bytes(gpu, ora, monkeypatch, seed):
    """sk_dtw_band_dev on device buffers, the pool at a nonzero offset, with spans and without: the host form's records
    and spans (checked against the statement), the same mismatch count, nothing written behind `records` or `spans`, and
    without spans nothing written to them at all."""
    from squigglekit_amd import api
    case = rc.case_of("band", seed)
    assert case["form"] == "device"
    exp = rc.expect_band(ora, case)
    rec, off, spans, counted, _, _ = run_again(monkeypatch, dict(case, form="list", paths=True), exp)
    for with_spans in (True, False):
        drec, dspans, dcounted, clean = rc.band_device_call(api, case, with_spans, len(spans))
        assert clean and drec.tobytes() == rec.tobytes(), (rc.describe(case), with_spans)
        assert not with_spans or (dspans.tobytes() == spans.tobytes() and dcounted == counted == exp["mismatches"])
        assert api.last_band_plan()[0] == (rc.band_slab_bytes(case["longest"], case["W"]) if with_spans else 0)


_hmmpost_cases = {}


def hmmpost_case(seed):
    """(case, the statement's answer) of a committed hmmpost seed: computed once, shared by the tests below, never changed"""
    if seed not in _hmmpost_cases:
        case = rc.case_of("hmmpost", seed)
        _hmmpost_cases[seed] = (case, rc.expect_hmmpost(None, case))
    return _hmmpost_cases[seed]


@pytest.mark.parametrize("seed", rc.SEEDS["hmmpost"])
def test_hmmpost_seed_matches_the_statement(gpu, monkeypatch, seed):
    """api.hmm_posterior_batch, hmm_posterior_ragged_f64 or hmm_posterior on a drawn model and drawn reads under drawn
    switches, with the outputs the case asks for: n_used, flags, every double of the records and of the counts by its
    bits, goff as integers, the dense rows by their bits and without a NaN (all in diff_hmmpost).  Then the complementary
    call -- counts where none were drawn and the other way round, likewise the dense rows -- which takes the other
    instantiation of k_hmm_bwd: what it returns is the statement's too, and its records are the first call's bytes."""
    case, exp = hmmpost_case(seed)
    got = run_again(monkeypatch, case, exp)
    assert (got[1] is not None) == case["counts"] and (got[3] is not None) == case["dense"], rc.describe(case)
    other = run_again(monkeypatch, dict(case, counts=not case["counts"], dense=not case["dense"]), exp)
    assert other[0].tobytes() == got[0].tobytes() == exp["post"].tobytes(), rc.describe(case)


def test_hmmpost_wavefront_with_both_kinds_of_reads_lane_by_lane(gpu, monkeypatch):
    """The hand-made case of randcases.hmmpost_both_kinds: 65 reads, a possible one (two samples in most) in every even
    lane and an impossible one in every odd lane, against the statement, with counts and dense rows and without."""
    made = rc.hmmpost_both_kinds(*hmmpost_case(rc.POST_BOTH_SEED))
    exp = rc.expect_hmmpost(None, made)
    assert (exp["post"]["flags"][0::2] == 0).all() and (exp["post"]["flags"][1::2] != 0).all()
    for counts, dense in ((True, True), (False, False)):
        got = run_again(monkeypatch, dict(made, counts=counts, dense=dense), exp)
        assert got[0].tobytes() == exp["post"].tobytes() and (got[1] is not None) == counts and (got[3] is not None) == dense


# a calibrated batch on the 2-byte load path (stride 1 499), six states | SK_HMM_SCRATCH_MB=1: 200 reads in four slices of
# one group, B = 4 096 | an aligned stride (1 032), calibrated: 16-byte loads as it stands, and vec = 0 through the base
# when that is shifted by 2 or by 8 bytes
HMMPOST_DEVICE_SEEDS = (162, 185, 34)
HMMPOST_SHIFTED_SEED = 34


@pytest.mark.parametrize("seed", HMMPOST_DEVICE_SEEDS)
def test_hmmpost_device_form_gives_the_host_form_bytes(gpu, monkeypatch, seed):
    """sk_hmm_posterior_dev_i16 on device buffers with guard bytes behind post, counts and the dense rows: the host form's
    bytes, which are the statement's; with counts and the dense rows NULL the same records and not a byte written to
    either buffer.  The seed with the aligned stride runs again with its rows 2 and 8 bytes behind a 16-byte boundary."""
    from squigglekit_amd import api
    case, exp = hmmpost_case(seed)
    assert case["feed"] == "batch"
    case = dict(case, counts=True, dense=True)
    host = run_again(monkeypatch, case, exp)
    assert seed != HMMPOST_SHIFTED_SEED or case["stride"] % 8 == 0
    for shift in ((0, 2, 8) if seed == HMMPOST_SHIFTED_SEED else (0,)):
        for counts, dense in ((True, True), (False, False)):
            got = rc.hmmpost_device_call(api, case, counts, dense, shift)
            msg = rc.diff_hmmpost(case, got, exp)
            assert msg is None, "%s shift %d counts %s dense %s\n  first difference: %s" % (rc.describe(case), shift, counts,
                                                                                         dense, msg)
            assert got[4], "%s shift %d counts %s dense %s: bytes behind an output, or in a buffer that was not asked for" % (
                rc.describe(case), shift, counts, dense)
            assert got[0].tobytes() == host[0].tobytes(), (rc.describe(case), shift)
            assert (got[1] is None) == (not counts) and (got[3] is None) == (not dense)
            if counts:
                assert got[1].tobytes() == host[1].tobytes() and got[3].tobytes() == host[3].tobytes(), (rc.describe(case), shift)


FILTER_CHUNKS = (0, 1, 2, 31, 32, 33, 127, 128, 129)                   # 0: a peek; the seams of both tiles


def same_as_records(filt, post, slots, what):
    """the filters of `slots` against loglik, final_post, n_used and flags of their posterior records, bit for bit"""
    want = np.zeros(len(slots), dtype=filt.dtype)
    for f, g in (("loglik", "loglik"), ("n_used", "n_used"), ("flags", "flags"), ("post", "final_post")):
        want[f] = post[g][slots]
    assert not np.isnan(filt["loglik"]).any() and not np.isnan(filt["post"]).any(), what
    if filt.tobytes() != want.tobytes():
        bad = [i for i in range(len(want)) if filt[i].tobytes() != want[i].tobytes()]
        raise AssertionError("%s: slot %d (%d slots differ)\n got  %r\n want %r" % (what, int(slots[bad[0]]), len(bad),
                                                                                  filt[bad[0]], want[bad[0]]))


@pytest.mark.parametrize("seed", rc.SEEDS["hmmpost"])
def test_filtered_session_twin_of_the_hmmpost_seed(gpu, monkeypatch, seed):
    """Every committed posterior case through a filtered session (k_hmms_push<FILT = true>) beside a plain one: each read's
    first n_used samples arrive as chunks cut by default_rng([99, 14, seed]) -- 0, 1, 2, the seams of both tiles, or the
    rest of the read at once -- for a shuffled subset of the slots per push, integer reads through push (under the case's
    calibration pairs), float reads through push_values.  The plain session's records are the filtered one's bytes after
    every push; once, at a drawn push, the filters of all slots are the statement of the prefixes pushed so far; at the end
    they are loglik, final_post, n_used and flags of the case's records, and a slot that got nothing has the empty filter."""
    import hmm_post_ref
    import hmmfilter_ref as FR
    from squigglekit_amd import api
    case, exp = hmmpost_case(seed)
    for key in rc.SWITCHES:
        monkeypatch.delenv(key, raising=False)
    rng = np.random.default_rng([99, 14, seed])
    x, used = rc.hmmpost_rows(case)
    R, reads = case["R"], case["reads"]
    is_int = np.array([rc._is_int_read(r) for r in reads])
    model = rc.hmm_model_of(api, case)
    everyone = np.arange(R)
    at = np.zeros(R, dtype=np.int64)
    check_at, rounds, checked = int(rng.integers(1, 5)), 0, False
    what = rc.describe(case)
    with api.HmmStream(model, R, filter=True) as hf, api.HmmStream(model, R) as hp:
        if case["cal"] is not None:
            hf.reset(everyone, case["cal"])
            hp.reset(everyone, case["cal"])
        assert hf.filter(everyone).tobytes() == FR.empty_filters(R).tobytes(), what
        while (at < used).any() or not checked:
            live = np.flatnonzero(at < used)
            named = np.concatenate([live[rng.random(live.size) < 0.7], everyone[rng.random(R) < 0.05]])
            named = rng.permutation(np.unique(np.concatenate([named, live[:1]]))).astype(np.int64)
            cut = np.where(rng.random(named.size) < 0.25, 1 << 30, rng.choice(FILTER_CHUNKS, size=named.size))
            cut = np.minimum(cut, used[named] - at[named])
            for ints in (True, False):
                sel = is_int[named] == ints
                slots, n = named[sel], cut[sel]
                if not slots.size:
                    continue
                chunks = [reads[s][at[s]:at[s] + k] for s, k in zip(slots, n)]
                if ints:
                    chunks = [np.asarray(c, dtype=np.int16) for c in chunks]
                    rec, plain = hf.push(slots, chunks), hp.push(slots, chunks)
                else:
                    rec, plain = hf.push_values(slots, chunks), hp.push_values(slots, chunks)
                at[slots] += n
                assert plain.tobytes() == rec.tobytes() and np.array_equal(rec["n_used"], at[slots]), (what, rounds)
            rounds += 1
            if rounds >= check_at and not checked:
                checked = True
                prefix = hmm_post_ref.posterior_rows(case["model"], x, at, counts=False, dense=False)[0]
                same_as_records(hf.filter(everyone), prefix, everyone, "%s: prefixes after %d rounds" % (what, rounds))
        assert np.array_equal(at, used)
        same_as_records(hf.filter(everyone), exp["post"], everyone, what + ": the whole reads")
        nothing = np.flatnonzero(used == 0)
        assert hf.filter(nothing).tobytes() == FR.empty_filters(nothing.size).tobytes(), what
        assert hf.peek(everyone).tobytes() == hp.peek(everyone).tobytes(), what
    assert api.last_hmm_stream_plan()["guard_hits"] == 0


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


def test_drna_calls_interleaved_with_the_segmenter_and_the_detector(gpu, ora, monkeypatch):
    """Both dRNA branches between segmenter, levels, hit-list and detector calls: c->mask, prep, comp and misc are the same
    grow-only buffers for all of them (the rolling branch lays two masks and its redo list or its prefix sums in them, the
    slow5 branch transposed words of nreads rows), a large case of each family before a small one."""
    run_sequence(monkeypatch, ora, rc.INTERLEAVE3)


def test_pair_calls_interleaved_with_the_path_and_screening_families(gpu, ora, monkeypatch):
    """Pair lists and their warping paths between paths, events, hit-list, screening and segmenter calls: c->pathcnt,
    c->pathlist (an 8-word header here, 2 words in sk_path.hip) and c->pathscratch are shared with the alignment paths,
    and a pair call resets the retry and profile state the screening counters are read through.  Every call against its
    reference (mismatch counts, tiers and guard counters included), a call that occurs twice the same bytes both times."""
    run_sequence(monkeypatch, ora, rc.INTERLEAVE4)


def test_band_calls_interleaved_with_the_pair_and_hit_families(gpu, ora, monkeypatch):
    """Band lists between pair lists, their warping paths and hit lists: c->pathcnt is the one mismatch counter of all
    path kernels (a call that counts some directly before one that must count none, both ways round), the band's table and
    slabs only grow (the widest slabs before a list of one short pair and again after it).  Every call against its
    reference, a call that occurs twice the same bytes both times."""
    run_sequence(monkeypatch, ora, rc.INTERLEAVE5)


def test_posterior_calls_interleaved_with_the_viterbi_and_other_families(gpu, ora, monkeypatch):
    """Posterior calls between Viterbi, detector, levels, pair-list and band calls: c->hmm holds the records of both HMM
    calls, c->hmmpost (L, checkpoints, slabs) and c->hmmpostout (counts, goff, dense rows) only grow -- the largest case
    before a call of one short read, a case in four slices directly after a state-path call in three slices of the same
    SK_HMM_SCRATCH_MB budget.  Every call against its reference, a call that occurs twice the same bytes both times."""
    run_sequence(monkeypatch, ora, rc.INTERLEAVE6)
