"""CPU leg of the seeded random cases (tests/randcases.py): the generators and the references alone over the committed
seed lists, asserting that the cases are what tests/RANDOM_CASES.md claims.  These are conditions on the INPUTS of
tests/test_gpu_random.py, not measurements of the code under test: if one fails, change the generator or the seed list,
never the cap."""
import numpy as np
import pytest

import randcases as rc


@pytest.fixture(scope="module")
def cases(ora):
    """family -> [(case, expectation)] over the committed seeds."""
    out = {}
    for fam in rc.SEEDS:
        out[fam] = []
        for seed in rc.SEEDS[fam]:
            case = rc.case_of(fam, seed)
            out[fam].append((case, rc.EXPECT[fam](ora, case)))
    return out


# ---- what one case reaches (labels; the seed lists must reach every label of REQUIRED) ----------------------------
def sweep_features(case):
    f = {"form=" + case["form"], "groups=%d" % len(case["group_counts"]), "rows=" + case["rowkind"]}
    general = "SK_WALK_GENERAL" in case["env"]
    for n, _ in case["group_counts"]:
        f.add("count=%d" % n)
        if n > rc.SWEEP_LANES:
            f.add("count>64")
    kinds = {rc.sweep_is_fast(s) for s in case["sets"]}
    if len(kinds) == 2 and not general:
        f.add("both walk kinds in one call")
    for s in case["sets"]:
        f.add("wide limits" if s["lim_hi"] - s["lim_low"] > 38000 else "narrow limits")
        if s["window"] == 0:
            f.add("window=0")
        if s["stall_len"] == 0:
            f.add("stall_len=0")
        if s["error"] >= s["corrector"]:
            f.add("error>=corrector")
        if s["error"] in (0, -1):
            f.add("error=%d" % s["error"])
        f.add("seg_dist=%s" % ("huge" if s["seg_dist"] >= 10 ** 9 else s["seg_dist"]))
    for r in case["reads"]:
        if len(r) in rc.SWEEP_LENS:
            f.add("len=%d" % len(r))
        if len(r) >= rc.SWEEP_LONG:
            f.add("len>=70000")
        if r.dtype == np.float64:
            f.add("float64<=4096" if len(r) <= rc.F64_STREAM_MAX else "float64>4096")
            if not np.all(np.isfinite(r)):
                f.add("NaN/inf inside")
            fin = r[np.isfinite(r)]
            if np.unique(fin).size < fin.size and np.all(np.round(fin, 2) == fin):
                f.add("ties on a 0.01 grid")
        elif len(r) and np.all(r == r[0]):
            f.add("constant row" if 0 < r[0] < 900 else "row empty after the filter")
    if case["rowkind"] in ("squiggle", "both") and case["M"] >= 512:
        f.add("squiggle_batch M>=512")
    if case["rowkind"] in ("pattern", "both") and case["M"] >= 512:
        f.add("pattern_reads M>=512")
    if case["form"] == "batch" or any(r.dtype == np.int16 for r in case["reads"]):
        f.add("int16 rows")
    if "SK_SEG_DELTA_SCALE" in case["env"]:
        f.add("forced redo")
    if general:
        f.add("SK_WALK_GENERAL")
    return f


SWEEP_REQUIRED = ({"count=%d" % n for n in rc.SWEEP_COUNTS} | {"len=%d" % n for n in rc.SWEEP_LENS} |
                  {"count>64", "both walk kinds in one call", "wide limits", "narrow limits", "window=0", "stall_len=0",
                   "error>=corrector", "error=0", "error=-1", "seg_dist=0", "seg_dist=1", "seg_dist=huge", "len>=70000",
                   "float64<=4096", "float64>4096", "NaN/inf inside", "ties on a 0.01 grid", "constant row",
                   "row empty after the filter", "squiggle_batch M>=512", "pattern_reads M>=512", "int16 rows",
                   "forced redo", "SK_WALK_GENERAL", "form=batch", "form=list", "groups=2", "groups=3", "groups=4"})


def hits_features(case):
    f = {"K=%d" % case["K"], "cut=" + case["cut"], "route=" + case["route"], "scale=" + case["scale"],
         "motifs=%d" % len(case["motifs"])}
    for N in case["Ns"]:
        if N in rc.HITS_N:
            f.add("N=%d" % N)
        else:
            f.add("N random")
    N0 = case["Ns"][0] if case["special"] != "plateau" else None
    lens = {len(r) for r in case["reads"]}
    if N0 is not None:
        for name, n in (("n=1", 1), ("n=N-1", max(2, N0 - 1)), ("n=N", max(2, N0)), ("n=N+1", N0 + 1), ("n=2N", 2 * N0)):
            if n in lens:
                f.add(name)
    if max(lens) >= rc.HITS_LONG:
        f.add("read>=100000")
    if any(n > rc.HIT_CACHE_COLS for n in lens):
        f.add("read beyond the register cache")
    if "t" in case["kinds"]:
        f.add("tie-heavy read")
    if "d" in case["kinds"]:
        f.add("many dropped samples")
    if case["route"] == "batch" and case["stride"] > case["longest"]:
        f.add("stride > longest row")
    if case["env"].get("SK_DTW_SMALL_MAX") == "0":
        f.add("SK_DTW_SMALL_MAX=0")
    if rc.hits_chunks(case) >= 3:
        f.add("chunks>=3")
    if case["family"] == "paths":
        lds = case["env"].get("SK_PATH_LDS_BYTES")
        f.add("lds=" + ("unset" if lds is None else "0" if lds == "0" else "split"))
        if "SK_PATH_SCRATCH_BYTES" in case["env"]:
            f.add("one scratch wavefront")
        if len(set(case["Ns"])) > 1:
            f.add("motifs of different lengths")
        if rc.hits_chunks(case) >= 3:
            f.add("chunks>=3 with paths")
        if case["special"] == "plateau":
            f.add("plateau read")
    return f


HITS_REQUIRED = ({"N=%d" % n for n in rc.HITS_N} | {"K=%d" % k for k in rc.HITS_K} |
                 {"route=" + r for r in rc.HITS_ROUTES} |
                 {"N random", "cut=inf", "cut=median2", "cut=below", "scale=medmad", "scale=zscale", "motifs=1", "motifs=2",
                  "motifs=3", "n=1", "n=N-1", "n=N", "n=N+1", "n=2N", "read>=100000", "read beyond the register cache",
                  "tie-heavy read", "many dropped samples", "stride > longest row", "SK_DTW_SMALL_MAX=0", "chunks>=3"})
PATHS_REQUIRED = (HITS_REQUIRED - {"read>=100000"}) | {"lds=unset", "lds=0", "lds=split", "one scratch wavefront",
                                                      "motifs of different lengths", "chunks>=3 with paths",
                                                      "plateau read"}


def _missing(required, cases, features):
    have = set()
    for case, _ in cases:
        have |= features(case)
    return sorted(required - have)


def test_sweep_cases_reach_every_boundary(cases):
    assert len(cases["sweep"]) >= 4
    assert not _missing(SWEEP_REQUIRED, cases["sweep"], sweep_features)


def test_hits_cases_reach_every_boundary(cases):
    assert len(cases["hits"]) >= 4
    assert not _missing(HITS_REQUIRED, cases["hits"], hits_features)


def test_paths_cases_reach_every_boundary(cases):
    assert len(cases["paths"]) >= 4
    assert not _missing(PATHS_REQUIRED, cases["paths"], hits_features)


def test_paths_cases_cross_the_word_packing_and_both_tiers(cases):
    """The widths W of the reference's hits lie on both sides of a multiple of 16 (one direction word) and of 64 (one
    block of steps); some case has hits in each tier under its own SK_PATH_LDS_BYTES; one window is wider than
    PATH_LDS_COLS."""
    res16, res64, both, widest = set(), set(), 0, 0
    for case, exp in cases["paths"]:
        tiers = set()
        for m, want in enumerate(exp["want"]):
            N = len(case["motifs"][m])
            for w in want:
                for (_, start, end), _sp in (w or []):
                    W = end - start + 1
                    widest = max(widest, W)
                    if W > 8:
                        res16.add(W % 16)
                    if W > 32:
                        res64.add(W % 64)
                    tiers.add(rc.path_tier(case, N, W))
        both += len(tiers) == 2
    assert {15, 0, 1} <= res16, sorted(res16)            # W = 16 m - 1, 16 m, 16 m + 1 (the last word holds 15, 16, 1 cells)
    assert {63, 0, 1} <= res64, sorted(res64)
    assert both >= 1
    assert widest > rc.PATH_LDS_COLS


@pytest.mark.parametrize("fam", ["hits", "paths"])
def test_hit_cases_have_hits_to_compare(cases, fam):
    """Reads the reference leaves out (None) are at most 10 % of the family's reads and at most half of any case; a
    quarter of the cases have a read with >= 2 hits; somewhere the reference returns fewer than K."""
    reads = none = multi = 0
    fewer = zero = False
    for case, exp in cases[fam]:
        want0 = exp["want"][0]
        n_none = sum(w is None for w in want0)
        assert 2 * n_none <= len(want0), rc.describe(case)
        reads += len(want0)
        none += n_none
        multi += any(w is not None and len(w) >= 2 for want in exp["want"] for w in want)
        fewer |= any(w is not None and len(w) < case["K"] for want in exp["want"] for w in want)
        zero |= any(w is not None and len(w) == 0 for want in exp["want"] for w in want)
    assert 10 * none <= reads, (none, reads)
    assert 4 * multi >= len(cases[fam]), (multi, len(cases[fam]))
    assert fewer
    assert zero                                          # a max_dist cut that leaves a read without hits


def test_sweep_cases_have_segments_to_compare(cases):
    """In at least half of the sets the oracle finds a segment in some read; some (set, read) has >= 3 segments before
    the two-segment cut, so the count after merges is exercised."""
    sets = found = 0
    most = 0
    for case, exp in cases["sweep"]:
        n = exp["nsegs_all"]
        sets += n.shape[0]
        found += int((n.max(axis=1) >= 1).sum())
        most = max(most, int(n.max()))
    assert 2 * found >= sets, (found, sets)
    assert most >= 3


def test_pull_cases_reach_every_alignment_and_token_length(cases):
    """Line starts and line ends take all 16 residues (with them the head / body / tail split of k_pull_write); the
    shortest and the longest tokens the kernel accepts stand next to each other; every listed length, both modes, both
    entry points."""
    assert len(cases["pull"]) >= 4
    starts, ends, lens, modes, entries, plens = set(), set(), set(), set(), set(), set()
    adjacent = False
    for case, exp in cases["pull"]:
        text = exp["text"]
        nl = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10)
        assert len(nl) == case["R"]
        off = np.concatenate([[0], nl + 1])
        starts |= {int(v) % rc.PULL_ALIGN for v in off[:-1]}
        ends |= {int(v) % rc.PULL_ALIGN for v in off[1:]}
        lens |= {int(n) for n in case["lens"]}
        plens |= {len(p) % rc.PULL_ALIGN for p in case["prefixes"]}
        modes.add(case["raw"])
        entries.add(case["entry"])
        if not case["raw"]:
            for r in range(case["R"]):
                if case["kinds"][r] != "h" or not case["lens"][r]:
                    continue
                toks = text[off[r] + len(case["prefixes"][r]):off[r + 1] - 1].split(b"\t")
                size = [len(t) for t in toks]
                assert max(size) <= rc.PULL_TOK_MAX - 1
                adjacent |= any({a, b} == {3, rc.PULL_TOK_MAX - 1} for a, b in zip(size, size[1:]))
    assert starts == set(range(16)) and ends == set(range(16)) and plens == set(range(16))
    assert set(rc.PULL_LENS) <= lens
    assert modes == {True, False} and entries == {"host", "dev"}
    assert adjacent
    kinds = "".join(case["kinds"] for case, _ in cases["pull"])
    assert set("nthf") <= set(kinds)


# ---- the four first families stay what they were ---------------------------------------------------------------------
# randcases.case_digest of every committed case, computed on the commit before randcases.FAMILY_INDEX replaced
# sorted(SEEDS).index(family) in rng_of: the mutant table and the "found by" note of RANDOM_CASES.md rest on these cases.
PINNED = {
    "hits": {
        1: "27f07b8c5942dbc366da0a38d2e04789c9ceb96821d5c99491a1b788eb5f3351",
        20: "4696bdc90ae0bb783c22db9599b8432f7e4a0e40e544740e44e8cbecf55328cb",
        87: "a48cca924de101d5ddad9d1f3dc1983032a46c750c248bf09986a281263c5bc4",
        95: "1c6e4e3cf70bc14d45f3f09662d5af7a16f70a5bc6e2e83ed5ef1676c2689607",
        131: "ae3b7e275dbc5940c51a7a0a16d8c34ef5886d4165605a9f65c773443dbc121a",
        214: "aa03c3f0e821a5082e78361067c943e1244eff365c3004b332724b8de5f870a4",
        298: "4cfaa403c86d3c7e49616f531d3612243a4111e833c61824f730f992d6b5428c",
        324: "f117a8271716f6ce94c278389a7db48a05f8560f9a5687f66205a1813f0e2bba",
    },
    "paths": {
        1: "0eee0e337e3fddb8ee06c73806af3314d18655fd183997dfcc3414456a189df6",
        12: "263943563af8b702342025e34f75015694e1bb9c8e9b086f7129280ba39fa309",
        29: "a8edb800ed46b0346ac2c7606de4b1238b24e7c7eeab527b21708b0a59048c7e",
        50: "e3d9d936b2299b420907542090b571c1bfe086e38840cef7ebfe98eb5040ec3b",
        123: "52ba1c4839baa8c1001b0e09c29e90f93dc2069bb45d119fd2a63b7be7c52753",
        135: "18b928e7be9147ef6bb75f585d2b931c8d07fd5a87a116a48cdc1cb4442a51cc",
        187: "a1aa203da67274cbe51ab7e6efb44ad1c323ffb80bcf26d070165e540f5155e8",
        272: "fdfef044c36d70963c06c5f257a7d3273c2b506dc7d916349ab00951b1a25e40",
    },
    "pull": {
        0: "aecb19223df2ce52c1527757ab6749adbd909787b8715bd3444f118ade46e50f",
        3: "c6caceb7c34d79a9859b0bc1fab888520cbbc347d1b8fa3c3c01458cdc856879",
        21: "cd714ff5ed05cb21b73e229e34a51bca18e92169ae0e2eb42b89566800352207",
        40: "f6562ed68411614fcd372dcc00618761de1b1eaea43038aba57fd9c566f01c34",
    },
    "sweep": {
        16: "c7390b1cb6a1c3713cdccdd83891432f3ddb3e4abc0a16948c93f0874714e854",
        22: "6d02cb7a3d88efdb1c4c5952ac7a1c64b28704b9c81ac452148d5b0b7c9d8618",
        60: "e258e763abcad720cb1b201d10841e8a190ac6fefce6d3899fbc8e5d216f707f",
        97: "50812934ad981e9924a89f7aefc608ceda918b0a88df58887da2d48b93e0535b",
    },
}


def test_old_families_keep_their_cases():
    assert {f: rc.FAMILY_INDEX[f] for f in PINNED} == dict(hits=0, paths=1, pull=2, sweep=3)
    assert sorted(set(rc.FAMILY_INDEX.values())) == list(range(len(rc.FAMILY_INDEX)))
    for fam, want in PINNED.items():
        assert list(want) == rc.SEEDS[fam], fam
        for seed, digest in want.items():
            assert rc.case_digest(rc.case_of(fam, seed)) == digest, (fam, seed)


# ---- panel -----------------------------------------------------------------------------------------------------------
def panel_scores(exp):
    recs, flags = exp["ref"][0], exp["ref"][1]
    with np.errstate(all="ignore"):
        s = (recs["dist"] - exp["means"][:, None]) / exp["sds"][:, None]
    s[:, flags != 0] = np.nan
    return s


def panel_features(case, exp):
    f = {"K=%d" % case["K"], "route=" + case["route"], "scale=" + case["scale"], case["route"] + " " + case["scale"]}
    Ns = case["Ns"]
    for g in rc.panel_groups(case):
        shaped = [sh for sh in g if sh is not None]
        for sh in shaped:
            L, R = sh
            f.add("L%d R=%d" % (L, R))
            for k in g[sh]:
                P = L * R - Ns[k]
                if P in (0, 1, L - 1):
                    f.add("L%d P=%s" % (L, {0: "0", 1: "1"}.get(P, "L-1")))
                if L == 16 and R == 1 and P > 0:
                    f.add("no-row lanes at L16")
        apart = [sh for sh in shaped if len(g[sh]) >= 2 and g[sh][-1] - g[sh][0] >= len(g[sh])]
        if len(shaped) >= 3 and len(apart) >= 2:
            f.add("three groups interleaved")
            if None in g:
                f.add("three groups interleaved and a long motif")
    for N in (1024, 1025):
        if N in Ns:
            f.add("N=%d" % N)
    wins = rc.panel_windows(case)
    N0 = Ns[0]
    L0 = (rc.panel_shape(N0, rc.panel_calls(case)[0] * case["K"], case["env"]) or (64, 0))[0]
    sizes = {w for _, w in wins}
    for name, w in (("0", 0), ("1", 1), ("7", 7), ("8", 8), ("9", 9), ("N-1", N0 - 1), ("N", N0), ("N+1", N0 + 1),
                    ("L-1", L0 - 1), ("L", L0), ("L+1", L0 + 1), ("2L+1", 2 * L0 + 1)):
        if w in sizes:
            f.add("window=" + name)
    if case["win"] is not None:
        f.add("win rows")
        if any(tuple(row) == (10 ** 6, -10 ** 6) for row in case["win"].tolist()):
            f.add("win row (1e6, -1e6)")
        pairs = [tuple(row) for row in case["win"].tolist()]
    else:
        pairs = [case["region"]]
    for a, b in pairs:
        if a < 0:
            f.add("negative begin")
        if b is None or b == rc.INT32_MAX:
            f.add("open end")
        if b is not None and 0 <= b <= a:
            f.add("begin >= end")
    if any(lo >= len(r) > 0 for (lo, _), r in zip(wins, case["reads"])):
        f.add("region beyond the read")
    flags = exp["ref"][1]
    if any(flags[r] == 2 and wins[r][1] >= 2 for r in range(case["nreads"])):
        f.add("MAD 0 window")
    if any(flags[r] == 1 and wins[r][1] >= 1 for r in range(case["nreads"])):
        f.add("nothing inside the limits")
    if "t" in case["kinds"]:
        f.add("tie-heavy window")
    if case["route"] == "batch" and case["stride"] > case["longest"] and \
            any(np.any(case["sig"][r, n:] != 0) for r, n in enumerate(case["lens"])):
        f.add("stride > longest row, padding not zeros")
    if case["route"] == "list" and 0 < case["nfloat"] < case["nreads"]:
        f.add("mixed list")
    if rc.panel_screened(case):
        f.add("screened")
    s = panel_scores(exp)
    best, second, sb, ss = exp["ref"][3:]
    if np.any((second >= 0) & (sb == ss)):
        f.add("tie for best")
    with np.errstate(invalid="ignore"):
        if np.any((second >= 0) & (ss > sb) & ((s == ss[None, :]).sum(axis=0) >= 2)):
            f.add("tie for second")
    return f


def subsequence_dtw(x, y, left_first=False):
    """(dist, start, end) of the subsequence DTW of motif x in y by the plain recurrence; the smallest of diag, left, up
    in that order (the reference's), or with left before diag"""
    N, n = len(x), len(y)
    D = np.empty((N, n))
    S = np.empty((N, n), dtype=np.int64)
    for i in range(N):
        for j in range(n):
            c = abs(x[i] - y[j])
            if i == 0:
                D[i, j], S[i, j] = c, j
            elif j == 0:
                D[i, j], S[i, j] = c + D[i - 1, 0], S[i - 1, 0]
            else:
                cand = [(D[i - 1, j - 1], S[i - 1, j - 1]), (D[i, j - 1], S[i, j - 1]), (D[i - 1, j], S[i - 1, j])]
                if left_first:
                    cand[0], cand[1] = cand[1], cand[0]
                best = cand[0]
                for v in cand[1:]:
                    if v[0] < best[0]:
                        best = v
                D[i, j], S[i, j] = c + best[0], best[1]
    end = int(np.argmin(D[-1]))
    return float(D[-1, end]), int(S[-1, end]), end


def panel_tie_moves_start(ora, case, exp):
    """The planted run at the window's median: the reference's record of the zero-led motif is the plain recurrence's, and
    the same recurrence with `left` before `diag` starts the hit elsewhere."""
    if not case["plateau"] or "z" not in case["kinds"]:
        return False
    k, r = case["plateau"][0], case["kinds"].index("z")
    lo, w = rc.panel_windows(case)[r]
    f = ora.scale_outliers(np.asarray(case["reads"][r][lo:lo + w], dtype=np.float64), *rc.PANEL_LIMITS)
    if exp["ref"][1][r] != 0 or not f.size:
        return False
    y = ora.medmad(f)[0]
    ref = exp["ref"][0][k][r]
    d, s0, e0 = subsequence_dtw(case["motifs"][k], y)
    assert (d, s0, e0) == (float(ref["dist"]), int(ref["start"]), int(ref["end"])), rc.describe(case)
    d2, s1, e1 = subsequence_dtw(case["motifs"][k], y, left_first=True)
    return d2 == d and e1 == e0 and s1 != s0


PANEL_REQUIRED = ({"K=%d" % k for k in rc.PANEL_K} | {"L%d R=%d" % (L, R) for L in (16, 64) for R in range(1, 17)} |
                  {"L%d P=%s" % (L, P) for L in (16, 64) for P in ("0", "1", "L-1")} |
                  {"window=" + w for w in ("0", "1", "7", "8", "9", "N-1", "N", "N+1", "L-1", "L", "L+1", "2L+1")} |
                  {"route=batch", "route=f64", "route=list", "f64 medmad", "f64 zscale", "scale=medmad", "scale=zscale",
                   "no-row lanes at L16", "three groups interleaved and a long motif", "N=1024", "N=1025", "win rows",
                   "win row (1e6, -1e6)", "negative begin", "open end", "begin >= end", "region beyond the read",
                   "MAD 0 window", "nothing inside the limits", "tie-heavy window",
                   "stride > longest row, padding not zeros", "mixed list", "screened", "tie for best", "tie for second",
                   "a left / diag tie that moves start"})


def test_panel_cases_reach_every_boundary(ora, cases):
    assert len(cases["panel"]) >= 4
    have = set()
    for case, exp in cases["panel"]:
        have |= panel_features(case, exp)
        if panel_tie_moves_start(ora, case, exp):
            have.add("a left / diag tie that moves start")
        if case["screen"]:
            assert case["Ns"][0] == 16, rc.describe(case)
    assert not sorted(PANEL_REQUIRED - have)


def test_panel_cases_compare_nine_reads_in_ten_within_the_cell_budget(cases):
    """In every case fewer than 10 % of the reads are left out of the comparison of dist (MAD 0: the reference divides by
    zero there), and the oracle fills at most PANEL_CELLS cells."""
    for case, exp in cases["panel"]:
        flags = exp["ref"][1]
        assert 10 * int(np.count_nonzero(flags == 2)) < case["nreads"], rc.describe(case)
        cells = sum(w for _, w in rc.panel_windows(case)) * sum(case["Ns"])
        assert cells <= rc.PANEL_CELLS, (cells, rc.describe(case))
        assert np.any(np.isfinite(exp["ref"][0]["dist"])) or case["kind"] in ("empty", "beyond"), rc.describe(case)


# ---- event detection ---------------------------------------------------------------------------------------------------
def detect_trace(x, params):
    """detect_ref.marks with one counter added: (marks, silenced) -- silenced counts the times the short detector's peak
    above its threshold resets the long detector while that one holds a peak above its own threshold."""
    import detect_ref
    w_short, w_long, th_short, th_long, h = params
    n = len(x)
    ws, th = (int(w_short), int(w_long)), (float(th_short), float(th_long))
    t = (detect_ref.tstat(x, ws[0]), detect_ref.tstat(x, ws[1]))
    pos, val, valid, masked_to, out, silenced = [-1, -1], [np.inf, np.inf], [False, False], [-1, -1], [], 0
    for i in range(n):
        for k in (0, 1):
            if i <= masked_to[k]:
                continue
            cur = t[k][i]
            if pos[k] == -1:
                if cur < val[k]:
                    val[k] = cur
                elif cur - val[k] > h:
                    val[k] = cur
                    pos[k] = i
            else:
                if cur > val[k]:
                    val[k] = cur
                    pos[k] = i
                if k == 0 and val[0] > th[0]:
                    silenced += pos[1] != -1 and val[1] > th[1]
                    masked_to[1] = pos[0] + ws[0]
                    pos[1] = -1
                    val[1] = np.inf
                    valid[1] = False
                if val[k] - cur > h and val[k] > th[k]:
                    valid[k] = True
                if valid[k] and i - pos[k] > ws[k] // 2:
                    out.append(pos[k])
                    pos[k] = -1
                    val[k] = cur
                    valid[k] = False
    return out, silenced


def detect_features(case, exp):
    import detect_ref
    ws, wl = case["params"][:2]
    f = {"R=%d" % case["R"], "preset=" + case["preset"], "stride % 8 == 0" if case["stride"] % 8 == 0 else "stride % 8 != 0"}
    f |= {"kind=" + k for k in case["kinds"]}
    if ws == 1:
        f.add("w_short=1")
    if wl == 64:
        f.add("w_long=64")
    if ws == wl:
        f.add("w_short=w_long")
    off, rec = exp["off"], exp["rec"]
    for r, x in enumerate(case["reads"]):
        n = len(x)
        if n in rc.DET_LENS:
            f.add("len=%d" % n)
        for w in (ws, wl):
            for name, v in (("2w-1", 2 * w - 1), ("2w", 2 * w), ("2w+1", 2 * w + 1)):
                if n == v:
                    f.add("len=" + name)
        if n > rc.DET_LONG:
            f.add("len>8192")
        marks = rec["start"][off[r]:off[r + 1]][1:].astype(np.int64)      # the boundaries between events
        if not marks.size:
            continue
        if np.any(marks % rc.DET_WORD == 0):
            f.add("mark at a multiple of 64")
        if np.any(marks // rc.DET_WORD == (n - 1) // rc.DET_WORD):
            f.add("mark in the last word")
        if np.unique(marks // rc.DET_WORD).size < marks.size:
            f.add("two marks in one word")
        for k in range(1, n // rc.DET_ROUND):
            lo, hi = k * rc.DET_ROUND, (k + 1) * rc.DET_ROUND
            if hi <= n and not np.any((marks >= lo) & (marks < hi)) and np.any(marks < lo) and np.any(marks >= hi):
                f.add("a round without a mark between events")
    return f


DETECT_REQUIRED = ({"R=%d" % n for n in rc.DET_COUNTS} | {"len=%d" % n for n in rc.DET_LENS} |
                   {"len=2w-1", "len=2w", "len=2w+1", "len>8192", "stride % 8 == 0", "stride % 8 != 0", "w_short=1",
                    "w_long=64", "w_short=w_long", "preset=dna", "preset=rna", "preset=drawn", "kind=l", "kind=r", "kind=f",
                    "kind=p", "mark at a multiple of 64", "mark in the last word", "two marks in one word",
                    "a round without a mark between events"})


def test_detect_cases_reach_every_boundary(cases):
    assert len(cases["detect"]) >= 4
    have = set()
    for case, exp in cases["detect"]:
        have |= detect_features(case, exp)
        assert case["total"] <= rc.DET_SAMPLES
    assert not sorted(DETECT_REQUIRED - have)


def detect_silenced(case, most=40):
    """Reads (of the first `most` with levels) in which the short detector silences a long-detector peak above its
    threshold; the trace's marks are detect_ref's."""
    import detect_ref
    count = 0
    for x, k in list(zip(case["reads"], case["kinds"]))[:most]:
        if k in "lp" and 0 < len(x) <= 6000:
            marks, silenced = detect_trace(x, case["params"])
            assert marks == detect_ref.marks(x, case["params"])
            count += silenced > 0
    return count


def test_detect_cases_silence_a_long_mark_by_a_short_peak(cases):
    assert sum(detect_silenced(case) for case, _ in cases["detect"]) >= 1


# ---- signal HMM ------------------------------------------------------------------------------------------------------
def hmm_final_scores(case):
    """v[R, S] after the last used sample of every read (hmm_ref's recurrence), NaN rows for empty reads"""
    import hmm_ref
    S, linit, ltrans, c, mu, h = hmm_ref.model_arrays(case["model"])
    if case["feed"] == "batch":
        x = case["sig"].astype(np.float64)
        lens = case["lens"].astype(np.int64)
        if case["cal"] is not None:
            x = (x + case["cal"][:, :1]) * case["cal"][:, 1:]
    else:
        lens = np.array([len(r) for r in case["reads"]], dtype=np.int64)
        x = np.zeros((len(lens), max(1, int(lens.max(initial=0)))))
        for i, r in enumerate(case["reads"]):
            x[i, :len(r)] = r
    if case["limit"] > 0:
        lens = np.minimum(lens, case["limit"])
    v = np.full((len(lens), S), np.nan)
    for t in range(int(lens.max(initial=0))):
        act = lens > t
        e = hmm_ref.emission(c, mu, h, x[:, t])
        if t == 0:
            nv = linit[None, :] + e
        else:
            with np.errstate(invalid="ignore"):
                cand = v[:, :, None] + ltrans[None, :, :]
            b = cand[:, 0, :].copy()
            for i in range(1, S):
                b = np.where(cand[:, i, :] > b, cand[:, i, :], b)
            with np.errstate(invalid="ignore"):
                nv = b + e
        v[act] = nv[act]
    return v


def hmm_features(ora, case, exp):
    f = {"R=%d" % case["R"], "feed=" + case["feed"], "limit=%d" % case["limit"], "S=%d" % case["S"]}
    if case["integer"]:
        f.add("integer scores")
    if case["feed"] == "batch":
        f.add("calibrated" if case["calibrated"] else "raw")
        f.add("stride % 8 == 0" if case["stride"] % 8 == 0 else "stride % 8 != 0")
    if case["feed"] == "list" and 0 < case["nfloat"] < case["R"]:
        f.add("mixed list")
    if "SK_INGEST_MB" in case["env"]:
        f.add("SK_INGEST_MB")
    if "SK_HMM_SCRATCH_MB" in case["env"] and rc.hmm_slices(case) >= 3 and case["R"] >= 130:
        f.add("three slices at 130 reads")
    for r in case["reads"]:
        if len(r) in rc.HMM_LENS:
            f.add("len=%d" % len(r))
        if len(r) > 2000:
            f.add("len>2000")
    rec = exp["rec"]
    used = rec["n_used"] > 0
    v = hmm_final_scores(case)
    top = np.nanmax(np.where(np.isnan(v), -np.inf, v), axis=1)
    if np.any(used & np.isfinite(top) & ((v == top[:, None]).sum(axis=1) >= 2)):
        f.add("final-state tie")
        tied = used & np.isfinite(top) & ((v == top[:, None]).sum(axis=1) >= 2)
        assert np.all(rec["final_state"][tied] == np.argmax(v[tied] == top[tied, None], axis=1))      # the lower state
    if case["S"] >= 2 and used.any() and np.any(np.all(rec["enter"][used][:, :case["S"]] == -1, axis=0)):
        f.add("a state no path enters")
    if case["S"] == 6 and np.any(np.all(rec["enter"][used] >= 0, axis=1)):
        f.add("every state of a 6-state model in one read")
    n1 = np.concatenate([p[3]["n1"] for p in exp["parts"]] + [np.zeros(0, dtype=np.int32)])
    ln = np.concatenate([p[3]["length"] for p in exp["parts"]] + [np.zeros(0, dtype=np.int32)])
    if np.any(n1 > 0) and np.any(n1 < ln):
        f.add("both components win")
    if 0 < case["limit"] < 100000:
        full = rc.expect_hmm(ora, dict(case, limit=0))
        for idx, _, off, seg in full["parts"]:
            for k, r in enumerate(idx):
                g = seg[int(off[k]):int(off[k + 1])]
                if len(case["reads"][r]) > case["limit"] and np.any((g["start"] < case["limit"]) &
                                                                    (g["start"] + g["length"] > case["limit"])):
                    f.add("limit cuts a segment")
    return f


HMM_REQUIRED = ({"R=%d" % n for n in rc.HMM_COUNTS} | {"len=%d" % n for n in rc.HMM_LENS} |
                {"limit=%d" % n for n in (0, 1, 33, 129)} | {"S=1", "S=6"} |
                {"feed=batch", "feed=f64", "feed=list", "mixed list", "calibrated", "raw", "stride % 8 == 0",
                 "stride % 8 != 0", "integer scores", "SK_INGEST_MB", "three slices at 130 reads", "len>2000",
                 "final-state tie", "a state no path enters", "every state of a 6-state model in one read",
                 "both components win", "limit cuts a segment"})


def test_hmm_cases_reach_every_boundary(ora, cases):
    import hmm_path_ref
    assert len(cases["hmm"]) >= 4
    have = set()
    for case, exp in cases["hmm"]:
        have |= hmm_features(ora, case, exp)
        assert case["total"] <= rc.HMM_SAMPLES
        for idx, rec, off, seg in exp["parts"]:          # the reference keeps its own invariants, and both references agree
            hmm_path_ref.invariants(case["model"], rec, off, seg)
            assert rec.tobytes() == exp["rec"][idx].tobytes()
    assert not sorted(HMM_REQUIRED - have)


# ---- segment levels --------------------------------------------------------------------------------------------------
def levels_features(case, exp):
    f = {"route=" + case["route"]}
    if "max_segs" in case:                               # (the list form takes none: nothing is claimed for it)
        assert case["route"] != "list"
        f.add("max_segs=%d" % case["max_segs"])
    if case["lo"] < 0:
        f.add("negative lim_low")
    for r, (x, segs) in enumerate(zip(case["reads"], exp["segs"])):
        n = len(x)
        if n in rc.LEVELS_LENS:
            f.add("len=%d" % n)
        if n > rc.SEGLEV_LDS_COLS:
            f.add("read above SEGLEV_LDS_COLS")
        if "max_segs" in case and len(segs) > case["max_segs"]:
            f.add("more segments than max_segs=%d" % case["max_segs"])
        kept = np.flatnonzero((x > case["lo"]) & (x < case["hi"]))
        y = x[kept]
        if kept.size and kept.size < n // 2 + n // 4:
            f.add("a quarter of the samples dropped")
        for s, e in segs:
            w = y[s:e]
            f.add("span of even length" if len(w) % 2 == 0 else "span of odd length")
            if len(w) > rc.SEGLEV_LDS_COLS:
                f.add("segment above SEGLEV_LDS_COLS")
            if len(w) and w.min() < 0 < w.max():
                f.add("keys of both signs in a span")
            if len(w) >= 16 and 4 * np.unique(w).size <= len(w):
                f.add("tie-heavy span")
            if len(w) and kept[s] != s:
                f.add("raw_start differs from the filtered index")
    if case["route"] == "list" and 0 < case["nfloat"] < case["R"]:
        f.add("mixed list")
    return f


LEVELS_REQUIRED = ({"route=" + r for r in rc.LEVELS_ROUTES} | {"max_segs=%d" % n for n in rc.LEVELS_MAX_SEGS} |
                   {"len=%d" % n for n in rc.LEVELS_LENS} |
                   {"negative lim_low", "read above SEGLEV_LDS_COLS", "segment above SEGLEV_LDS_COLS",
                    "more segments than max_segs=1", "more segments than max_segs=2", "a quarter of the samples dropped", "span of even length",
                    "span of odd length", "keys of both signs in a span", "tie-heavy span",
                    "raw_start differs from the filtered index", "mixed list"})


def test_levels_cases_reach_every_boundary(cases):
    assert len(cases["levels"]) >= 4
    have = set()
    segments = 0
    for case, exp in cases["levels"]:
        have |= levels_features(case, exp)
        segments += sum(len(s) for s in exp["segs"])
    assert not sorted(LEVELS_REQUIRED - have)
    assert segments >= 10 * len(cases["levels"])         # spans to compare, not only whole reads


# ---- the screening scheme's switches ----------------------------------------------------------------------------------
def screen_features(case):
    env, plan = case["env"], rc.screen_plan(case)
    f = {"motifs=%d" % len(case["Ns"]), "QL=%s" % case["ql"], "hint=" + case["hint"], "scale=" + case["scale"],
         "limits=%d,%d" % (case["lo"], case["hi"]), "ck=%d" % case["ck"]}
    f |= {"N=%d" % N for N in case["Ns"] if N in rc.SCREEN_N}
    if any(N not in rc.SCREEN_N for N in case["Ns"]):
        f.add("N random")
    for key in ("SK_DTW_SORT_MIN", "SK_DTW_NOFUSE", "SK_DTW_NO_SIBLINGS", "SK_DTW_NO_EARLY"):
        if key in env:
            f.add(key)
    if case["stride"] > int(case["lens"].max()) and np.any(case["sig"][:, case["M"]:] != 0):
        f.add("stride > longest row, padding not zeros")
    if case["M"] == rc.screen_min_len(max(case["Ns"]), case["ck"]) and case["stride"] == case["M"]:
        f.add("rows at the threshold")
    if max(p["chunks"] for p in plan) >= 3:
        f.add("chunks>=3")
    for p in plan:
        f.add("L%d P%s0" % (p["L"], "=" if p["P"] == 0 else ">"))
    asked = case["hint"] == "on"
    hinted = [p for p in plan if p["hinted"]]
    if asked and any(p["L"] == 64 or p["R"] > rc.HINT_MAX_R or p["N"] < rc.HINT_MIN_N for p in plan):
        f.add("the gate switches the hint off")
    if case["hint"] == "default":
        assert not hinted
    if asked and hinted:
        for p in hinted:
            f.add("hint L%d R%%4=%d" % (p["L"], p["R"] % 4))
            f.add("hint L%d P%s0" % (p["L"], "=" if p["P"] == 0 else ">"))
            if p["chunks"] >= 3:
                f.add("hint + chunks>=3")
        if "SK_DTW_SORT_MIN" in env:
            f.add("hint + sorted order")
        if case["scale"] == "zscale":
            f.add("hint + zscale")
        if "SK_DTW_NOFUSE" in env:
            f.add("hint + SK_DTW_NOFUSE")
        if case["ck"] != 128:
            f.add("hint + ck=%d" % case["ck"])
        Ls = [p["L"] for p in plan]
        if len(plan) > 1 and all(a != b for a, b in zip(Ls, Ls[1:])):
            f.add("hint + a motif list that changes L")
    return f


SCREEN_REQUIRED = ({"hint L%d R%%4=%d" % (L, k) for L in (8, 16) for k in range(4)} |
                   {"L%d P%s0" % (L, c) for L in (8, 16, 64) for c in "=>"} |
                   {"hint L%d P%s0" % (L, c) for L in (8, 16) for c in "=>"} |
                   {"limits=%d,%d" % p for p in rc.SCREEN_LIMITS} | {"ck=%d" % c for c in rc.SCREEN_CK} |
                   {"QL=None", "QL=8", "QL=16", "QL=64", "hint=on", "hint=off", "hint=default", "scale=medmad",
                    "scale=zscale", "motifs=1", "motifs=2", "motifs=3", "N random", "SK_DTW_SORT_MIN", "SK_DTW_NOFUSE",
                    "SK_DTW_NO_SIBLINGS", "SK_DTW_NO_EARLY", "stride > longest row, padding not zeros",
                    "rows at the threshold", "chunks>=3", "the gate switches the hint off", "hint + sorted order",
                    "hint + chunks>=3", "hint + zscale", "hint + SK_DTW_NOFUSE", "hint + ck=64", "hint + ck=256",
                    "hint + a motif list that changes L"})


def test_screen_cases_reach_every_switch_combination(cases):
    """The combinations no other test of the suite has: the hint together with the sorted order, three chunks, zscale,
    SK_DTW_NOFUSE, a motif list that changes L, both other checkpoint distances; every R % 4 under both hinted layouts;
    P = 0 and P > 0 under every L; a case the gate itself keeps from the hint."""
    assert len(cases["screen"]) >= 4
    have = set()
    for case, _ in cases["screen"]:
        have |= screen_features(case)
        assert rc.SCREEN_MIN_READS <= case["R"] <= 700 and case["sig"].shape == (case["R"], case["stride"])
        assert case["stride"] >= rc.screen_min_len(max(case["Ns"]), case["ck"])      # every motif of the call is screened
        assert int(case["lens"].max()) == case["M"]
    assert not sorted(SCREEN_REQUIRED - have)
    assert any(p["L"] == 64 and p["R"] >= 9 for case, _ in cases["screen"] for p in rc.screen_plan(case))


def test_screen_cases_compare_nine_reads_in_ten_within_the_cell_budget(cases):
    """In every case the reads the reference leaves out (MAD or std 0) are under 10 %, few of the others have a path
    wider than the second tier's look-back (those take the exact retry, whatever the library does), and the oracle fills at
    most SCREEN_CELLS cells."""
    for case, exp in cases["screen"]:
        assert case["R"] * case["stride"] * sum(case["Ns"]) <= rc.SCREEN_CELLS, rc.describe(case)
        for N, want in zip(case["Ns"], exp["want"]):
            out = ~np.isfinite(want["dist"]) & (want["n"] > 0)
            assert 10 * int(out.sum()) < case["R"], rc.describe(case)
            wide = ~out & (want["end"] - want["start"] + 1 > 2 * N + N // 4 + 16)
            assert 8 * int(wide.sum()) < case["R"], (rc.describe(case), int(wide.sum()))


def test_the_screening_batch_has_two_rows_without_a_result():
    """randcases.screen_batch over every length of tests/test_gpu_screen_grid.py: the constant row and the one-sample row
    (unless the filter drops its sample) are the only ones with MAD = 0; one read at least has the full length; the
    lengths give the layout asked for."""
    seen = set()
    for L, R in rc.SCREEN_GRID:
        lengths = rc.screen_grid_lengths(L, R)
        assert lengths[0] == L * R and all(0 < N <= L * R for N in lengths)
        for N in lengths:
            M = rc.screen_min_len(N)
            assert M % 8 == 0 and 0 <= M - 4 * (N + N // 8 + 8 + 128) < 8
            assert rc.screen_shape(N, rc.SCREEN_MIN_READS, M, str(L)) == (L, R)
            if N in seen:
                continue
            seen.add(N)
            sig, lens, motif = rc.screen_batch(rc.SCREEN_MIN_READS, M, N, 70000 + N)
            h = rc.SCREEN_MIN_READS - rc.SCREEN_HOSTILE
            # (the rows of full length cannot have MAD 0 unless more than half of their samples are one value)
            full = np.flatnonzero(lens == M)
            top = np.array([np.bincount(sig[r] - sig[r].min()).max() for r in full])
            suspects = set(full[2 * top >= M - 8]) | set(np.flatnonzero(lens < M))
            assert full.size >= h and h + 9 in suspects
            bad = [r for r in sorted(suspects) if rc._np_mad_is_zero(sig[r, :lens[r]], 0, 1200)]
            assert set(bad) <= {h + 9, h + 13} and h + 9 in bad, (N, bad)
    assert {p for L, R in rc.SCREEN_GRID for p in [L * R - rc.screen_grid_lengths(L, R)[-1]]} >= {1, 4, 7, 8, 15, 32, 63}
    assert (rc.screen_min_len(8), rc.screen_min_len(256), rc.screen_min_len(512), rc.screen_min_len(1024)) == \
        (584, 1696, 2848, 5152)


def test_same_seed_same_case():
    for fam in rc.SEEDS:
        seed = rc.SEEDS[fam][0]
        a, b = rc.case_of(fam, seed), rc.case_of(fam, seed)
        assert rc.describe(a) == rc.describe(b)
        for key in ("reads", "rows", "motifs", "seqs"):
            if key in a:
                assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[key], b[key]))
        if "pairs" in a:
            assert a["pairs"].tobytes() == b["pairs"].tobytes() and rc.case_digest(a) == rc.case_digest(b)


def test_interleaved_sequence_is_what_it_claims():
    """>= 24 calls, all four families and the three older calls, sizes going up and down, repeats."""
    seq = rc.INTERLEAVE
    assert len(seq) >= 24
    assert {f for f, _ in seq} == {"sweep", "hits", "paths", "pull", "segment", "motifseq", "pa"}
    assert len(seq) - len(set(seq)) >= 4                 # calls that occur twice
    for fam, seed in seq:
        assert fam not in rc.SEEDS or seed in rc.SEEDS[fam]
    size = []
    for fam, seed in seq:
        case = rc.interleave_case(fam, seed)
        size.append(max(len(r) for r in case["reads"]) if "reads" in case else int(np.max(case["lens"])))
    turns = sum((b - a) * (c - b) < 0 for a, b, c in zip(size, size[1:], size[2:]))
    assert turns >= 8, size                              # the longest read of a call goes up and down
    first_paths = next(i for i, (f, _) in enumerate(seq) if f == "paths")
    assert any(f == "hits" and size[i] > max(size[:i]) for i, (f, _) in enumerate(seq) if i > first_paths)
    assert seq.index(seq[first_paths], first_paths + 1) > first_paths      # the first paths call comes again


def test_second_interleaved_sequence_is_what_it_claims():
    """>= 24 calls: the four newer families and both twins between older calls, the longest read going up and down, four
    calls or more occurring twice."""
    seq = rc.INTERLEAVE2
    assert len(seq) >= 24
    fams = {f for f, _ in seq}
    assert {"panel", "detect", "hmm", "levels", "background", "events"} <= fams
    assert len(fams & {"sweep", "hits", "paths", "pull", "segment", "motifseq", "pa"}) >= 4
    assert len(seq) - len(set(seq)) >= 4
    for fam, seed in seq:
        assert fam not in rc.SEEDS or seed in rc.SEEDS[fam]
        assert fam not in rc.TWIN_OF or seed in rc.SEEDS[rc.TWIN_OF[fam]]
    size = []
    for fam, seed in seq:
        case = rc.interleave_case(fam, seed)
        size.append(max(len(r) for r in case["reads"]) if "reads" in case else int(np.max(case["lens"])))
    turns = sum((b - a) * (c - b) < 0 for a, b, c in zip(size, size[1:], size[2:]))
    assert turns >= 8, size
    scr = [i for i, (f, _) in enumerate(seq) if f == "screen"]              # screening calls, one twice, not side by side
    assert len(scr) >= 3 and len({seq[i] for i in scr}) < len(scr) and all(b - a >= 2 for a, b in zip(scr, scr[1:]))
    new = [i for i, (f, _) in enumerate(seq) if f in ("panel", "detect", "hmm", "levels")]
    assert any(size[i] > max(size[:i]) for i in new[1:])                    # a newer family grows the shared buffers
    assert any(size[i] < size[i - 1] // 4 for i in new if i)               # and one runs in buffers left much larger


# ---- the dRNA segmenter, slow5 branch -----------------------------------------------------------------------------------
def _runs_of(mask):
    """Lengths of the in-band runs of a bool mask that an out-of-band sample follows."""
    m = np.concatenate([[False], np.asarray(mask, dtype=bool), [False]])
    d = np.flatnonzero(m[1:] != m[:-1])
    return [int(b - a) for a, b in zip(d[::2], d[1::2]) if b < len(mask)]


def drna_seams(case, mask):
    """Labels of the scan's seams in one read's band mask: from the sample-level trace of the reference scan (drna_trace)
    and, for the 64-sample windows of a lane, from the trips of the piece model (_drna_pieces); both are held to the oracle
    by tests/test_walk_model.py."""
    from test_walk_model import _drna_pieces, drna_trace
    p = case["params"]
    scan = (p["error"], p["no_err_thresh"], p["w"], p["window"], p["seg_dist"])
    net, sd = p["no_err_thresh"], p["seg_dist"]
    segs, ev = drna_trace(mask, *scan)
    f = set()
    closes = [e for e in ev if e[0] == "close"]
    for e in ev:
        if e[0] == "rearm" and e[1] % 64 in (0, 63):
            f.add("re-arm on the %s sample of a word" % ("last" if e[1] % 64 == 63 else "first"))
        elif e[0] == "free" and net % 64 and any(c[2] < e[1] < net < c[1] for c in closes):
            f.add("a piece cut by no_err_thresh in mid-word takes a sample it does not count")
        elif e[0] == "short":
            f.add("a run shorter than window")
        elif e[0] == "idle" and e[1] == sd:
            f.add("no stop at i - last_end = seg_dist")
        elif e[0] == "stop" and e[2] == sd + 1 and any(n >= max(p["window"], 1) for n in _runs_of(mask[e[1]:])):
            f.add("stop at i - last_end = seg_dist + 1 with a run behind it")
        elif e[0] == "close":
            _, i, start, end, prev_err, merged, gap, low, spent = e
            if low <= -2 and spent >= p["error"] + 2:
                f.add("err < 0 after two re-arms, then the larger budget spent")
            if merged and gap == sd - 1:
                f.add("merge at seg_dist - 1")
            if not merged and gap == sd:
                f.add("no merge at seg_dist")
            if spent > 64:
                f.add("more than 64 counted samples taken by one run")
    if len(segs) > case["max_segs"]:
        f.add("more segments than max_segs")
    if len(segs) == case["max_segs"] and closes and closes[-1][5]:
        f.add("max_segs segments and a merge into the last")
    if rc.drna_walk(case) == "runs":
        trips = []
        assert _drna_pieces(mask, *scan, trips=trips) == segs
        for t in trips:
            if t[0] == "close":
                _, pos, q, L, before, prev_err, counted = t
                if q in (0, 63):
                    f.add("closed at bit %d of the lane's window" % q)
                if prev_err > 0 and before:
                    f.add("end = i - prev_err inside one piece")
                if prev_err > q and not before:
                    f.add("end = i - prev_err across two pieces")
    return f


def drna_features(ora, case, exp):
    p, R, kept = case["params"], case["nreads"], exp["kept"]
    t0, t1, w, win, net = p["t_start"], p["t_end"], p["w"], p["window"], p["no_err_thresh"]
    lo, hi = p["lim_low"], p["lim_hi"]
    stats = rc.drna_route(case)
    f = {"R=%d" % R if R < 200 else "R>=200", "route=" + case["route"], "stats=" + stats, "walk=" + rc.drna_walk(case),
         "limits=(%d, %d)" % (lo, hi), "bins=%d" % (hi - lo - 1), "w=%d" % w, "error=%d" % p["error"],
         "seg_dist=%d" % p["seg_dist"], "std_scale=%g" % p["std_scale"]}
    assert rc.drna_walk(case, {"SK_DRNA_STEP": "1"}) == "step" and rc.drna_route(case, {"SK_DRNA_STEP": "1"}) != "one-look"
    if case["kind"] == "stride":
        f.add("stride=%d, t_start=0" % case["stride"])
        assert t0 == 0 and all(len(r) < t1 for r in case["reads"])
    if R % 64:
        f.add("dead lanes in the last wave")
    for a in range(0, R, 64):
        if len({(k - 1) // 64 for k in kept[a:a + 64] if k}) >= 3:
            f.add("a wave's reads end at three or more words")
    for x, k in zip(case["reads"], kept):
        n = len(x)
        if n in rc.DRNA_LENS:
            f.add("len=%d" % n)
        for d in (-1, 0, 1):
            if n == t0 + d and t0 > 0:
                f.add("len=t_start%+d" % d)
            if n == t1 + d:
                f.add("len=t_end%+d" % d)
        if n >= rc.DRNA_LONG:
            f.add("len>=70000")
        if n and not k:
            f.add("nothing kept")
        if 0 < k < t1:
            f.add("a read ends before t_end")
        if k and k == t0:
            f.add("t_start at the kept count")
        if 0 < k < t0:
            f.add("t_start beyond the kept count")
        if n > 1000 and 0.005 < 1 - k / n < 0.02:
            f.add("1 % of a read dropped")
        if n > 1000 and 0.2 < 1 - k / n < 0.3:
            f.add("25 % of a read dropped")
        if k > t1 and n >= rc.DRNA_TILE and t1 < (1 << 20):
            keep = (x > lo) & (x < hi)
            at = np.cumsum(keep)[rc.DRNA_TILE - 1::rc.DRNA_TILE]
            if t1 in at.tolist():
                f.add("kept count reaches t_end at a tile's end")
    # the gates of sk_launch_prep_i16
    if t1 in (16384, 16385):
        f.add("t_end=%d" % t1)
    if t0 == t1:
        f.add("t_start=t_end")
    if 1 <= hi - lo - 1 <= 2048 and 0 <= t0 < t1 <= 16384 and case["stride"] < (1 << 19):
        need = rc.drna_lds_bytes(case["stride"], hi - lo - 1, t1)
        assert (stats == "one-look") == (need <= rc.DRNA_LDS_GATE)
        if abs(need - rc.DRNA_LDS_GATE) <= 8:
            f.add("LDS need %s the gate" % ("at" if need <= rc.DRNA_LDS_GATE else "past"))
    else:
        assert stats != "one-look"
    # top
    tops = [t for t, k in zip(exp["top"], kept) if k > t0]
    if p["std_scale"] == 0:
        f |= {"std_scale=0, median %s" % ("integer" if t == int(t) else "ends in .5") for t in tops}
    if any(t > 32767 for t in tops):
        f.add("top > 32767")
    if p["std_scale"] < 0 and any(t <= lo for t in tops):
        f.add("nothing in band")
    if any(np.isnan(t) for t, k in zip(exp["top"], kept) if k):
        f.add("NaN band")
        assert all(not s for s, t in zip(exp["segs"], exp["top"]) if np.isnan(t))
    # the scan's parameters
    f.add("window " + ("= 0" if win == 0 else "= 1" if win == 1 else "< w" if win < w else "= w" if win == w else
                       "= k w" if win % w == 0 else "> w"))
    most = max(kept)
    f.add("no_err_thresh " + ("= 0" if net == 0 else "< 0" if net < 0 else "= 2^31 - 1" if net == rc.INT32_MAX else
                              "beyond the read" if net >= most else "on a multiple of 64" if net % 64 == 0 else "in mid-word"))
    if case["kind"] in ("mask", "crafted"):          # two-level reads: the band mask is the drawn bit pattern
        for x, t in zip(case["reads"], exp["top"]):
            assert len(x) < rc.DRNA_PREFIX or (rc.DRNA_IN < t < rc.DRNA_FAR and set(np.unique(x)) <= {rc.DRNA_IN, rc.DRNA_FAR})
    if case["kind"] == "crafted":
        for r in case["crafted_at"]:
            x = case["reads"][r]
            assert rc.DRNA_IN < exp["top"][r] < rc.DRNA_FAR and set(np.unique(x)) <= {rc.DRNA_IN, rc.DRNA_FAR}
            f |= drna_seams(case, x < exp["top"][r])
    return f


DRNA_REQUIRED = ({"R=%d" % n for n in rc.DRNA_COUNTS if n < 200} | {"R>=200"} | {"len=%d" % n for n in rc.DRNA_LENS} |
                 {"len=t_start%+d" % d for d in (-1, 0, 1)} | {"len=t_end%+d" % d for d in (-1, 0, 1)} |
                 {"route=" + r for r in rc.DRNA_ROUTES} | {"stride=%d, t_start=0" % s for s in rc.DRNA_STRIDES} |
                 {"limits=(%d, %d)" % l for l in rc.DRNA_LIMITS} | {"bins=2048", "bins=2049"} |
                 {"stats=one-look", "stats=prep<lds,win>", "stats=prep<mem,win>", "stats=prep<lds,all>", "stats=prep<mem,all>",
                  "walk=runs", "walk=step"} |
                 {"w=%d" % w for w in rc.DRNA_W} | {"error=%d" % e for e in rc.DRNA_ERROR} |
                 {"seg_dist=%d" % s for s in rc.DRNA_SEG_DIST} | {"std_scale=%g" % s for s in rc.DRNA_STD} |
                 {"window " + s for s in ("= 0", "= 1", "< w", "= w", "> w", "= k w")} |
                 {"no_err_thresh " + s for s in ("= 0", "< 0", "in mid-word", "on a multiple of 64", "beyond the read",
                                                 "= 2^31 - 1")} |
                 {"dead lanes in the last wave", "a wave's reads end at three or more words", "len>=70000", "nothing kept",
                  "a read ends before t_end", "t_start at the kept count", "t_start beyond the kept count",
                  "1 % of a read dropped", "25 % of a read dropped", "kept count reaches t_end at a tile's end",
                  "t_end=16384", "t_end=16385", "t_start=t_end", "LDS need at the gate", "LDS need past the gate",
                  "std_scale=0, median integer", "std_scale=0, median ends in .5", "top > 32767", "nothing in band", "NaN band",
                  "re-arm on the last sample of a word", "re-arm on the first sample of a word",
                  "a piece cut by no_err_thresh in mid-word takes a sample it does not count", "a run shorter than window",
                  "no stop at i - last_end = seg_dist", "stop at i - last_end = seg_dist + 1 with a run behind it",
                  "err < 0 after two re-arms, then the larger budget spent", "merge at seg_dist - 1", "no merge at seg_dist",
                  "more than 64 counted samples taken by one run", "more segments than max_segs",
                  "max_segs segments and a merge into the last", "closed at bit 0 of the lane's window",
                  "closed at bit 63 of the lane's window", "end = i - prev_err inside one piece",
                  "end = i - prev_err across two pieces"})


def test_drna_cases_reach_every_boundary(ora, cases):
    have, segments = set(), 0
    for case, exp in cases["drna"]:
        assert sum(len(r) for r in case["reads"]) <= rc.DRNA_SAMPLES, rc.describe(case)
        have |= drna_features(ora, case, exp)
        segments += sum(len(s) for s in exp["segs"])
        if case["kind"] == "crafted" and case["arg"] == "exact":      # no read of the case makes the call grow its columns
            assert max(len(s) for s in exp["segs"]) == case["max_segs"]
    assert not sorted(DRNA_REQUIRED - have)
    assert segments >= 100 * len(cases["drna"])


# ---- the dRNA segmenter, --signal branch ---------------------------------------------------------------------------------
def roll_features(ora, case, exp):
    p, R = case["params"], case["nreads"]
    w, lo_t, hi_t, sd = p["w"], p["lo_thresh"], p["hi_thresh"], p["seg_dist"]
    f = {"R=%d" % R, "route=" + case["route"], "path=" + rc.roll_route(case), "w=%d" % w, "std_scale=%g" % p["std_scale"],
         "shift=%d" % p["shift"]}
    assert rc.roll_route(case, {"SK_ROLL_TWO_KERNELS": "1"}) == rc.roll_route(case, {"SK_DRNA_STEP": "1"}) == "two-kernels"
    assert rc.roll_route(case, {"SK_ROLL_ONE_LOOK": "1"}) != "stream"
    if rc.roll_route(case) == "stream" and case["stride"] > rc.ROLL_LDS_LONG:
        assert rc.roll_one_lds(case["stride"], w) == 0
        f.add("redo list through scratch rows")
    if w > case["longest"]:
        f.add("w above every read")
    for x, k in zip(case["reads"], exp["kept"]):
        n = len(x)
        for name, v in (("0", 0), ("1", 1), ("w-1", w - 1), ("w", w), ("w+1", w + 1), ("2w", 2 * w)):
            if n == v:
                f.add("len=" + name)
        if n in rc.ROLL_CHUNK:
            f.add("len=%d" % n)
        if n >= rc.ROLL_LDS_LONG:
            f.add("len>35000")
        if n >= rc.ROLL_SCRATCH_LONG:
            f.add("len>2^17")
        if k < n:
            f.add("limits drop samples")
    for xy in exp["xy"]:
        if xy is not None and xy[0] < 0:
            f.add("negative result")
    if case["kind"] == "crafted":
        op = ora.RollParams(**{k: v for k, v in p.items() if not k.startswith("lim")})
        for x, want in zip(case["reads"], exp["xy"]):
            res, t, (mn, sdv, bot) = ora.drna_roll(ora.scale_outliers(x.astype(float), p["lim_low"], p["lim_hi"]), op,
                                                   want_t=True)
            segs, ev = rc.roll_scan(t, bot, sd)
            ok = [s for s in segs if lo_t <= s[1] - s[0] <= hi_t]
            assert res == want == ((ok[0][0] - p["shift"], ok[0][1] - p["shift"]) if ok else None)
            for e in ev:
                if e[0] == "equal":
                    f.add("t == bot " + ("inside a run" if e[2] else "outside a run"))
                elif e[0] == "merge" and e[1] == sd - 1:
                    f.add("merge at seg_dist - 1")
                elif e[0] == "new" and e[1] == sd:
                    f.add("no merge at seg_dist")
                elif e[0] == "open":
                    f.add("a run open at the end" + (" behind a segment" if segs else ""))
            for s in segs:
                for name, v in (("lo_thresh", lo_t), ("lo_thresh - 1", lo_t - 1), ("hi_thresh", hi_t),
                                ("hi_thresh + 1", hi_t + 1)):
                    if s[1] - s[0] == v:
                        f.add("a segment of " + name)
            if len(ok) and ok[0] is not segs[0]:
                f.add("first segment rejected by length, a later one accepted")
    return f


ROLL_REQUIRED = ({"R=%d" % n for n in rc.ROLL_COUNTS} | {"w=%d" % w for w in rc.ROLL_W} | {"std_scale=%g" % s for s in rc.ROLL_STD} |
                 {"len=" + s for s in ("0", "1", "w-1", "w", "w+1", "2w")} | {"len=%d" % n for n in rc.ROLL_CHUNK} |
                 {"route=list", "route=padded", "route=odd", "path=stream", "path=one-look", "path=two-kernels",
                  "redo list through scratch rows", "w above every read", "len>35000", "len>2^17", "limits drop samples",
                  "shift=0", "shift=1000", "negative result", "t == bot outside a run", "merge at seg_dist - 1",
                  "no merge at seg_dist", "a run open at the end", "a run open at the end behind a segment",
                  "a segment of lo_thresh", "a segment of lo_thresh - 1", "a segment of hi_thresh",
                  "a segment of hi_thresh + 1", "first segment rejected by length, a later one accepted"})


def test_roll_cases_reach_every_boundary(ora, cases):
    have, found = set(), 0
    for case, exp in cases["roll"]:
        assert sum(len(r) for r in case["reads"]) <= rc.DRNA_SAMPLES, rc.describe(case)
        have |= roll_features(ora, case, exp)
        found += sum(xy is not None for xy in exp["xy"])
    assert not sorted(ROLL_REQUIRED - have)
    assert found >= 5 * len(cases["roll"])


def test_roll_one_look_lds_restated():
    """randcases.roll_one_lds against the figures DESIGN.md gives for k_roll_one: rows of about 35 000 samples fit 160 KB."""
    assert rc.roll_one_lds(35000, 2000) and not rc.roll_one_lds(35008, 2000)
    assert not rc.roll_one_lds(1000, 65536) and rc.roll_one_lds(1000, 65535)
    assert rc.roll_stream_ok(30000, 12000, 0, 1200) and not rc.roll_stream_ok(30000, 12001, 0, 1200)


# ---- the dRNA families stay what they are: a later family or a change of the generators must not renumber or alter them ----
PINNED_DRNA = {
    "drna": {
        0: "905021223d8bc7fa02d0b5d6ffe11434c1675248cd033afbb72a0ef56773f60c",
        1: "c8efd62f262ecf6223d7f356ec76cf4a1da1c619693e591fa3be8b778bcdcaf0",
        2: "ac2570c9b20173d36e0b9e65906aaef32cde0648555df89d65f69d5be02bd003",
        3: "25188d7415fef0ccf03f52277584513b451745e7ae39ce72d6d644fabb076127",
        4: "fbd9ca14f53feed52047337f4a810cb9c735a85d4f4fd8ffae2d373a0827de37",
        5: "f843df0d9a1a98918ed917c2838c59495ed97bf20a24ebfa4343f563eb22714f",
        6: "c2909816528c1c9468b3a5e8c4b37d8acc6ae5449fe257d2ddc9193dd648cb59",
        7: "1dadab3fc904bac902545b386893eb2ef30910bf495e3e4536671fb46849c93b",
        8: "7153f3e4760c8821e578ed0311e2698be00625bdfdda87908bca7818c4bfdd17",
        10: "f0dc609d91bd048571b8262f986b9c0183e423fceabce0764202f5a29ec957de",
        11: "79803c7c601b2fbd133ba9f49ac86c96964ef281af96d07cc4fdf22ecc000448",
        14: "d73cc3f6ad0f746ac932219e11c58d0cb8e0b72fd813ed7c0a58840568712b32",
        15: "c4331c7668efbd62569446cfc345548fac582874945b3ea0610ea72899c9a8a7",
        17: "885f0b9e653ce0d882b47c7c55e40cd6d21d96299d5e52b4bfdab1483d1c7a05",
        18: "aa5a2766a70cf76acbc1feb3796912ba883ddd60f44c27590a0da7310a25b626",
        20: "cc46e094e0ca3272e69a0d2bda4860a21472c90432eee5930a5c30b1dd274f51",
        22: "f2222ada881e2a1d301d7f52d149be79b611cabd8c81ec335fec03c3e7cbff41",
        24: "0678ce47a523ef1b5c53725965de0b92f04a5e169892e486a09f264938f7423a",
        27: "2b15032219da0eccdf1d10436e65e7764a06b802593904c5080958c49bcc8f42",
        28: "53f7bf0cd9d821a4dee7b901a7e2aee47f4fda46bcfed945dec06985761949fd",
        29: "68b6b4fc2081cb5590d912df29cbb5034900bae4b9020b11fea63a6dcdcab5d9",
        30: "aef1d4eac9b5c10f0bf4fdce83b37d68669c22bdb9504fc0385aebefe4f67263",
        31: "eeba8f5b8b2b1de32679bbe98dcf7a2e02d16f77073053c5a87c9f4ab122dcf6",
        34: "3341c223753eff2e9cea847c39d8ff8ccbfc9e23a86fe9d1d124015299e893e9",
        35: "5cc1c9b6fd1b26231e98b43a875523516db5d44dc59de23647777be01f0dfe2b",
        36: "36bf030f72abeb78ec8a7e5dc388ee039e8a8f5c7346dfe5e726b3d31746b8f1",
        37: "ef65f82778015f5cf99cdafee6d066090e7489c8eef3406ef66cbbad574fdda9",
        38: "68626a03088d6f29cc8566f77dac463452bdbc2afdebc089024146e41b926ebc",
        39: "28f4557ce57d6c92d5db50f7d7cbc22fc7e3682448e20a5fb3e33b8718afb2bb",
        40: "2753c7b49819f229c9188847757c88c5fb346cc73f65be132d6d5503c1cda6b1",
        54: "e5a3da041916c5e3c3a46a62800601ef7eb41346a9796baa40baaa54e057daf7",
        56: "bb12df92500c7e6165a69ca9d5444513088fd6de26abba16919aac5d44fcf915",
        65: "affc2c7b431cf83218bf1bac20263511100388aad10e8d11e1391bda5728f6a2",
        66: "4a37bf5741cad8259f5fe94100a9e8fb9d610fb2d03b30658e4a424fd48d48c3",
        74: "4647fd38a561079ba9690a2aaa011bb64a0c33192eabc97822cac9c33c7442bd",
        116: "3ddb9cf6364995df9c9760ef906b510bfe84522309f995f1bcf288e4e4c81186",
        117: "5343bb02fef28e1e9c38cf682ec6e03d8040b68345085f07b4a730437558835b",
        140: "24bdc3ede8df580f4a426e35911bde0925c9e47bbd18eb770ede31b3105ab18e",
        170: "0709bfbad753619d12d7f339b63bc692bc1d1725bb1ac5c44813e21509a126ce",
        210: "8c392f1f4a11b696ed34e4ac139dfde82bd2a70c5dc323dff9a5e83524c91762",
    },
    "roll": {
        0: "88b5fa6950bb988e204efdbfc56d98ec9e2c0432ec3d04b80b53717e993b60dd",
        1: "1419196a609d8ed15762febaf11e8fc3e2acc6e7f425f6e370fd29797919c83e",
        2: "86660a49f8a14afe7841aa56c11b185a8d5b90e6ac1c4c1547397aa11f5f6b37",
        3: "9458fe6b94b8b7e64d6fe09782494690fcba67b3e6ceab694fe26f3df2f27741",
        4: "5afed6e662940734327a200e3c5989a08006c75ad38f1a92d8f4e3f7d37de10e",
        10: "e1043e5ca66b80b5417347f9c6f3e3cbaa3d9a81875a7e03abdac2c70c559374",
        11: "b9e1609168f7a916f642fac8baebc42a33698417e3aa368094a8749baf2ff34d",
        13: "6b3890a9ef6ee4b1615faacf658038b384fe3631c549f1793850395b59b90523",
        16: "e7abec7884634bb51c7c9cabfcbaf29c1bb84f2161b27b6e68b98eab20f0e6b4",
        21: "8917af4b9aa06634c0fbf87d28c68b9a88ebb5faeedade094c4b81095f54d389",
        23: "1c69647b62d3d19c46a61cf767f38a0903fb9b36d0f9a48182467fedb6ffebb4",
        24: "9ceadb852be1753c606d6a82932a2525a24d9b4f081f91de0d0b673f2f9e96ef",
        29: "fb40338895dca86cdf9dbec1f2c3026af2b46d55d7717a329f13cf4adb0f069c",
        31: "065c557da3d3e8d4502a102fe13784c51043bbc6b2208b727ceb697de226d99b",
        59: "3489bda94222d16b1f7828c47c1ef9441db26a9a803e53c9fcbbeebe4dde964d",
    },
}


def test_drna_families_keep_their_cases():
    assert (rc.FAMILY_INDEX["drna"], rc.FAMILY_INDEX["roll"]) == (9, 10)
    for fam, want in PINNED_DRNA.items():
        assert list(want) == rc.SEEDS[fam], fam
        for seed, digest in want.items():
            case = rc.case_of(fam, seed)
            assert rc.case_digest(case) == digest, (fam, seed)
            assert rc.describe(case).startswith("%s seed=%d kind=" % (fam, seed))


def test_third_interleaved_sequence_is_what_it_claims():
    """Both dRNA branches between segment, levels, hits and detect calls; of each branch a large case before a small one;
    calls that occur twice."""
    seq = rc.INTERLEAVE3
    fams = {f for f, _ in seq}
    assert fams == {"drna", "roll", "segment", "levels", "hits", "detect"}
    assert len(seq) - len(set(seq)) >= 4
    for fam, seed in seq:
        assert fam not in rc.SEEDS or seed in rc.SEEDS[fam]
    for fam in ("drna", "roll"):
        size = [sum(len(r) for r in rc.case_of(f, s)["reads"]) for f, s in seq if f == fam]
        assert any(b < a // 20 for a, b in zip(size, size[1:])), (fam, size)      # a small case in buffers left much larger
        assert any(b > 20 * a for a, b in zip(size, size[1:])), (fam, size)       # and one that grows them again
    assert all(a != b for (a, _), (b, _) in zip(seq, seq[1:]))                     # never the same family twice in a row


# ---- DTW over a pair list and its warping paths ------------------------------------------------------------------------
PAIRS_QUERY_LENGTHS = (1, 16, 17, 31, 32, 256, 257, 1023, 1024)
PAIRS_TIE_CELLS = 400_000                        # pairs up to here get their last row looked at for a tie


def pairs_features(ora, case, exp):
    seqs, pairs, env = case["seqs"], [tuple(p) for p in case["pairs"].tolist()], case["env"]
    plan = rc.pairs_plan(case)
    groups = plan["groups"]
    assert sum(g["count"] for g in groups.values()) == len(pairs) == case["npairs"]
    assert sorted(p for g in groups.values() for p in g["order"]) == list(range(len(pairs)))
    f = {"mode=" + case["mode"], "form=" + case["form"]}
    if case["form"] == "flat":
        values, off = rc.pairs_pool_of(case)
        assert off[0] == case["pad"] > 0 and off[-1] == values.size and np.all(np.isnan(values[:off[0]]))
    if len(pairs) > rc.PAIRS_SMALL_MAX and not env:
        assert case["kind"] == "natural" and max(len(seqs[t]) for _, t in pairs) <= rc.PAIRS_NATURAL_TARGET
        if any(L == 16 and R >= 3 for L, R in groups):
            f.add("natural: an L=16 group with R>=3")
        if all((16, R) in groups for R in range(1, 17)) and any(L == 64 for L, _ in groups):
            f.add("natural: all 16 L=16 groups beside L=64")
    if len(pairs) <= rc.PAIRS_SMALL_MAX:
        f.add("<=2048 pairs, " + ("SK_DTW_NO_SMALL" if "SK_DTW_NO_SMALL" in env else "plain"))
    if len(groups) >= 6:
        f.add(">=6 groups")
    for (L, R), g in groups.items():
        if g["count"] == 1:
            f.add("a group of one pair")
        if g["count"] % (64 // L):
            f.add("a group that ends inside a wavefront")
        for P in g["P"]:
            assert 0 <= P < L
            if P in (0, L - 1):
                f.add("P=" + ("0" if P == 0 else "L-1"))
        if L == 16:
            for k in range(0, g["count"], 4):
                M = g["M"][k:k + 4]
                assert M == sorted(M, reverse=True)
                if 0 in M and max(M) > 0:
                    f.add("an empty target beside live mates at L=16")
                if max(M) >= rc.PAIRS_CLIFF and any(m <= 3 for m in M):
                    f.add(">=3000 points beside <=3 in a wavefront")
    f |= {"N=%d" % len(seqs[q]) for q, _ in pairs if len(seqs[q]) in PAIRS_QUERY_LENGTHS}
    uses = np.bincount([q for q, _ in pairs])
    if uses.max() >= 3:
        f.add("a query in >=3 pairs")
    if any(q == t for q, t in pairs):
        f.add("(i, i)")
    if len(set(pairs)) < len(pairs):
        f.add("a pair repeated verbatim")
    for p, (q, t) in enumerate(pairs):
        N, M = len(seqs[q]), len(seqs[t])
        if M == 1:
            f.add("M=1")
        if 0 < M < N:
            f.add("M<N " + case["mode"])
        if M == N and q != t:
            f.add("M=N " + case["mode"])
        if case["ties"] and case["mode"] == "subsequence" and 0 < N * M <= PAIRS_TIE_CELLS and "tie" not in f:
            last = ora.dtw_subsequence(seqs[q], seqs[t], want_cost=True)[3][-1]
            if int((last == last.min()).sum()) >= 2:
                assert exp["want"]["end"][p] == int(np.argmin(last))                # the first minimum is the record's
                f.add("tie")
    return f


PAIRS_REQUIRED = ({"N=%d" % n for n in PAIRS_QUERY_LENGTHS} |
                  {"mode=subsequence", "mode=global", "form=list", "form=flat", "natural: an L=16 group with R>=3",
                   "natural: all 16 L=16 groups beside L=64", "<=2048 pairs, plain", "<=2048 pairs, SK_DTW_NO_SMALL",
                   ">=6 groups", "a group of one pair", "a group that ends inside a wavefront", "P=0", "P=L-1",
                   "a query in >=3 pairs", "(i, i)", "a pair repeated verbatim", "an empty target beside live mates at L=16",
                   "M=1", "M<N subsequence", "M<N global", "M=N subsequence", "M=N global",
                   ">=3000 points beside <=3 in a wavefront", "tie"})


def test_pairs_cases_reach_every_boundary(ora, cases):
    """Both modes and pool forms; the natural L = 16 route (more than 2 048 pairs, no switch) with every R of L = 16 beside
    L = 64 groups in one call; both switch routes below it; six groups and more, a group of one pair, one that ends inside
    a wavefront, P = 0 and P = L - 1; the query lengths at the layout's seams; repeats; empty, one-point, shorter and equal
    targets; a long target beside short ones in a wavefront; a tie on the last row.  The plan is randcases.pairs_plan."""
    assert len(cases["pairs"]) >= 4
    have = set()
    for case, exp in cases["pairs"]:
        have |= pairs_features(ora, case, exp)
        assert case["cells"] <= rc.PAIRS_CELLS and len(exp["want"]) == case["npairs"], rc.describe(case)
    assert not sorted(PAIRS_REQUIRED - have)


def pairpaths_features(case, exp):
    seqs, pairs, mode, kind = case["seqs"], case["pairs"].tolist(), case["mode"], case["records"]
    plan = rc.pairpaths_plan(case, exp["records"])
    traced, listed = plan["traced"], plan["listed"]
    f = {"mode=" + mode, "records=" + kind}
    scratch = "SK_PATH_LDS_BYTES" in case["env"]
    if case["tier"] == 0 and traced:
        words = {p: N * ((W + 15) // 16) for p, N, W in traced}
        width = {p: W for p, N, W in traced}
        if not listed:
            f.add("the LDS tier alone")
        if any(words[p] > rc.PP_LDS_WORDS for p in listed) and len(listed) < len(traced):
            f.add("listed by more than 6400 words")
        if mode == "global" and any(words[p] <= rc.PP_LDS_WORDS and width[p] > rc.PP_LDS_COLS for p in listed):
            f.add("listed by a global window above 1024 columns")
    if case["tier"] == 1 and traced:
        assert len(listed) == len(traced) and plan["waves"] == min(len(listed), rc.PP_MAX_WAVES)
        if len(listed) >= 2:
            f.add("every pair listed")
    if case["tier"] == 2 and traced:
        assert len(listed) == len(traced) and plan["waves"] == 1
        d = np.sign(np.diff(plan["W"]))
        if len(listed) >= 3 and (d > 0).any() and (d < 0).any():
            f.add("one wavefront, windows up and down")
    for p, N, W in traced:
        M = len(seqs[pairs[p][1]])
        if W % 16 in (0, 1, 15):
            f.add("W%%16=%d" % (W % 16))
        if N % 64 in (0, 1, 63):
            f.add("N%%64=%d" % (N % 64))
        if (N + 63) // 64 in (1, 2, 16):
            f.add("stripes=%d" % ((N + 63) // 64))
        if mode == "global" and M == 1:
            f.add("global M=1")
        if mode == "global" and N == 1:
            f.add("global N=1")
        if mode == "subsequence" and W == 1:
            f.add("subsequence: a window of one column")
    nan = np.isnan(exp["records"]["dist"])
    if kind == "tiles":
        assert mode == "subsequence" and not exp["mismatches"]
        if any(len(seqs[t]) > case["piece"] for _, t in pairs):
            f.add("tiles: a target of several pieces")
            if scratch:
                f.add("tiles: in the scratch tier")
        # the merged records are whole-target records wherever the whole-target match fits the overlap
        fits = ~nan & (exp["truth"]["end"] - exp["truth"]["start"] + 1 <= case["overlap"])
        assert np.array_equal(exp["records"]["dist"][fits], exp["truth"]["dist"][fits])
    if kind in ("own", "tiles") and nan.any() and not nan.all():
        assert np.all(exp["records"]["flags"][nan] == 1)
        f.add("empty-target records among good ones")
        if kind == "own" and mode == "global":
            f.add("empty-target records: global")
        if kind == "own" and scratch:
            f.add("empty-target records: scratch tier")
    if kind == "wrong" and exp["wrong"]:
        assert exp["mismatches"] == len(exp["wrong"]) <= case["nwrong"] and len(exp["wrong"]) < len(pairs)
        for p in exp["wrong"]:
            a, b = exp["records"][p], exp["truth"][p]
            M = len(seqs[pairs[p][1]])
            assert 0 <= a["start"] <= a["end"] < M and a["end"] == b["end"]        # inside the target
            assert (a["dist"] != b["dist"]) != (a["start"] != b["start"])         # one change per record
            f.add("wrong: dist by one ulp" if a["dist"] != b["dist"] else "wrong: start moved")
        f.add("wrong: " + mode)
        if scratch:
            f.add("wrong: scratch tier")
    return f


PAIRPATHS_REQUIRED = ({"W%%16=%d" % k for k in (0, 1, 15)} | {"N%%64=%d" % k for k in (0, 1, 63)} |
                      {"stripes=%d" % k for k in (1, 2, 16)} |
                      {"mode=subsequence", "mode=global", "records=computed", "records=own", "records=tiles", "records=wrong",
                       "the LDS tier alone", "listed by more than 6400 words", "listed by a global window above 1024 columns",
                       "every pair listed", "one wavefront, windows up and down", "global M=1", "global N=1",
                       "subsequence: a window of one column", "tiles: a target of several pieces",
                       "tiles: in the scratch tier", "empty-target records among good ones", "empty-target records: global",
                       "empty-target records: scratch tier", "wrong: dist by one ulp", "wrong: start moved",
                       "wrong: subsequence", "wrong: global", "wrong: scratch tier"})


def test_pairpaths_cases_reach_every_boundary(cases):
    """Both modes; records computed, the reference's own, merged tile records against whole targets, records with a
    handful changed; the LDS tier alone, pairs listed by their words and by a global window, every pair listed, one
    wavefront for a list whose windows go up and down; the windows, query lengths and stripe counts at the seams; and
    every reference passes pair_paths_ref.check_invariants."""
    import pair_paths_ref
    assert len(cases["pairpaths"]) >= 4
    have = set()
    for case, exp in cases["pairpaths"]:
        have |= pairpaths_features(case, exp)
        assert case["cells"] <= rc.PAIRS_CELLS and case["npairs"] <= rc.PP_MAX_WAVES, rc.describe(case)
        off, rec = exp["off"], exp["records"]
        for p in range(case["npairs"]):
            sp = exp["spans"][off[p]:off[p + 1]]
            if np.isnan(rec["dist"][p]) or p in exp["wrong"]:
                assert np.all(sp == -1), (rc.describe(case), p)
            else:
                pair_paths_ref.check_invariants(sp, case["mode"], rec["start"][p], rec["end"][p])
    assert not sorted(PAIRPATHS_REQUIRED - have)


def test_pair_references_stay_inside_the_budget(ora):
    """The reference of every committed case of either family, timed one by one: PAIRS_CELLS cells at the oracle's rate
    (150 M cells a second and more on one core) stay under 2 s with room to spare for a slower machine."""
    import time
    for fam in ("pairs", "pairpaths"):
        for seed in rc.SEEDS[fam]:
            case = rc.case_of(fam, seed)
            t0 = time.perf_counter()
            rc.EXPECT[fam](ora, case)
            assert time.perf_counter() - t0 < 2.0, rc.describe(case)


# ---- the pair families stay what they are -------------------------------------------------------------------------------
PINNED_PAIRS = {
    "pairs": {
        4: "f298d3fdd3ee0d2258e5127ad6d1f650b1a42ff7f6c572b96bca57a206c326f9",
        5: "91fd9d154b4805ca71410a6647a8a04ce01325c2e5e95edbf240f122cc62d5c2",
        7: "da10a6959f684f47935bbf0a457b3a756c05aedf15241dffcb7a1f737a92aa51",
        9: "ff8168cb67718f396fd8bd7d1c83236d9da57b2c63709c75bcf6ad9ceda21b91",
        23: "5615e1c6197dca89ec7d816c6aa70ecc8e0bd04798cbef7e5fb03c171837f4e6",
        54: "1199f293ef58d73ddc9235aff7fdf85d6b9ce0224bf019b17b2ff2dda24cd79f",
        119: "dbf5735ed43e3e4bd0b75bd55a82bd1600791e65be83a104a755f90a51fc9755",
        130: "51588b5ab46d399dbf0db7d34256a3a9ce843ca4e8c71996be39b21978449177",
        133: "5ed148d98d0a266a688d0e023b5530b3f5d475f92793c1e4e5592ef0fcc59ad9",
    },
    "pairpaths": {
        1: "8674aff0641370c848b59f221bb06df931f09a0a94bdc0c53e2d6ae2a9c84cb4",
        5: "10e36102ac944aaf036ffbb0df9fa22876b5c203e4cb78839293181a43838715",
        6: "07142cf7b721cee4bb37bdb8a4d8b71ee50a0822594ba7c1c817d41cdaf702bb",
        7: "91dfa94ff94aadb9ac03e16fd624f01acf8fc8bdc02feeccc789d2546889f4af",
        13: "8f25c28f9330a3bbfae0587c69721ad5b6987c973467c2d89a9c12cfb6466b21",
        17: "009ec2e709e48fe301985e101c77fa2ba4980e0486241b815b350133541889c2",
        21: "0ebc367519d15d5c5a42ddd8f784bfbfe8f8c73c58c4c504b57b195ea3887b7b",
        22: "e2ef8856d14c130390f64b9d1a8bbe20830158fad640b84caf6b9db435be6188",
        23: "305c0cfd9dae4ac06eecf8f5aac22f51ce7c9c0702c5ff95c2f1bc16201c0b43",
        36: "60e2bebb73995afc174f7557e8b25f74d02af045fe1658676a5184aef1b8059e",
        50: "99cb656e2ff7f69ba8472c3e124b0415a29d4ff9b52e02c661291f04bc8b7a18",
        145: "e85ebd97a5517f80374111bb7db6bc43e9ac9f177a9581b0b7285ab0eb391d5e",
    },
}


def test_pair_families_keep_their_cases():
    assert (rc.FAMILY_INDEX["pairs"], rc.FAMILY_INDEX["pairpaths"]) == (11, 12)
    assert [rc.FAMILY_INDEX[f] for f in ("hits", "paths", "pull", "sweep", "panel", "detect", "hmm", "levels", "screen",
                                         "drna", "roll")] == list(range(11))              # the older numbers stay
    for fam, want in PINNED_PAIRS.items():
        assert list(want) == rc.SEEDS[fam], fam
        for seed, digest in want.items():
            case = rc.case_of(fam, seed)
            assert rc.case_digest(case) == digest, (fam, seed)
            assert rc.describe(case).startswith("%s seed=%d kind=" % (fam, seed))
            assert set(case["env"]) <= {"SK_DTW_NO_SMALL", "SK_PATH_LDS_BYTES", "SK_PATH_SCRATCH_BYTES"} <= set(rc.SWITCHES)


def test_fourth_interleaved_sequence_is_what_it_claims():
    """Pair lists and pair paths between paths, events, hits, screen and segment calls; of each pair family a large case
    before a small one; calls that occur twice; an all-listed pair-path case directly before and after a paths case that
    puts its hits into the scratch tier; a pair-path case that counts mismatches directly before a paths case."""
    seq = rc.INTERLEAVE4
    fams = {f for f, _ in seq}
    assert fams == {"pairs", "pairpaths", "paths", "events", "hits", "screen", "segment"}
    assert len(seq) >= 24 and len(seq) - len(set(seq)) >= 6
    for fam, seed in seq:
        assert fam not in rc.SEEDS or seed in rc.SEEDS[fam]
        assert fam not in rc.TWIN_OF or seed in rc.SEEDS[rc.TWIN_OF[fam]]
    assert all(a != b for (a, _), (b, _) in zip(seq, seq[1:]))                    # never the same family twice in a row
    for fam in ("pairs", "pairpaths"):
        assert sum(f == fam for f, _ in seq) - len({s for f, s in seq if f == fam}) >= 2       # two of its cases come twice
        size = [rc.case_of(f, s)["cells"] for f, s in seq if f == fam]
        assert any(b < a // 20 for a, b in zip(size, size[1:])), (fam, size)      # a small case in buffers left much larger
        assert any(b > 20 * a for a, b in zip(size, size[1:])), (fam, size)       # and one that grows them again
    between = others = False
    for (fa, sa), (fb, sb), (fc, sc) in zip(seq, seq[1:], seq[2:]):
        if (fa, fb, fc) == ("pairpaths", "paths", "pairpaths"):
            a, b, c = rc.case_of(fa, sa), rc.case_of(fb, sb), rc.case_of(fc, sc)
            between |= (a["env"].get("SK_PATH_LDS_BYTES") == b["env"].get("SK_PATH_LDS_BYTES") ==
                        c["env"].get("SK_PATH_LDS_BYTES") == "0") and min(a["npairs"], c["npairs"]) >= 3
    assert between
    for (fa, sa), (fb, _) in zip(seq, seq[1:]):
        others |= fa == "pairpaths" and rc.case_of(fa, sa)["records"] == "wrong" and fb == "paths"
    assert others
    scr = [i for i, (f, _) in enumerate(seq) if f == "screen"]                 # a pair call directly behind every screening call
    assert len(scr) >= 3 and all(seq[i + 1][0] in ("pairs", "pairpaths") for i in scr)


# ---- adaptive-band DTW over a pair list ---------------------------------------------------------------------------------
from band_ref import NONFINITE                  # noqa: E402
BAND_LONG_STEPS = 6000                           # the longest pair of the older band tests has 5 999 anti-diagonals


def band_features(case, exp):
    """From the case and the statement's answer alone.  The three outcome classes of a pair with a target: a finite
    dist with a path, a NaN dist with a path (a NaN reached the pinned corner), lost (dist +inf, no path)."""
    import band_ref
    seqs, pairs, W = case["seqs"], [tuple(p) for p in case["pairs"].tolist()], case["W"]
    rec, off, spans = exp["records"], exp["off"], exp["spans"]
    assert len(rec) == case["npairs"] == len(pairs) <= rc.BAND_LIST and case["nseq"] == len(seqs) <= rc.BAND_POOL
    assert case["steps"] == sum(rc.band_steps(len(seqs[q]), len(seqs[t])) for q, t in set(pairs))
    assert case["longest"] == max(rc.band_steps(len(seqs[q]), len(seqs[t])) for q, t in pairs)
    if case["form"] != "list":
        values, voff = rc.pairs_pool_of(case)
        assert voff[0] == case["pad"] > 0 and voff[-1] == values.size and np.all(np.isnan(values[:voff[0]]))
    how = "paths" if case["paths"] else "records only"
    f = {"W=%d %s %s" % (W, case["end"], how), "form=" + case["form"],
         "SK_BAND_WAVES=%s" % case["env"].get("SK_BAND_WAVES", "unset")}
    lost = failed = 0
    for p, (q, t) in enumerate(pairs):
        N, M = len(seqs[q]), len(seqs[t])
        sp = spans[off[p]:off[p + 1]]
        assert sp.shape == (N, 2)
        for name, n in (("N", N), ("M", M)):
            if n in rc.BAND_EDGES:
                f.add("%s=%d" % (name, n))
            if n - W // 2 in (-1, 0, 1):
                f.add("%s=W/2%+d" % (name, n - W // 2))
        if M == 0:
            assert np.isnan(rec["dist"][p]) and rec["flags"][p] == band_ref.FLAG_EMPTY and np.all(sp == -1)
            continue
        if rc.band_steps(N, M) > BAND_LONG_STEPS:
            f.add(">6000 anti-diagonals")
        if q != t and np.all(seqs[q] == seqs[q][0]) and np.all(seqs[t] == seqs[t][0]) and min(N, M) > W // 2:
            f.add("a constant against a constant beyond W/2")
        if rec["flags"][p] & band_ref.FLAG_BAND_LOST:
            assert rec["dist"][p] == np.inf and (rec["start"][p], rec["end"][p]) == (-1, -1) and np.all(sp == -1)
            lost += 1
            f.add(how + ": lost")
        elif np.all(sp == -1):
            failed += 1
            f.add(how + ": a walk that fails")
        else:
            band_ref.check_invariants(sp, rec["end"][p])
            if np.isnan(rec["dist"][p]):
                assert case["end"] == "pinned"
                f.add(how + ": a NaN dist with a path")
            else:
                assert rec["dist"][p] < np.inf
                f.add(how + ": a finite dist with a path")
    assert exp["lost"] == lost and exp["mismatches"] == lost + failed, rc.describe(case)
    if case["nonfinite"] is None:
        assert lost == 0 and failed == 0, rc.describe(case)        # no finite input loses the corner (RANDOM_CASES_BAND.md)
    else:
        f.add("non-finite: " + case["nonfinite"])
    queries, targets = {q for q, _ in pairs}, {t for _, t in pairs}
    shape = {"shared": any(q in targets and any(t == q and qq != q for qq, t in pairs) for q in queries),
             "(i, i)": any(q == t for q, t in pairs), "repeated": len(set(pairs)) < len(pairs),
             "empty": any(len(seqs[t]) == 0 for _, t in pairs)}
    f |= {"list: " + k for k, v in shape.items() if v}
    if all(shape.values()):
        f.add("list: shared, (i, i), repeated and empty together")
    if len(pairs) == 1:
        f.add("a list of one pair")
    return f


BAND_REQUIRED = ({"W=%d %s %s" % (W, end, how) for W in (64, 128, 256) for end in ("pinned", "free")
                  for how in ("paths", "records only")} |
                 {"form=" + v for v in rc.BAND_FORMS} | {"SK_BAND_WAVES=%s" % (v or "unset") for v in rc.BAND_WAVES} |
                 {"%s=%d" % (a, n) for a in "NM" for n in rc.BAND_EDGES} |
                 {"%s=W/2%+d" % (a, d) for a in "NM" for d in (-1, 0, 1)} |
                 {"paths: a finite dist with a path", "paths: a NaN dist with a path", "paths: lost", "records only: lost",
                  "paths: a walk that fails", "list: shared, (i, i), repeated and empty together", "a list of one pair",
                  "a constant against a constant beyond W/2", ">6000 anti-diagonals"} |
                 {"non-finite: " + v for v in NONFINITE})


def test_band_cases_reach_every_boundary(cases):
    """All 12 (W, end, paths) calls, the three pool forms, every SK_BAND_WAVES value; with paths the three outcome classes
    and without them a lost record; a list with a shared sequence, an (i, i) pair, a repeated pair and an empty target;
    and a list of one pair; every edge length as N and as M; constants against each other beyond the half band; a pair
    above 6 000 anti-diagonals; every non-finite kind, and a walk that leaves the band (counted, though the corner was
    not lost).  Without a non-finite value no pair is lost and no walk fails."""
    assert len(cases["band"]) >= 12
    have = set()
    for case, exp in cases["band"]:
        have |= band_features(case, exp)
        assert case["steps"] <= max(rc.BAND_STEPS, case["longest"]), rc.describe(case)
    assert not sorted(BAND_REQUIRED - have)
    assert sum(exp["mismatches"] for case, exp in cases["band"] if case["paths"]) > 0


def test_band_references_stay_inside_the_budget(ora):
    """The statement on every committed case, timed one by one: BAND_STEPS anti-diagonals at 35 to 45 microseconds each
    stay under 2 s with room for a slower machine (tests/RANDOM_CASES_BAND.md has the times)."""
    import time
    for seed in rc.SEEDS["band"]:
        case = rc.case_of("band", seed)
        t0 = time.perf_counter()
        rc.EXPECT["band"](ora, case)
        assert time.perf_counter() - t0 < 2.0, rc.describe(case)


PINNED_BAND = {
    27: "a948bc6592b0a81021cdb5a8d414bde0ffe1bfd759d31881758222d29fb72da0",
    29: "b3fdc1970d5bbf9ffcb5b20e8d578fc5a35e175709e6cac662b64246a14de7f8",
    44: "105b94b82bd50879eb2602793d2c033c52a4a5f6b44245168568049a386d8a97",
    54: "8bfbfbae94127ef9490e18f4bf844095910eab19bad26eebd0a485ae1c407ec4",
    61: "32311bbe505dba175be17d3318b5292a764e51c83bebb1549aa4f6f406069309",
    70: "2773fe8be1e9b1d457d9852d36625c4fa0f130cfbcdbb01bbec0d97b6fd7a3ac",
    75: "57a97cb81e3817c0e7193126237d51dddc82e79b1347397d5f4c97693408107e",
    112: "ea361cfae51a61063814b4cc7c9a3e02be65d2a7ee58efe3f808b19783f98106",
    138: "6f83b0f8c42bcb2fac1573edb4d4149bc971c1686ec655470e2174bb2dd38b6e",
    195: "f000435ffc8f9b3c71c67d98f7cb61ad3fc20946d99189e7e7aa65d9a841437c",
    238: "5a1b35c96fb4970e01d67f02bebf69b212748b258167c1912a5ae4324bb3bd91",
    240: "40b9bcfcfea7c734da48d7f6012f4d84b15f99687a30dc21f82943f0c56bfc6a",
    297: "e9260a83638589e5db86b7afbf999786232fda6f73f4d8a2c3aa3ad87a50fbc5",
    299: "fd863a3ea01cd09240a026bda6a47a82c0f967183e3006e94abc76e87d9c7116",
    331: "8df9bc53056cff0b2bbe94300faf42b25809b174f22f8be7cbeaa8b67c369bea",
    351: "e39b2f15f47a26d1e4c7519e8f9709fbb3cc1960ead490bb15d341b250242225",
    423: "48683d6668712253fe0607df669b4c2f9348fd62cf4a15762edb535dbfeb478f",
    458: "07111f3946cc07a40dbe00906fc0e1ff13c0abe1aebf7eb90988fc2aefa61620",
}


def test_band_family_keeps_its_cases():
    assert rc.FAMILY_INDEX["band"] == 13 and rc.SWITCHES[-1] == "SK_BAND_WAVES"
    assert [rc.FAMILY_INDEX[f] for f in ("hits", "paths", "pull", "sweep", "panel", "detect", "hmm", "levels", "screen",
                                         "drna", "roll", "pairs", "pairpaths")] == list(range(13))     # (they stay)
    assert list(PINNED_BAND) == rc.SEEDS["band"]
    for seed, digest in PINNED_BAND.items():
        case = rc.case_of("band", seed)
        assert rc.case_digest(case) == digest, seed
        assert rc.describe(case).startswith("band seed=%d W=" % seed) and set(case["env"]) <= {"SK_BAND_WAVES"}


def test_fifth_interleaved_sequence_is_what_it_claims(cases):
    """Band lists between pairs, pairpaths and hits cases, never two of a family in a row; band cases that come twice; a
    call that counts mismatches directly before one of the other kind that must count none, both ways round; the widest
    slabs before a list of one short pair and again after it."""
    seq = rc.INTERLEAVE5
    assert {f for f, _ in seq} == {"band", "pairs", "pairpaths", "hits"}
    assert all(fam not in rc.SEEDS or seed in rc.SEEDS[fam] for fam, seed in seq)
    assert all((a == "band") != (b == "band") for (a, _), (b, _) in zip(seq, seq[1:]))
    band = [s for f, s in seq if f == "band"]
    assert len(band) - len(set(band)) >= 3
    counted = {case["seed"]: exp["mismatches"] if case["paths"] else None for case, exp in cases["band"]}
    wrong = {case["seed"]: exp["mismatches"] for case, exp in cases["pairpaths"]}
    steps = list(zip(seq, seq[1:]))
    assert any(fa == "pairpaths" and wrong[sa] > 0 and fb == "band" and counted[sb] == 0 for (fa, sa), (fb, sb) in steps)
    assert any(fa == "band" and (counted[sa] or 0) > 0 and fb == "pairpaths" and wrong[sb] == 0 for (fa, sa), (fb, sb) in steps)
    slab = [rc.band_slab_bytes(max(rc.case_of("band", s)["longest"], 1), rc.case_of("band", s)["W"]) for s in band]
    assert any(b < a // 20 for a, b in zip(slab, slab[1:])) and any(b > 20 * a for a, b in zip(slab, slab[1:])), slab


# ---- signal HMM posteriors ----------------------------------------------------------------------------------------------
# the seeds chosen for the two labels that need impossible reads; every other committed case is held to the 90 % cap
HMMPOST_IMPOSSIBLE_SEEDS = (22, 68, 339)
HMMPOST_MIXED_CASES = 4


def hmmpost_features(case, exp):
    """(labels, stats) from the case and the statement's answer alone.  stats: reads with samples, the possible ones among
    them, whether the case counts as "mixed" (S >= 4, and at least half of all used samples lie in a possible read and
    have max_j gamma_j(t) < 0.999)."""
    import hmm_post_ref
    from hmm_ref import model_arrays
    post, cnt, goff, gamma = exp["post"], exp["counts"], exp["goff"], exp["gamma"]
    R, S, env = case["R"], case["S"], case["env"]
    x, used = rc.hmmpost_rows(case)
    assert np.array_equal(post["n_used"], used) and case["total"] <= rc.POST_SAMPLES and case["longest"] <= rc.POST_LONGEST
    assert case["total"] == sum(len(r) for r in case["reads"]) and case["longest"] == max(len(r) for r in case["reads"])
    B = rc.post_block_of(env)
    f = {"R=%d" % R, "S=%d" % S, "integer" if case["integer"] else "real", "block=%s" % env.get("SK_HMM_POST_BLOCK", "unset"),
         "counts=%d dense=%d" % (case["counts"], case["dense"])}
    f |= {"n_used=%d" % n for n in set(used.tolist()) if n in rc.POST_LENS}
    if case["feed"] == "batch":
        assert (case["stride"] % 8 == 0) == case["aligned"]
        f.add("batch %s %s" % ("aligned" if case["aligned"] else "unaligned", "calibrated" if case["calibrated"] else "raw"))
    elif case["feed"] == "f64":
        assert case["nfloat"] == int((np.array([len(r) for r in case["reads"]]) > 0).sum())
        f.add("feed=f64")
    elif 0 < case["nfloat"] < R:
        f.add("feed=list, integer and float reads")
    if B == 128 and used.max(initial=0) > 19 * 128:
        f.add("20 blocks at B = 128")
    if env.get("SK_HMM_POST_BLOCK") == "4096" and 0 < used.max(initial=0) < 4096:
        f.add("4096: every read shorter than the block")
    if "SK_HMM_SCRATCH_MB" in env:
        f |= {"%d slices" % k for k in (2, 3) if rc.hmmpost_slices(case) >= k}
    if "SK_INGEST_MB" in env and rc.hmmpost_sub_batches(case) >= 2:
        f.add("2 sub-batches")
    lens = np.array([len(r) for r in case["reads"]])
    if np.any(used < lens) and np.any((used == lens) & (lens > 0)):
        f.add("the limit cuts some reads and not others")
    live = (post["flags"] == 0) & (used > 0)
    dead = post["flags"] != 0
    assert not np.any(dead & (used == 0)) and np.all(np.isfinite(post["loglik"][live])) and np.all(post["loglik"][dead] == -np.inf)
    lanes = 0                                                             # possible reads in a group that has both kinds
    if case["feed"] != "list" and rc.hmmpost_sub_batches(case) == 1:      # (reads r and r + 1 share a wavefront by r // 64)
        for g in range(0, R, 64):
            if live[g:g + 64].any() and dead[g:g + 64].any():
                f.add("a group of 64 with possible and impossible reads")
                lanes = max(lanes, int(live[g:g + 64].sum()))
    for r in np.flatnonzero(dead & (used >= 3))[:8]:
        if hmm_post_ref.posterior_rows(case["model"], x[r:r + 1], [2], counts=False, dense=False)[0]["flags"][0] == 0:
            f.add("a possible prefix of an impossible read, n >= 3")
    if np.any(live[:, None] & (post["occ"][:, :S] == 0.0)):
        f.add("a possible read with a state of occ 0.0")
    if np.any(live[:, None] & (cnt["n"][:, :S, 0] > 0) & (cnt["n"][:, :S, 1] > 0)):
        f.add("both components win in one read")
    _, _, _, c, mu, h = model_arrays(case["model"])
    at = np.arange(x.shape[1])[None, :] < used[:, None]
    with np.errstate(invalid="ignore"):
        a0 = c[:, 0] - ((x[..., None] - mu[:, 0]) * (x[..., None] - mu[:, 0])) * h[:, 0]
        a1 = c[:, 1] - ((x[..., None] - mu[:, 1]) * (x[..., None] - mu[:, 1])) * h[:, 1]
    if np.any(at[..., None] & (a1 == a0) & np.isfinite(a0)):
        assert case["integer"]
        f.add("a1 == a0")
    top = gamma[:, :S].max(axis=1, initial=0.0)
    row_live = np.repeat(live, used)
    inner = (gamma[:, :S] > 0.0) & (gamma[:, :S] < 1.0)
    for r in np.flatnonzero(live):
        g = gamma[goff[r]:goff[r + 1], :S]
        if np.any(g == 0.0) and inner[goff[r]:goff[r + 1]].any():
            f.add("an exact 0.0 beside values inside (0, 1)")
            break
    assert not gamma[:, S:].any() and not gamma[~row_live].any() and not np.isnan(gamma).any()
    mixed = S >= 4 and len(top) > 0 and 2 * int((row_live & (top < 0.999)).sum()) >= len(top)
    return f, dict(reads=int((used > 0).sum()), possible=int(live.sum()), mixed=bool(mixed), lanes=lanes)


HMMPOST_REQUIRED = ({"R=%d" % n for n in rc.HMM_COUNTS} | {"n_used=%d" % n for n in rc.POST_LENS} |
                    {"S=%d" % s for s in range(1, 7)} | {"integer", "real", "feed=f64", "feed=list, integer and float reads"} |
                    {"batch %s %s" % (a, c) for a in ("aligned", "unaligned") for c in ("calibrated", "raw")} |
                    {"block=%s" % (b or "unset") for b in rc.POST_BLOCKS} |
                    {"counts=%d dense=%d" % (c, d) for c in (0, 1) for d in (0, 1)} |
                    {"20 blocks at B = 128", "4096: every read shorter than the block", "2 slices", "3 slices",
                     "2 sub-batches", "the limit cuts some reads and not others",
                     "a group of 64 with possible and impossible reads", "a possible prefix of an impossible read, n >= 3",
                     "a possible read with a state of occ 0.0", "both components win in one read", "a1 == a0",
                     "an exact 0.0 beside values inside (0, 1)"})
HMMPOST_IMPOSSIBLE_LABELS = ("a group of 64 with possible and impossible reads", "a possible prefix of an impossible read, n >= 3")


def test_hmmpost_cases_reach_every_boundary(cases):
    """Every read count, every length of POST_LENS as some read's n_used, S = 1 .. 6, integer and real-valued models, every
    feed (the batch aligned and unaligned, each calibrated and raw), every SK_HMM_POST_BLOCK setting, a read of 20 blocks
    at B = 128 and a case under 4096 whose reads are all shorter than the block, two and three slices, two ingest
    sub-batches, a limit that cuts some reads only, the four (counts, dense) calls; possible and impossible reads in one
    wavefront, an impossible read with a possible prefix; an unreachable state in a possible read, both components
    winning within a read, a1 == a0, an exact 0.0 beside values inside (0, 1); and HMMPOST_MIXED_CASES cases with S >= 4
    in which at least half of all samples have max_j gamma_j(t) < 0.999.  Outside HMMPOST_IMPOSSIBLE_SEEDS nine reads in
    ten with samples are possible, and over all cases at least 2 000 reads are possible and not empty -- also when the
    cases of POST_MANY short reads are left out.  The wavefront with both kinds of reads is reached by two cases at the
    least, in one of them with four possible reads or more (a case has impossible reads only where every path of its
    model ends, so its possible reads have at most S samples and are few among lengths drawn up to 70 and more)."""
    assert 12 <= len(cases["hmmpost"]) <= 24 and set(HMMPOST_IMPOSSIBLE_SEEDS) <= set(rc.SEEDS["hmmpost"])
    have, mixed, possible, ordinary, lanes = set(), 0, 0, 0, []
    for case, exp in cases["hmmpost"]:
        f, st = hmmpost_features(case, exp)
        have |= f
        mixed += st["mixed"]
        possible += st["possible"]
        ordinary += st["possible"] if case["R"] <= max(rc.HMM_COUNTS) else 0
        lanes += [st["lanes"]] if st["lanes"] else []
        if case["seed"] in HMMPOST_IMPOSSIBLE_SEEDS:
            assert f & set(HMMPOST_IMPOSSIBLE_LABELS), rc.describe(case)
        else:
            assert 10 * st["possible"] >= 9 * st["reads"], (rc.describe(case), st)
    assert not sorted(HMMPOST_REQUIRED - have)
    assert mixed >= HMMPOST_MIXED_CASES and possible >= 2000, (mixed, possible)
    # ... and not through the cases of POST_MANY reads of 0 .. 12 samples alone: as many among the cases of HMM_COUNTS
    assert ordinary >= 2000, ordinary
    # the group with both kinds of reads rests on more than one case and on more than one possible read in it
    assert len(lanes) >= 2 and max(lanes) >= 4, lanes


def test_hmmpost_references_stay_inside_the_budget():
    """The statement on every committed case, timed one by one: POST_SAMPLES samples and POST_LONGEST time steps stay under
    3 s with room for a slower machine (tests/RANDOM_CASES_HMMPOST.md has the times)."""
    import time
    for seed in rc.SEEDS["hmmpost"]:
        case = rc.case_of("hmmpost", seed)
        t0 = time.perf_counter()
        rc.EXPECT["hmmpost"](None, case)
        assert time.perf_counter() - t0 < 3.0, rc.describe(case)


def test_hmmpost_statement_by_classes_is_the_one_call():
    """expect_hmmpost calls the statement once per class of randcases.hmmpost_classes (short rectangles in place of the wide
    one: the CPU time of 8 400 short reads beside one of 130 samples falls sevenfold).  Every read's arithmetic is its own,
    so the bytes are those of one call over all reads: asserted on three committed cases that fall into several classes,
    a batch of 8 400 reads, a calibrated batch and a mixed list."""
    for seed in (22, 34, 37):
        case = rc.case_of("hmmpost", seed)
        parts = rc.hmmpost_classes(rc.hmmpost_rows(case)[1])
        assert len(parts) >= 2 and sorted(np.concatenate(parts).tolist()) == list(range(case["R"])), rc.describe(case)
        one, whole = rc.expect_hmmpost(None, case), rc.expect_hmmpost(None, case, whole=True)
        assert all(one[k].dtype == whole[k].dtype and one[k].tobytes() == whole[k].tobytes() for k in whole), rc.describe(case)


PINNED_HMMPOST = {
    2: "c3be055e3107ddb68c979ffb9b3e7b329de437e39ddfba0465a8dd24f5c4e7d3",
    8: "ae0ed0e2a993f72efb6a5a0ff41742ba0048ef81e9a5d64d2fda4a2e485bd2b9",
    21: "9ec3b96a0b3a769489749d252ddd90540a38349ccb0f043403d6da057fc72d16",
    22: "3076e13e18a3d4ca0dd73cbebcd1336586e243558fa09a645b00d9ecc7f61109",
    31: "c47f114ad41dd9d59a36b55eaa24e89dc2f67dd6c667cce2e4ba9d1fe3f73d91",
    34: "bd5aa16bb987d7afba355555c0d1bc15d8bd42ef0badf1d900cd1d6059d87021",
    37: "2e976b4767da6bc67f5d8a50deb798eb56bef4b16644d2a4f73a6e906d814f20",
    48: "c5efd520e99019c80d6e597ca6841dd16807dd9e28f75a230ba793c7411b7077",
    68: "6270a1803c908c6104b63e3e62ce13553568578ccd4a5c9de2108145d2db5d24",
    77: "862c0ced2f190c9cf178327276b6e3e6e61ed6a4b01724b1bfad39161c6157a2",
    124: "e9f68ac8b790d9e047981b6cb0a0425e5b9eadcc3782c003c5cc1dbe742a6a12",
    137: "f4edfda1a03261c7a044e01603f029cfade24b0de89fc2c35074b08aa56228ce",
    148: "3ed3272a2065c188ee2b60e0885314c811b7940bc5c151c72fa66215b1347260",
    162: "0fd449fdced58a4ccedfa886cc97b2ba09f8c64740919352cc0bcacaf132a6c9",
    185: "be327027757d85b5be490af3a0cbc9352a6b7de72ac3c4d55b6a0db4ff4188ff",
    215: "e49dce7958f7dc1edd4ddd669887889c48564b2811c8427463f28aaab9865b30",
    217: "65579ee21f7a053cf70cf25a51d021bbdcab77e756a96e62b7a69831432e1340",
    239: "bb36e3b9cb15811a7b4603a92736791b9103cd9aa1d5dc66f75f37513bc07ba7",
    305: "cdac25454e5c02998888ed0d1381d4de33d40731ae7c0d06b76a8f2ed454463f",
    339: "189ab78722dc67d81d3f1ed280b69b716017ba8377177f567e9a1be12cc53f3d",
    427: "75f9ea0051e3a5916b699c122c8eb89ebef81020fa94da9f1024e66098606756",
    465: "af8cb7bfe2fd0815b7a7bbffa3e8905b71af8d0aa142a87d3c5ffc97618941cb",
}


def test_hmmpost_family_keeps_its_cases():
    assert rc.FAMILY_INDEX["hmmpost"] == 14 and "SK_HMM_POST_BLOCK" in rc.SWITCHES
    assert list(PINNED_HMMPOST) == rc.SEEDS["hmmpost"]
    for seed, digest in PINNED_HMMPOST.items():
        case = rc.case_of("hmmpost", seed)
        assert rc.case_digest(case) == digest, seed
        assert rc.describe(case).startswith("hmmpost seed=%d R=" % seed)
        assert set(case["env"]) <= {"SK_HMM_POST_BLOCK", "SK_HMM_SCRATCH_MB", "SK_INGEST_MB"}


def test_hmmpost_hand_made_case_holds_both_kinds_of_reads_lane_by_lane(cases):
    """randcases.hmmpost_both_kinds out of seed POST_BOTH_SEED: one call, one sub-batch, and in its first group of 64 a
    possible read in every even lane, an impossible one in every odd lane; at least 20 of the possible ones have two
    samples, so that they take a forward step, a backward step and a transition count beside lanes that are dead."""
    case, exp = next((c, e) for c, e in cases["hmmpost"] if c["seed"] == rc.POST_BOTH_SEED)
    made = rc.hmmpost_both_kinds(case, exp)
    post = rc.expect_hmmpost(None, made)["post"]
    assert made["R"] == rc.POST_BOTH_READS == 65 and rc.hmmpost_sub_batches(made) == 1 and made["sig"].shape[0] == 65
    live, dead = (post["flags"] == 0) & (post["n_used"] > 0), post["flags"] != 0
    assert live[0::2].all() and dead[1::2].all() and int((post["n_used"][:64][live[:64]] >= 2).sum()) >= 20
    assert np.all(post["n_used"][dead] >= 3) and made["total"] == sum(len(r) for r in made["reads"]) <= case["total"]


def test_diff_hmmpost_reports_an_unclean_device_call_whatever_it_returned():
    """The fifth entry of what hmmpost_device_call returns (nothing written behind an output, nothing at all to a buffer
    that was not asked for) is looked at with and without counts and dense rows; a host call has no fifth entry."""
    case = rc.case_of("hmmpost", 427)
    exp = rc.expect_hmmpost(None, case)
    full = (exp["post"].copy(), exp["counts"].copy(), exp["goff"].copy(), exp["gamma"].copy())
    bare = (exp["post"].copy(), None, None, None)
    for got in (full, bare):
        assert rc.diff_hmmpost(case, got, exp) is None and rc.diff_hmmpost(case, got + (True,), exp) is None
        assert "not asked for" in rc.diff_hmmpost(case, got + (False,), exp)


def hmmpost_against_scipy(case, exp, most=8, longest=600):
    """(largest |loglik difference| in ulp of the scipy route's, largest |gamma difference|, the same divided by
    max(1, |loglik|) * 2^-52, reads compared): up to `most` possible reads of at most `longest` samples"""
    from test_hmm_post_host import plain_forward_backward
    x, used = rc.hmmpost_rows(case)
    post, goff, gamma, S = exp["post"], exp["goff"], exp["gamma"], case["S"]
    worst_l = worst_g = worst_s = 0.0
    rows = [r for r in range(case["R"]) if post["flags"][r] == 0 and 0 < used[r] <= longest][:most]
    for r in rows:
        with np.errstate(divide="ignore", invalid="ignore"):
            L, g, _ = plain_forward_backward(case["model"], x[r, :used[r]])
        worst_l = max(worst_l, abs(post["loglik"][r] - L) / np.spacing(abs(L)))
        d = float(np.abs(gamma[goff[r]:goff[r + 1], :S] - g).max())
        worst_g = max(worst_g, d)
        worst_s = max(worst_s, d / (max(1.0, abs(L)) * 2.0 ** -52))
    return worst_l, worst_g, worst_s, len(rows)


def test_hmmpost_statement_against_the_scipy_route(cases):
    """The statement is the oracle of the GPU leg: on the real-valued committed cases (up to 8 possible reads of at most 600
    samples each) it is compared with plain_forward_backward of tests/test_hmm_post_host.py, scipy's logsumexp and numpy's
    exp.

    Measured (numpy 2, scipy 1.x, glibc): loglik equals the scipy route's to the last bit on all 106 reads (bound: 4 ulp, as in
    test_statement_against_a_plain_logsumexp_forward_backward), gamma differs by at most 3.64e-12, which is 1.43 in units of
    max(1, |L|) * 2^-52.  Both routes carry |L| * 2^-53 in the argument of the last exp, and the
    drawn reads hold anything an int16 holds, so |L| reaches 1e10 and more where the planted reads of
    test_statement_against_a_plain_logsumexp_forward_backward stay near 1e4: the absolute gamma difference is that rounding
    error, which the scaled figure shows.  The bounds are four times the measured values, for other libm and scipy builds."""
    worst = [0.0, 0.0, 0.0, 0]
    for case, exp in cases["hmmpost"]:
        if case["integer"]:
            continue
        got = hmmpost_against_scipy(case, exp)
        worst = [max(a, b) for a, b in zip(worst[:3], got[:3])] + [worst[3] + got[3]]
    print("loglik %.3g ulp, gamma %.3g absolute, %.3g in units of max(1, |L|) * 2^-52, %d reads" % tuple(worst))
    assert worst[3] >= 40
    assert worst[0] <= 4 and worst[1] <= 4 * 3.64e-12 and worst[2] <= 4 * 1.43


def test_sixth_interleaved_sequence_is_what_it_claims(cases):
    """Posterior cases between hmm, detect, levels, pairs and band cases, never two of a family in a row; two posterior
    cases that come twice; the largest case before the smallest; a case in at least two slices under SK_HMM_SCRATCH_MB=1
    directly after a Viterbi case whose state-path call is sliced under the same budget."""
    seq = rc.INTERLEAVE6
    assert {f for f, _ in seq} == {"hmmpost", "hmm", "detect", "levels", "pairs", "band"}
    assert all(seed in rc.SEEDS[fam] for fam, seed in seq)
    assert all((a == "hmmpost") != (b == "hmmpost") for (a, _), (b, _) in zip(seq, seq[1:]))
    mine = [s for f, s in seq if f == "hmmpost"]
    assert len(mine) - len(set(mine)) >= 2
    by_seed = {case["seed"]: case for case, _ in cases["hmmpost"]}
    used = {case["seed"]: int(exp["post"]["n_used"].sum()) for case, exp in cases["hmmpost"]}      # (samples the call uses)
    assert used[mine[0]] == max(used.values()) > 1000 * used[mine[1]] and used[mine[1]] == min(used.values())
    hmm = {case["seed"]: case for case, _ in cases["hmm"]}
    assert any(fa == "hmm" and "SK_HMM_SCRATCH_MB" in hmm[sa]["env"] and rc.hmm_slices(hmm[sa]) >= 2 and fb == "hmmpost" and
               "SK_HMM_SCRATCH_MB" in by_seed[sb]["env"] and rc.hmmpost_slices(by_seed[sb]) >= 2
               for (fa, sa), (fb, sb) in zip(seq, seq[1:]))
