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


def test_same_seed_same_case():
    for fam in rc.SEEDS:
        seed = rc.SEEDS[fam][0]
        a, b = rc.case_of(fam, seed), rc.case_of(fam, seed)
        assert rc.describe(a) == rc.describe(b)
        for key in ("reads", "rows", "motifs"):
            if key in a:
                assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[key], b[key]))


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
