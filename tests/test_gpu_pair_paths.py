"""GPU: warping paths over a pair list (sk_dtw_pairs_paths, sk_pairpath.hip) against the references of
tests/pair_paths_ref.py, which never are the code under test: the oracle's dtw_subsequence_path for the subsequence mode,
for the global mode the oracle through the sentinel form that tests/test_pair_paths_host.py holds to mlpy's path() over a
plain double-loop matrix.  Spans equal as integers; records the bytes of dtw_pairs."""
import numpy as np
import pytest

import detect_ref
import pair_paths_ref as ppr
import pairs_ref
from test_cli import run_cli

pytestmark = pytest.mark.gpu
MODES = ("subsequence", "global")


def spans_differ(got, want, off):
    """the pairs whose spans differ (first five), for the assertion message"""
    return [(p, got[off[p]:off[p + 1]][:4].tolist(), want[off[p]:off[p + 1]][:4].tolist()) for p in range(len(off) - 1)
            if not np.array_equal(got[off[p]:off[p + 1]], want[off[p]:off[p + 1]])][:5]


# ---- shape grid ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid(ora):
    seqs, pairs = ppr.path_grid()
    return seqs, pairs, {m: ppr.list_spans(ora, seqs, pairs, m) for m in MODES}


@pytest.fixture(scope="module")
def grid_gpu(gpu, grid):
    """the grid through the library as is: {mode: (records, span_off, spans)}, shared and left unchanged"""
    from squigglekit_amd import api
    seqs, pairs, _ = grid
    out = {}
    for m in MODES:
        out[m] = api.dtw_pairs_paths(seqs, pairs, m)
        assert api.last_path_mismatches() == 0, m
    return out


@pytest.mark.parametrize("mode", MODES)
def test_shape_grid_in_one_call(gpu, grid, grid_gpu, mode):
    """every query length around the stripe edges against windows around the word edge, the LDS column and word limits
    and a window wider than 4 096, all in ONE call; the same list shuffled and with duplicates gives the same spans"""
    from squigglekit_amd import api
    seqs, pairs, want = grid
    woff, wspans = want[mode]
    rec, off, spans = grid_gpu[mode]
    assert off.dtype == np.int64 and np.array_equal(off, woff)
    assert spans.dtype == np.int32 and spans.shape == wspans.shape
    assert np.array_equal(spans, wspans), spans_differ(spans, wspans, off)
    assert rec.tobytes() == api.dtw_pairs(seqs, pairs, mode).tobytes()
    for p, (q, t) in enumerate(pairs):
        ppr.check_invariants(spans[off[p]:off[p + 1]], mode, rec["start"][p], rec["end"][p])
    rng = np.random.default_rng(1)
    idx = np.concatenate([rng.permutation(len(pairs)), rng.integers(0, len(pairs), size=40)])
    rec2, off2, spans2 = api.dtw_pairs_paths(seqs, [pairs[i] for i in idx], mode)
    assert api.last_path_mismatches() == 0
    assert rec2.tobytes() == rec[idx].tobytes()
    assert np.array_equal(np.diff(off2), np.diff(off)[idx])
    for k, i in enumerate(idx):
        assert np.array_equal(spans2[off2[k]:off2[k + 1]], wspans[off[i]:off[i + 1]]), (mode, k, i)


# ---- tiers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_every_tier_gives_the_same_bytes(gpu, grid, grid_gpu, monkeypatch, mode):
    """as is; every pair in the scratch tier; ... and one wavefront with one slab working through all of them"""
    from squigglekit_amd import api
    seqs, pairs, _ = grid
    rec, off, spans = grid_gpu[mode]
    monkeypatch.setenv("SK_PATH_LDS_BYTES", "0")
    rec1, _, spans1 = api.dtw_pairs_paths(seqs, pairs, mode)
    assert api.last_path_mismatches() == 0
    listed, slab, waves = api.last_pair_paths_tiers()
    assert listed == len(pairs) and slab > 0 and 1 <= waves <= listed
    monkeypatch.setenv("SK_PATH_SCRATCH_BYTES", "1000")
    rec2, _, spans2 = api.dtw_pairs_paths(seqs, pairs, mode)
    assert api.last_path_mismatches() == 0
    assert api.last_pair_paths_tiers() == (listed, slab, 1)
    assert spans1.tobytes() == spans.tobytes() and spans2.tobytes() == spans.tobytes()
    assert rec1.tobytes() == rec.tobytes() and rec2.tobytes() == rec.tobytes()


def test_the_slab_is_sized_from_the_listed_windows(gpu, ora):
    """short queries in a long target: the scratch slab holds the widest listed window, not the target"""
    from squigglekit_amd import api
    rng = np.random.default_rng(9)
    ref = rng.normal(size=20000)
    qs = [ref[a:a + 400] + rng.normal(scale=0.05, size=400) for a in (100, 7000, 19000)]
    seqs, pairs = qs + [ref], [(0, 3), (1, 3), (2, 3)]
    rec, off, spans = api.dtw_pairs_paths(seqs, pairs)
    listed, slab, waves = api.last_pair_paths_tiers()
    width = int((rec["end"] - rec["start"] + 1).max())
    assert listed == 3 and waves == 3                               # 400 x 25 words: above the LDS tier's 6 400
    assert width < 1000 and slab <= 8 * width + 4 * 400 * ((width + 15) // 16) + 8
    assert api.last_path_mismatches() == 0
    assert np.array_equal(spans, ppr.list_spans(ora, seqs, pairs, "subsequence")[1])


# ---- supplied records ------------------------------------------------------------------------------------------------
def test_tiled_mapping_traced_against_the_whole_targets(gpu, ora):
    """merged records of a tiled search, in whole-target coordinates, traced against the whole targets: the oracle's path
    of the query in the winning piece, shifted by the piece's origin"""
    from squigglekit_amd import api
    queries, targets = pairs_ref.mapping_case()
    pieces, tiling = api.tile_targets(targets, 1024, 512)
    rec, _ = api.map_queries(queries, pieces)
    merged = api.merge_tiles(rec, tiling)
    span_off, spans = api.map_paths(queries, targets, merged)
    assert api.last_path_mismatches() == 0
    best = api.best_targets(merged)
    assert np.array_equal(np.diff(span_off), [len(q) for q in queries])
    for q, x in enumerate(queries):
        mine = [p for p in range(len(pieces)) if tiling["target"][p] == best[q]]
        win = min(mine, key=lambda p: (rec["dist"][p, q], rec["end"][p, q] + tiling["origin"][p], p))
        want = ppr.spans(ora, x, pieces[win], "subsequence") + int(tiling["origin"][win])
        got = spans[span_off[q]:span_off[q + 1]]
        assert np.array_equal(got, want), (q, win)
        assert got[0, 0] == merged["start"][best[q], q] and got[-1, 1] == merged["end"][best[q], q]
    # a query without a target has a zero-length entry
    which = best.copy()
    which[[0, 5]] = -1
    so2, sp2 = api.map_paths(queries, targets, merged, which)
    assert so2[1] == 0 and so2[6] == so2[5] and len(sp2) == len(spans) - len(queries[0]) - len(queries[5])
    assert np.array_equal(sp2[so2[1]:so2[2]], spans[span_off[1]:span_off[2]])


@pytest.mark.parametrize("mode", MODES)
def test_the_calls_own_records_supplied_give_the_same_bytes(gpu, grid, grid_gpu, mode):
    from squigglekit_amd import api
    seqs, pairs, _ = grid
    rec, off, spans = grid_gpu[mode]
    rec2, off2, spans2 = api.dtw_pairs_paths(seqs, pairs, mode, records=rec)
    assert api.last_path_mismatches() == 0
    assert rec2.tobytes() == rec.tobytes() and off2.tobytes() == off.tobytes() and spans2.tobytes() == spans.tobytes()


# ---- mismatches ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_mismatches_are_counted_not_faults(gpu, mode):
    """three corrupted records (dist moved by one ulp; start + 1; in global mode end - 1, in subsequence mode a second
    dist) get spans -1 and are counted; a NaN record gets -1 and is not; every other pair keeps its spans"""
    from squigglekit_amd import api
    rng = np.random.default_rng(21)
    seqs, pairs = [], []
    for N, M in ((40, 300), (70, 90), (25, 500), (130, 140), (64, 64), (30, 31), (90, 700), (10, 45)):
        pairs.append((len(seqs), len(seqs) + 1))
        seqs += [rng.normal(size=N), rng.normal(size=M)]
    rec, off, spans = api.dtw_pairs_paths(seqs, pairs, mode)
    assert api.last_path_mismatches() == 0 and np.all(spans >= 0)
    assert rec["end"][3] > rec["start"][3]
    bad = rec.copy()
    bad["dist"][1] = np.nextafter(bad["dist"][1], np.inf)
    bad["start"][3] += 1
    if mode == "global":
        bad["end"][4] -= 1
    else:
        bad["dist"][4] = np.nextafter(bad["dist"][4], -np.inf)
    bad["dist"][6] = np.nan
    rec2, off2, spans2 = api.dtw_pairs_paths(seqs, pairs, mode, records=bad)
    assert api.last_path_mismatches() == 3
    assert rec2.tobytes() == bad.tobytes()                          # supplied records are input only
    for p in range(len(pairs)):
        part = spans2[off[p]:off[p + 1]]
        if p in (1, 3, 4, 6):
            assert np.all(part == -1), p
        else:
            assert np.array_equal(part, spans[off[p]:off[p + 1]]), p


@pytest.mark.parametrize("mode", MODES)
def test_records_outside_the_target_are_mismatches(gpu, mode):
    """start / end outside [0, M), end < start: checked before any load, spans -1, counted; SK_FLAG_EMPTY: not counted"""
    from squigglekit_amd import api
    rng = np.random.default_rng(22)
    seqs = [rng.normal(size=20), rng.normal(size=50)]
    pairs = [(0, 1)] * 8
    rec, off, spans = api.dtw_pairs_paths(seqs, pairs, mode)
    bad = rec.copy()
    bad["end"][0] = 50
    bad["start"][1] = -1
    bad["start"][2], bad["end"][2] = 30, 29
    bad["end"][3] = 2 ** 31 - 1
    bad["start"][4], bad["end"][4] = -2 ** 31, 2 ** 31 - 1
    bad["start"][5], bad["end"][5] = 2 ** 31 - 1, 2 ** 31 - 1
    bad["flags"][6] = gpu.SK_FLAG_EMPTY
    _, _, spans2 = api.dtw_pairs_paths(seqs, pairs, mode, records=bad)
    assert api.last_path_mismatches() == 6
    assert np.all(spans2[:off[7]] == -1)
    assert np.array_equal(spans2[off[7]:], spans[off[7]:])


# ---- refusals --------------------------------------------------------------------------------------------------------
def raw_call(gpu, values, off, pairs, mode, rec, have, spans):
    L = gpu.load()
    pr = np.zeros(len(pairs), dtype=[("query", "<i4"), ("target", "<i4")])
    if len(pairs):
        pr["query"], pr["target"] = zip(*pairs)
    rc = L.sk_dtw_pairs_paths(gpu.ptr(values), gpu.ptr(off), off.size - 1, gpu.ptr(pr), len(pr), mode,
                              gpu.ptr(rec), have, None if spans is None else gpu.ptr(spans))
    return rc, L.sk_last_error().decode()


@pytest.mark.parametrize("mode", (0, 1))
def test_edge_cases_refuse_with_code_and_message_and_write_nothing(gpu, ora, mode):
    rng = np.random.default_rng(3)
    seqs = [rng.normal(size=30), np.zeros(0), rng.normal(size=1025), rng.normal(size=50)]
    values = np.ascontiguousarray(np.concatenate(seqs))
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    name = MODES[mode]
    good = [(0, 3), (3, 0), (0, 2)]
    want = pairs_ref.records(ora, seqs, good, name)
    woff, wspans = ppr.list_spans(ora, seqs, good, name)

    def valid_call():
        rec = np.zeros(len(good), dtype=gpu.HIT_DTYPE)
        sp = np.zeros((int(woff[-1]), 2), dtype=np.int32)
        rc, msg = raw_call(gpu, values, off, good, mode, rec, 0, sp)
        assert rc == 0, msg
        assert pairs_ref.same_records(rec, want.astype(rec.dtype)) and np.array_equal(sp, wspans)

    for have in (0, 1):
        for pairs, code, words in (([(0, 3), (1, 3)], gpu.SK_ERR_INVALID, ("pair 1", "empty query")),
                                   ([(0, 4)], gpu.SK_ERR_INVALID, ("pair 0", "target index 4")),
                                   ([(0, 3), (0, 3), (-1, 0)], gpu.SK_ERR_INVALID, ("pair 2", "query index -1")),
                                   ([(3, 0), (2, 3)], gpu.SK_ERR_UNSUPPORTED, ("pair 1", "1025 points"))):
            rec = np.full(len(pairs) * 24, 0xAB, dtype=np.uint8)
            sp = np.full(4096 * 8, 0xAB, dtype=np.uint8)
            rc, msg = raw_call(gpu, values, off, pairs, mode, rec, have, sp)
            assert rc == code and all(w in msg for w in words), (pairs, rc, msg)
            assert np.all(rec == 0xAB) and np.all(sp == 0xAB), pairs    # no record, no span was written
            valid_call()                                                # a valid call after a refused one
    rec = np.full(24, 0xAB, dtype=np.uint8)
    sp = np.full(4096 * 8, 0xAB, dtype=np.uint8)
    rc, msg = raw_call(gpu, values, off, [], mode, rec, 0, sp)          # npairs == 0
    assert rc == 0 and np.all(rec == 0xAB) and np.all(sp == 0xAB)
    rc, msg = raw_call(gpu, values, off, [(0, 3)], 2, rec, 0, sp)
    assert rc == gpu.SK_ERR_INVALID and "mode" in msg and np.all(rec == 0xAB) and np.all(sp == 0xAB)
    rc, msg = raw_call(gpu, values, off, [(0, 3)], mode, rec, 0, None)  # NULL spans
    assert rc == gpu.SK_ERR_INVALID and "spans" in msg and np.all(rec == 0xAB)
    # an empty target is a record, not an error: flagged, spans -1, not counted
    rec = np.zeros(2, dtype=gpu.HIT_DTYPE)
    sp = np.zeros((60, 2), dtype=np.int32)
    rc, msg = raw_call(gpu, values, off, [(0, 1), (0, 3)], mode, rec, 0, sp)
    assert rc == 0, msg
    assert pairs_ref.same_records(rec, pairs_ref.records(ora, seqs, [(0, 1), (0, 3)], name).astype(rec.dtype))
    assert np.isnan(rec["dist"][0]) and rec[0].tolist()[1:] == (-1, -1, 0, 1)
    assert np.all(sp[:30] == -1) and np.array_equal(sp[30:], wspans[:30])
    assert gpu.load().sk_last_path_mismatches() == 0


# ---- device-resident form --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_device_resident_form_equals_the_host_form(gpu, grid, grid_gpu, mode):
    from squigglekit_amd import api
    L = gpu.load()
    seqs, pairs, _ = grid
    values, off = api._as_pool(seqs)
    pad = np.concatenate([np.full(7, np.nan), values])                # the pool need not start at off = 0
    off7 = off + 7
    pr = api._as_pairs(pairs)
    rec, span_off, spans = api.dtw_pairs_paths((pad, off7), pr, mode)
    assert rec.tobytes() == grid_gpu[mode][0].tobytes() and spans.tobytes() == grid_gpu[mode][2].tobytes()
    d_val, d_rec, d_sp = L.sk_dev_alloc(pad.nbytes), L.sk_dev_alloc(len(pr) * 24), L.sk_dev_alloc(spans.nbytes)
    try:
        gpu.check(L.sk_dev_upload(d_val, gpu.ptr(pad), pad.nbytes))
        for have in (0, 1):                                           # computed, then the same records supplied
            gpu.check(L.sk_dtw_pairs_paths_dev(d_val, gpu.ptr(off7), off7.size - 1, gpu.ptr(pr), len(pr),
                                               api.PAIRS_MODES[mode], d_rec, have, d_sp))
            gpu.check(L.sk_sync())
            assert L.sk_last_path_mismatches() == 0
            dev_rec = np.zeros(len(pr), dtype=gpu.HIT_DTYPE)
            dev_sp = np.zeros_like(spans)
            gpu.check(L.sk_dev_download(gpu.ptr(dev_rec), d_rec, dev_rec.nbytes))
            gpu.check(L.sk_dev_download(gpu.ptr(dev_sp), d_sp, dev_sp.nbytes))
            assert dev_rec.tobytes() == rec.tobytes() and dev_sp.tobytes() == spans.tobytes(), have
    finally:
        L.sk_dev_free(d_val)
        L.sk_dev_free(d_rec)
        L.sk_dev_free(d_sp)


# ---- mlpy's boundary -------------------------------------------------------------------------------------------------
def test_dtw_std_returns_mlpys_path(gpu):
    from squigglekit_amd import api
    rng = np.random.default_rng(4)
    for x, y in ((rng.normal(size=163), rng.normal(size=900)),
                 (pairs_ref.draw(rng, 17, True), pairs_ref.draw(rng, 17, True))):
        want_dist, wx, wy = ppr.global_path_plain(x, y)
        dist, cost, (px, py) = api.dtw_std(x, y, dist_only=False)
        assert api.last_path_mismatches() == 0
        assert cost is None
        assert np.array_equal(px, wx) and np.array_equal(py, wy)
        rec = api.dtw_pairs([x, y], [(0, 1)], "global")
        assert pairs_ref.bits(dist) == pairs_ref.bits(rec["dist"][0]) == pairs_ref.bits(want_dist)
        only = api.dtw_std(x, y)
        assert isinstance(only, float) and pairs_ref.bits(only) == pairs_ref.bits(dist)


# ---- command line ----------------------------------------------------------------------------------------------------
def test_cli_align_table_on_synthetic_reads(gpu, ora, tmp_path):
    """squiggle_map --align on 24 synthetic reads (the reads of test_gpu_pairs.test_cli_on_synthetic_reads): the table
    equals the composition of tests/detect_ref.py, numpy, the oracle's path and the same formatting; whole targets, then
    tiled (the merged record traced against the whole target); stdout is what the run without --align prints"""
    from squigglekit_amd import api
    from squigglekit_amd.map_cli import main
    rng = np.random.default_rng(77)
    model = tmp_path / "ref.model"
    levels = {}
    with open(model, "w") as fh:
        for name, n in (("recA", 150), ("recB", 90)):
            levels[name] = np.array([float("%.3f" % v) for v in rng.uniform(60, 130, size=n)])   # (as the text reads back)
            fh.write("#%s\npos\tbase\tcurrent\tsd\tdwell\n" % name)
            for i, v in enumerate(levels[name]):
                fh.write("%d\tA\t%.3f\t1.5\t8.0\n" % (i, v))
    reads = np.zeros((24, 1500), dtype=np.int16)
    for r in range(22):
        src = levels[("recA", "recB")[r % 2]]
        src = src[::-1] if r % 3 == 0 else src
        a = int(rng.integers(0, len(src) - 60))
        lev = np.repeat(src[a:a + 60] * 5.0, rng.integers(18, 32, size=60))[:1500]
        reads[r, :len(lev)] = np.round(lev + rng.normal(scale=2.0, size=len(lev)))
        reads[r, len(lev):] = reads[r, len(lev) - 1]
    reads[22] = 7                                                   # one event: no match, no table lines
    reads[23, :] = np.repeat([300, 500], 750)                       # cut by the prefix to its first level: the same
    path = tmp_path / "reads.npy"
    np.save(path, reads)

    targets = []
    for name in ("recA", "recB"):
        z = pairs_ref.zscore(levels[name])
        targets += [(name, "+", z), (name, "-", z[::-1].copy())]
    ys = [t[2] for t in targets]

    def expected(pieces=None):
        lines = ["readID\ttarget\tstrand\tevent\tsample_start\tsample_length\tlevel\tz\tref_first\tref_last\n"]
        for r in range(24):
            rec = detect_ref.events(reads[r, :700])
            lev = rec["sum"].astype(np.float64) / rec["length"].astype(np.float64)
            if len(lev) < 2 or not lev.std() > 0:
                continue
            q = (lev - lev.mean()) / lev.std()
            if pieces:
                cut, tiling = api.tile_targets(ys, *pieces)
                per = pairs_ref.oracle_map(ora, [q], cut)[:, 0]
                hits = api.merge_tiles(per.astype(api.HIT_DTYPE).reshape(-1, 1), tiling)[:, 0]
            else:
                hits = pairs_ref.oracle_map(ora, [q], ys)[:, 0]
            b = sorted(range(4), key=lambda t: (hits["dist"][t], t))[0]
            if pieces:
                mine = [p for p in range(len(cut)) if tiling["target"][p] == b]
                win = min(mine, key=lambda p: (per["dist"][p], per["end"][p] + tiling["origin"][p], p))
                sp = ppr.spans(ora, q, cut[win], "subsequence") + int(tiling["origin"][win])
            else:
                sp = ppr.spans(ora, q, ys[b], "subsequence")
            assert sp[0, 0] == hits["start"][b] and sp[-1, 1] == hits["end"][b]
            for e in range(len(q)):
                lines.append("{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\n".format(
                    r, targets[b][0], targets[b][1], e, int(rec["start"][e]), int(rec["length"][e]), float(lev[e]),
                    float(q[e]), int(sp[e, 0]), int(sp[e, 1])))
        return "".join(lines)

    argv = ["--i16", str(path), "-m", str(model), "--both", "--prefix", "700", "--batch", "10"]
    for extra, pieces in (([], None), (["--piece", "64", "--overlap", "40"], (64, 40))):
        plain, se, code = run_cli(main, argv + extra)
        assert code == 0, se
        table = tmp_path / ("align%d.tsv" % len(extra))
        so, se, code = run_cli(main, argv + extra + ["--align", str(table)])
        assert code == 0, se
        assert so == plain                                          # stdout does not change
        got = open(table).read()
        assert got == expected(pieces)
        assert len({ln.split("\t")[0] for ln in got.split("\n")[1:-1]}) == 22
