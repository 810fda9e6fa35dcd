"""GPU: adaptive-band DTW over a pair list (sk_dtw_band, sk_band.hip) against the statement in tests/band_ref.py, which
never is the code under test.  Every comparison: the records bit for bit, the spans equal as integers, the mismatches
counted those of the statement -- none for finite inputs, the pairs without a path where an inf or a NaN makes some.
Equality with the full matrix is asserted only where every cell lies in its band (N, M <= W / 2)."""
import functools

import numpy as np
import pytest

import band_ref as br
import pairs_ref

pytestmark = pytest.mark.gpu
WIDTHS = br.WIDTHS
ENDS = br.ENDS


def check(got, want, what=""):
    """(records, span_off, spans) of the library against those of band_ref.records"""
    rec, off, spans = got
    wrec, woff, wspans, _ = want
    bad = [p for p in range(len(wrec)) if not pairs_ref.same_records(rec[p:p + 1], wrec[p:p + 1].astype(rec.dtype))]
    assert not bad, (what, bad[:5], rec[bad[:3]], wrec[bad[:3]])
    assert off.dtype == np.int64 and np.array_equal(off, woff), what
    assert spans.dtype == np.int32 and spans.shape == wspans.shape, what
    diff = [p for p in range(len(wrec)) if not np.array_equal(spans[off[p]:off[p + 1]], wspans[off[p]:off[p + 1]])]
    assert not diff, (what, diff[:5], spans[off[diff[0]]:off[diff[0] + 1]][:6].tolist(),
                      wspans[off[diff[0]]:off[diff[0] + 1]][:6].tolist())


def run(seqs, pairs, W, end):
    from squigglekit_amd import api
    got = api.dtw_band(seqs, pairs, W, end)
    return got, api.last_path_mismatches()


# ---- the whole matrix in the band ------------------------------------------------------------------------------------
def small_list(W, seed=11):
    rng = np.random.default_rng(seed + W)
    sizes = (1, 2, 3, 31, 32) + ((33,) if W >= 128 else ())
    seqs, pairs = [], []
    for k, N in enumerate(sizes):
        for M in sizes:
            pairs.append((len(seqs), len(seqs) + 1))
            seqs += [pairs_ref.draw(rng, N, (k + M) % 2 == 0), pairs_ref.draw(rng, M, (k + M) % 2 == 0)]
    return seqs, pairs


@pytest.mark.parametrize("W", WIDTHS)
def test_whole_matrix_in_band_equals_the_statement_and_the_global_mode(gpu, W):
    from squigglekit_amd import api
    seqs, pairs = small_list(W)
    for end in ENDS:
        got, mism = run(seqs, pairs, W, end)
        assert mism == 0
        check(got, br.records(seqs, pairs, W, end), (W, end))
        for p in range(len(pairs)):
            br.check_invariants(got[2][got[1][p]:got[1][p + 1]], got[0]["end"][p])
    got, _ = run(seqs, pairs, W, "pinned")
    assert got[0].tobytes() == api.dtw_pairs(seqs, pairs, "global").tobytes()
    grec, goff, gspans = api.dtw_pairs_paths(seqs, pairs, "global")
    assert np.array_equal(goff, got[1]) and np.array_equal(gspans, got[2])


# ---- edges of the machinery ------------------------------------------------------------------------------------------
def edge_list(seed=12):
    """stream refills (63 .. 129 points), word flushes (N + M - 1 = 15 .. 65), shapes that hug an edge; every other pair
    tie-heavy integers"""
    rng = np.random.default_rng(seed)
    shapes = [(N, M) for N in (63, 64, 65, 127, 128, 129) for M in (63, 64, 65, 127, 128, 129)]
    for s in (15, 16, 17, 31, 32, 33, 63, 64, 65):
        shapes += [((s + 1) // 2, s + 1 - (s + 1) // 2), (1, s), (s, 1)]
    shapes += [(1, 500), (500, 1), (2, 300), (300, 2), (700, 90), (90, 700)]
    seqs, pairs = [], []
    for k, (N, M) in enumerate(shapes):
        pairs.append((len(seqs), len(seqs) + 1))
        seqs += [pairs_ref.draw(rng, N, k % 2 == 0), pairs_ref.draw(rng, M, k % 2 == 0)]
    return seqs, pairs


@pytest.fixture(scope="module")
def edges():
    seqs, pairs = edge_list()
    return seqs, pairs, {(W, end): br.records(seqs, pairs, W, end) for W in WIDTHS for end in ENDS}


@pytest.mark.parametrize("W", WIDTHS)
def test_edges_of_the_machinery_in_one_call(gpu, edges, W):
    seqs, pairs, want = edges
    for end in ENDS:
        got, mism = run(seqs, pairs, W, end)
        assert mism == want[(W, end)][3] == 0
        check(got, want[(W, end)], (W, end))


# ---- drift -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drift():
    rng = np.random.default_rng(13)
    cases = [br.drift_pair(rng, 400, 0.55, 0.3, 120) for _ in range(8)] + \
            [br.drift_pair(rng, 400, 0.3, 0.5, 0) for _ in range(8)]
    return cases


def test_drifting_paths_equal_the_statement_and_bound_the_global_distance(gpu, ora, drift):
    seqs = [s for xy in drift for s in xy]
    pairs = [(2 * k, 2 * k + 1) for k in range(len(drift))]
    full = np.array([pairs_ref.dtw_global_sentinel(ora, x, y)[0] for x, y in drift])
    for W in WIDTHS:
        got, mism = run(seqs, pairs, W, "pinned")
        assert mism == 0
        check(got, br.records(seqs, pairs, W, "pinned"), W)
        assert np.all(got[0]["dist"] >= full), (W, got[0]["dist"], full)


def test_free_end_against_longer_targets(gpu, drift):
    rng = np.random.default_rng(14)
    seqs, pairs = [], []
    for x, y in drift:
        pairs.append((len(seqs), len(seqs) + 1))
        seqs += [x, np.concatenate([y, rng.normal(size=150)])]
    for W in WIDTHS:
        want = br.records(seqs, pairs, W, "free")
        got, mism = run(seqs, pairs, W, "free")
        assert mism == want[3]
        check(got, want, W)
        assert np.array_equal(got[0]["end"], want[0]["end"])
        assert np.all(got[0]["end"] < np.array([len(seqs[t]) for _, t in pairs]))


# ---- scheduling ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(15)
    lens = [1, 2, 3, 40, 64, 65, 200, 333, 700, 1024, 1500, 3000]
    seqs = [pairs_ref.draw(rng, n, k % 3 == 0) for k, n in enumerate(lens)] + [np.zeros(0)]
    pairs = [(int(q), int(t)) for q, t in zip(rng.integers(0, len(lens), size=40), rng.integers(0, len(lens), size=40))]
    pairs += [(11, 11), (0, 11), (11, 0), (3, 12)]
    return seqs, pairs, br.records(seqs, pairs, 128, "pinned")


def test_scheduling_does_not_change_a_byte(gpu, mixed, monkeypatch):
    from squigglekit_amd import api
    seqs, pairs, want = mixed
    got, mism = run(seqs, pairs, 128, "pinned")
    assert mism == want[3] == 0
    check(got, want)
    rec, off, spans = got
    slab, waves, steps = api.last_band_plan()
    assert steps == 5999 and waves == len(pairs) == 44 and slab == ((steps * 2 + 15) // 16) * 256 + ((steps + 63) // 64) * 8 + 8
    # shuffled and with duplicates
    rng = np.random.default_rng(1)
    idx = np.concatenate([rng.permutation(len(pairs)), rng.integers(0, len(pairs), size=20)])
    (rec2, off2, spans2), mism = run(seqs, [pairs[i] for i in idx], 128, "pinned")
    assert mism == 0 and rec2.tobytes() == rec[idx].tobytes()
    for k, i in enumerate(idx):
        assert np.array_equal(spans2[off2[k]:off2[k + 1]], spans[off[i]:off[i + 1]]), (k, i)
    # records only
    assert api.dtw_band(seqs, pairs, 128, "pinned", paths=False).tobytes() == rec.tobytes()
    assert api.last_band_plan() == (0, len(pairs), steps)
    # one wavefront with one slab through the whole list
    monkeypatch.setenv("SK_BAND_WAVES", "1")
    (rec3, off3, spans3), mism = run(seqs, pairs, 128, "pinned")
    assert api.last_band_plan() == (slab, 1, steps)
    assert mism == 0 and rec3.tobytes() == rec.tobytes() and spans3.tobytes() == spans.tobytes()
    assert api.dtw_band(seqs, pairs, 128, "pinned", paths=False).tobytes() == rec.tobytes()


def test_device_resident_form_equals_the_host_form(gpu, mixed):
    from squigglekit_amd import api
    L = gpu.load()
    seqs, pairs, _ = mixed
    values, off = api._as_pool(seqs)
    pad = np.concatenate([np.full(7, np.nan), values])                # the pool need not start at off = 0
    off7 = off + 7
    pr = api._as_pairs(pairs)
    for W, end in [(W, end) for W in WIDTHS for end in ENDS]:
        rec, span_off, spans = api.dtw_band(seqs, pairs, W, end)
        rec7, _, spans7 = api.dtw_band((pad, off7), pr, W, end)
        assert rec7.tobytes() == rec.tobytes() and spans7.tobytes() == spans.tobytes()
        d_val, d_rec, d_sp = L.sk_dev_alloc(pad.nbytes), L.sk_dev_alloc(len(pr) * 24), L.sk_dev_alloc(spans.nbytes)
        try:
            gpu.check(L.sk_dev_upload(d_val, gpu.ptr(pad), pad.nbytes))
            for with_spans in (True, False):
                gpu.check(L.sk_dtw_band_dev(d_val, gpu.ptr(off7), off7.size - 1, gpu.ptr(pr), len(pr), W,
                                            api.BAND_ENDS[end], d_rec, d_sp if with_spans else None))
                gpu.check(L.sk_sync())
                dev_rec = np.zeros(len(pr), dtype=gpu.HIT_DTYPE)
                dev_sp = np.zeros_like(spans)
                gpu.check(L.sk_dev_download(gpu.ptr(dev_rec), d_rec, dev_rec.nbytes))
                gpu.check(L.sk_dev_download(gpu.ptr(dev_sp), d_sp, dev_sp.nbytes))
                assert dev_rec.tobytes() == rec.tobytes() and dev_sp.tobytes() == spans.tobytes(), (W, end, with_spans)
            assert L.sk_last_path_mismatches() == 0
        finally:
            L.sk_dev_free(d_val)
            L.sk_dev_free(d_rec)
            L.sk_dev_free(d_sp)


def test_empty_target_is_a_record_not_an_error(gpu):
    from squigglekit_amd import api
    rng = np.random.default_rng(16)
    seqs = [rng.normal(size=30), np.zeros(0), rng.normal(size=50)]
    pairs = [(0, 1), (0, 2), (2, 1)]
    for end in ENDS:
        rec, off, spans = api.dtw_band(seqs, pairs, 64, end)
        assert api.last_path_mismatches() == 0
        check((rec, off, spans), br.records(seqs, pairs, 64, end))
        assert np.isnan(rec["dist"][0]) and rec[0].tolist()[1:] == (-1, -1, 0, gpu.SK_FLAG_EMPTY)
        assert np.all(spans[:30] == -1) and np.all(spans[30:60] >= 0) and np.all(spans[60:] == -1)


# ---- seeded random ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("end", ENDS)
def test_seeded_random_pairs(gpu, end):
    """200 pairs, N and M in [1, 1 500], W drawn per call: four calls of 50 pairs"""
    rng = np.random.default_rng(17 + ENDS.index(end))
    for call in range(4):
        W = int(rng.choice(WIDTHS))
        seqs, pairs = [], []
        for k in range(50):
            N, M = (int(v) for v in rng.integers(1, 1501, size=2))
            pairs.append((len(seqs), len(seqs) + 1))
            if k % 5 == 0:
                seqs += [pairs_ref.draw(rng, N, True), pairs_ref.draw(rng, M, True)]
            elif k % 5 == 1:
                seqs += list(br.drift_pair(rng, max(M // 3, 1), 0.45, 0.35, 0))
            else:
                seqs += [rng.normal(size=N), rng.normal(size=M)]
        want = br.records(seqs, pairs, W, end)
        got, mism = run(seqs, pairs, W, end)
        assert mism == want[3]
        check(got, want, (call, W, end))


# ---- lists longer than the launch ------------------------------------------------------------------------------------
LAUNCH_PAIRS, LAUNCH_ENTRIES = 240, 20000


@functools.lru_cache(maxsize=None)
def launch_pairs(W):
    """(seqs, pairs, {end: (records, spans per pair, pairs without a path)}): LAUNCH_PAIRS distinct pairs, N and M in
    [1, 200] with the edge lengths among them, every third pair tie-heavy, every twentieth lost by an inf in its query"""
    rng = np.random.default_rng(18 + W)
    edges = [n for n in (1, 2, 3, W // 2 - 1, W // 2, W // 2 + 1, 63, 64, 65, 127, 128, 129, 199, 200) if n <= 200]
    seqs, pairs = [], []
    for k in range(LAUNCH_PAIRS):
        N, M = (int(rng.choice(edges)) if rng.random() < 0.3 else int(rng.integers(1, 201)) for _ in range(2))
        x, y = pairs_ref.draw(rng, N, k % 3 == 0), pairs_ref.draw(rng, M, k % 3 == 0)
        if k % 20 == 7:
            x, y = br.lay_non_finite(rng, x, y, "+inf in a query")
        pairs.append((len(seqs), len(seqs) + 1))
        seqs += [x, y]
    want = {}
    for end in ENDS:
        rec, off, spans, lost = br.records(seqs, pairs, W, end)
        parts = [spans[off[p]:off[p + 1]] for p in range(LAUNCH_PAIRS)]
        nopath = np.array([sp[0, 0] == -1 for sp in parts])
        assert lost == LAUNCH_PAIRS // 20 <= br.mismatches(seqs, pairs, off, spans) == nopath.sum()
        want[end] = (rec, parts, nopath)
    return seqs, pairs, want


def launch_index(W, n):
    """n list entries over the distinct pairs, every pair at least once"""
    rng = np.random.default_rng(180 + W)
    return rng.permutation(np.concatenate([np.arange(LAUNCH_PAIRS), rng.integers(0, LAUNCH_PAIRS, size=n - LAUNCH_PAIRS)]))


@pytest.mark.parametrize("W", WIDTHS)
def test_lists_longer_than_the_launch(gpu, W):
    """20 000 entries under the launch the library chooses (at most 32 wavefronts per CU: 8 192 on 256 CUs): every
    wavefront strides to a second pair and further, takes its slab from a longer pair to a shorter one, and adds to the
    one mismatch counter.  The expectations are the 240 distinct pairs' by index."""
    from squigglekit_amd import api
    seqs, pairs, want = launch_pairs(W)
    n = LAUNCH_ENTRIES
    for end in ENDS + ("records only",):
        while True:
            idx = launch_index(W, n)
            listed = [pairs[i] for i in idx]
            got = api.dtw_band(seqs, listed, W, "pinned" if end == "records only" else end, paths=end != "records only")
            waves = api.last_band_plan()[1]
            if 2 * waves < n or n > LAUNCH_ENTRIES:
                break
            n = 2 * waves + LAUNCH_ENTRIES                            # a device that holds more: a list longer than that
        assert 2 * waves < len(idx), (waves, len(idx))                # nothing forced: every wavefront takes pairs in turn
        wrec, parts, nopath = want["pinned" if end == "records only" else end]
        rec = got if end == "records only" else got[0]
        assert pairs_ref.same_records(rec, wrec[idx].astype(rec.dtype)), (W, end)
        if end == "records only":
            continue
        assert np.array_equal(got[1], np.concatenate([[0], np.cumsum([len(parts[i]) for i in idx])])), (W, end)
        assert got[2].dtype == np.int32 and np.array_equal(got[2], np.concatenate([parts[i] for i in idx])), (W, end)
        assert api.last_path_mismatches() == nopath[idx].sum() > 0, (W, end)


# ---- long reads ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_reads():
    """a drifting pair of an 18 000-level target (a stall of 500, 2 000 more target points) and a tie-heavy pair of
    20 000 x 20 000"""
    rng = np.random.default_rng(19)
    x, y = br.drift_pair(rng, 18000, 0.6, 0.3, 500, 2000)
    return [x, y, br.ties(rng, 20000), br.ties(rng, 20000)]


@pytest.mark.parametrize("W", WIDTHS)
def test_long_reads(gpu, W):
    """50 000 and 40 000 anti-diagonals in a pair: 8 times the longest pair of the tests above"""
    from squigglekit_amd import api
    seqs = long_reads()
    for end, pairs in (("pinned", [(2, 3), (0, 1)]), ("free", [(0, 1)])):
        want = br.records(seqs, pairs, W, end)
        assert want[3] == 0 and br.mismatches(seqs, pairs, want[1], want[2]) == 0     # a condition on the input
        got, mism = run(seqs, pairs, W, end)
        assert mism == 0
        check(got, want, (W, end))
        steps = max(len(seqs[q]) + len(seqs[t]) - 1 for q, t in pairs)
        slab = -(-steps * W // 1024) * 256 + -(-steps // 64) * 8 + 8          # the header's formula for one wavefront's slab
        assert steps > 39000 and api.last_band_plan() == (slab, len(pairs), steps)
        for p in range(len(pairs)):
            br.check_invariants(got[2][got[1][p]:got[1][p + 1]], got[0]["end"][p])
        assert end == "pinned" or got[0]["end"][0] < len(seqs[1]) - 1000             # the free end is not the pinned one


# ---- non-finite values -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def non_finite_list():
    """(seqs, pairs, kinds): 48 pairs, drifting (odd k) and tie-heavy (even k) in turn, pair k with kind k % 9 of
    band_ref.NONFINITE -- 2 and 9 are coprime, so every kind meets both sorts of pair"""
    rng = np.random.default_rng(21)
    seqs, pairs, kinds = [], [], []
    for k in range(48):
        if k % 2:
            x, y = br.drift_pair(rng, int(rng.integers(30, 160)), 0.55, 0.3, 40 * (k % 4 == 1), 50 * (k % 8 == 3))
        else:
            x, y = br.ties(rng, int(rng.integers(1, 300))), br.ties(rng, int(rng.integers(1, 300)))
        kinds.append(br.NONFINITE[k % len(br.NONFINITE)])
        x, y = br.lay_non_finite(rng, x, y, kinds[-1])
        pairs.append((len(seqs), len(seqs) + 1))
        seqs += [x, y]
    return seqs, pairs, kinds


@pytest.mark.parametrize("W", WIDTHS)
def test_non_finite_values_follow_the_statement(gpu, W):
    """NaN and inf in the pool: a NaN at a band end moves the band by parity, a NaN never is the free end, an inf costs
    +inf along its row or column.  From the statement alone the list holds pairs with a finite dist and a path, pairs
    with a NaN dist and a path (pinned), pairs with a NaN dist whose walk leaves the band (counted, not lost) and lost
    pairs; the library gives the same records, spans and count."""
    from squigglekit_amd import api
    seqs, pairs, kinds = non_finite_list()
    for drifting in (0, 1):                                          # from the list alone: every kind, on both sorts of pair
        assert {kinds[k] for k in range(drifting, len(pairs), 2)} == set(br.NONFINITE)
    assert all(not (np.isfinite(seqs[q]).all() and np.isfinite(seqs[t]).all()) for q, t in pairs)
    seen = set()
    for end in ENDS:
        want = br.records(seqs, pairs, W, end)
        wrec, woff, wspans, lost = want
        path = np.array([wspans[woff[p], 0] != -1 for p in range(len(pairs))])
        seen |= {"finite with a path"} if (np.isfinite(wrec["dist"]) & path).any() else set()
        seen |= {"NaN with a path"} if (np.isnan(wrec["dist"]) & path).any() else set()
        seen |= {"NaN, the walk fails"} if (np.isnan(wrec["dist"]) & ~path).any() else set()
        seen |= {"lost"} if lost else set()
        assert end == "pinned" or not np.isnan(wrec["dist"]).any()       # a NaN never wins the free end's `<`
        got, mism = run(seqs, pairs, W, end)
        check(got, want, (W, end))
        assert mism == br.mismatches(seqs, pairs, woff, wspans) >= lost > 0, (W, end)
        only = api.dtw_band(seqs, pairs, W, end, paths=False)
        assert pairs_ref.same_records(only, wrec.astype(only.dtype)) and only.tobytes() == got[0].tobytes(), (W, end)
    assert seen == {"finite with a path", "NaN with a path", "NaN, the walk fails", "lost"}
