"""GPU: adaptive-band DTW over a pair list (sk_dtw_band, sk_band.hip) against the statement in tests/band_ref.py, which
never is the code under test.  Every comparison: the records bit for bit, the spans equal as integers, no mismatch
counted.  Equality with the full matrix is asserted only where every cell lies in its band (N, M <= W / 2)."""
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
    for end in ENDS:
        rec, span_off, spans = api.dtw_band(seqs, pairs, 128, end)
        rec7, _, spans7 = api.dtw_band((pad, off7), pr, 128, end)
        assert rec7.tobytes() == rec.tobytes() and spans7.tobytes() == spans.tobytes()
        d_val, d_rec, d_sp = L.sk_dev_alloc(pad.nbytes), L.sk_dev_alloc(len(pr) * 24), L.sk_dev_alloc(spans.nbytes)
        try:
            gpu.check(L.sk_dev_upload(d_val, gpu.ptr(pad), pad.nbytes))
            for with_spans in (True, False):
                gpu.check(L.sk_dtw_band_dev(d_val, gpu.ptr(off7), off7.size - 1, gpu.ptr(pr), len(pr), 128,
                                            api.BAND_ENDS[end], d_rec, d_sp if with_spans else None))
                gpu.check(L.sk_sync())
                dev_rec = np.zeros(len(pr), dtype=gpu.HIT_DTYPE)
                dev_sp = np.zeros_like(spans)
                gpu.check(L.sk_dev_download(gpu.ptr(dev_rec), d_rec, dev_rec.nbytes))
                gpu.check(L.sk_dev_download(gpu.ptr(dev_sp), d_sp, dev_sp.nbytes))
                assert dev_rec.tobytes() == rec.tobytes() and dev_sp.tobytes() == spans.tobytes(), (end, with_spans)
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
