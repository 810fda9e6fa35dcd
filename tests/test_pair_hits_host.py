"""CPU: the statement of the hit lists over a pair list (tests/pair_hits_ref.py) holds its own properties on tie-heavy
integers, and the host helpers of the API -- merge_tile_hits, locus_margin, map_decide_loci -- equal the statement."""
import numpy as np
import pytest

import mapstream_ref
import pair_hits_ref as ref
import pairs_ref


def tie_cases():
    rng = np.random.default_rng(41)
    out = []
    for N, M in ((1, 1), (1, 40), (3, 2), (5, 64), (8, 65), (16, 130), (17, 300), (33, 97)):
        out.append((rng.integers(-3, 4, size=N).astype(np.float64), rng.integers(-3, 4, size=M).astype(np.float64)))
    return out


@pytest.mark.parametrize("case", range(8))
def test_reference_properties_on_tie_heavy_integers(ora, case):
    x, y = tie_cases()[case]
    d, s = ref.last_row(ora, x, y)
    full, _ = ref.greedy(d, s, len(y) + 1)
    # hit 1 is the oracle's record
    dist, start, end = ora.dtw_subsequence(x, y)
    assert full[0] == (dist, start, end)
    for K in (1, 2, 3, 8):
        hits, _ = ref.greedy(d, s, K)
        more, _ = ref.greedy(d, s, K + 1)
        assert more[:len(hits)] == hits and len(hits) == min(K, len(full))        # a prefix of the K + 1 list
        assert all(a[0] <= b[0] for a, b in zip(hits, hits[1:]))                  # dists never decrease
        for i, (_, a0, e0) in enumerate(hits):
            assert 0 <= a0 <= e0 < len(y)
            for _, a1, e1 in hits[i + 1:]:
                assert e1 < a0 or a1 > e0                                          # intervals are disjoint
    cut = sorted(d)[len(d) // 3]
    assert all(h[0] <= cut for h in ref.greedy(d, s, 64, cut)[0])
    assert ref.greedy(d, s, 64, -1.0)[0] == []


@pytest.mark.parametrize("case", range(8))
def test_chained_rows_over_any_cut_equal_the_one_shot_last_row(ora, case):
    x, y = tie_cases()[case]
    d, s = ref.last_row(ora, x, y)
    for name, lens in mapstream_ref.splits_of(len(x)).items():
        if min(lens) < 0 or sum(lens) != len(x):
            continue
        state = None
        for ch in mapstream_ref.cut(x, lens):
            if len(ch):
                state = mapstream_ref.chained_rows(ch, y, state)
        assert state[0] == d and [int(v) for v in state[1]] == [int(v) for v in s], name


def host_lists(ora, queries, targets, K, max_dist=np.inf):
    """[T, Q, K] / [T, Q] by the statement"""
    T, Q = len(targets), len(queries)
    hits = np.zeros((T, Q, K), dtype=ref.HIT)
    count = np.zeros((T, Q), dtype=np.int32)
    for t, y in enumerate(targets):
        h, c, _ = ref.pair_hits(ora, list(queries) + [y], [(q, Q) for q in range(Q)], K, max_dist)
        hits[t], count[t] = h, c
    return hits, count


def test_merge_tile_hits_equals_the_statement_and_hit_1_is_merge_tiles(ora):
    from squigglekit_amd import api
    cases = pairs_ref.planted_cases(count=6, M=600)
    for K in (1, 3):
        for q, y in cases:
            pieces, tiling = api.tile_targets([y, y[::-1].copy()], 250, 120)
            hits, count = host_lists(ora, [q], pieces, K)
            got_h, got_c = api.merge_tile_hits(hits, count, tiling, K)
            want_h, want_c = ref.merge_tile_hits(hits, count, tiling, K)
            assert ref.same(got_h, want_h) is None and np.array_equal(got_c, want_c)
            merged = api.merge_tiles(hits[:, :, 0], tiling)
            assert ref.same(got_h[:, :, 0], merged) is None
            for t in range(2):                                        # disjoint, in whole-target coordinates
                iv = [(int(h["start"]), int(h["end"])) for h in got_h[t, 0, :got_c[t, 0]]]
                assert all(b[1] < a[0] or b[0] > a[1] for i, a in enumerate(iv) for b in iv[i + 1:])
                assert all(0 <= a <= e < 600 for a, e in iv)
    # more room than loci: the count says so, the rest are empty slots
    q, y = cases[0]
    pieces, tiling = api.tile_targets([y], 250, 120)
    hits, count = host_lists(ora, [q], pieces, 2)
    got_h, got_c = api.merge_tile_hits(hits, count, tiling, 64)
    assert got_h.shape == (1, 1, 64) and 1 <= got_c[0, 0] <= 2 * len(pieces)
    assert np.isnan(got_h["dist"][0, 0, got_c[0, 0]:]).all() and (got_h["start"][0, 0, got_c[0, 0]:] == -1).all()


def drawn_lists(seed, T, Q, K):
    """hit lists with ties between targets and inside them, some empty"""
    rng = np.random.default_rng(seed)
    hits = np.zeros((T, Q, K), dtype=ref.HIT)
    hits["dist"], hits["start"], hits["end"] = np.nan, -1, -1
    count = rng.integers(0, K + 1, size=(T, Q)).astype(np.int32)
    for t in range(T):
        for q in range(Q):
            d = np.sort(rng.integers(0, 6, size=count[t, q]).astype(np.float64))
            for k in range(count[t, q]):
                hits[t, q, k] = (d[k], 10 * k, 10 * k + 5 + (k and int(d[k] == d[k - 1])), 100, 0)
    return hits, count


@pytest.mark.parametrize("T,K", [(1, 1), (1, 2), (2, 1), (3, 2), (4, 8)])
def test_locus_margin_equals_the_statement(T, K):
    from squigglekit_amd import api
    hits, count = drawn_lists(100 * T + K, T, 40, K)
    best, rec, second = api.locus_margin(hits, count)
    want = ref.locus_margin(hits, count)
    for q, (t, r, s2) in enumerate(want):
        assert best[q] == t and second[q] == s2, (q, best[q], t, second[q], s2)
        if t < 0:
            assert np.isnan(rec["dist"][q]) and rec["start"][q] == -1 and rec["end"][q] == -1
        else:
            assert (rec["dist"][q], rec["start"][q], rec["end"][q]) == r and rec["n"][q] == 100


@pytest.mark.parametrize("T,K", [(1, 2), (2, 2), (3, 8)])
def test_map_decide_loci_equals_the_statement(T, K):
    from squigglekit_amd import api
    hits, count = drawn_lists(7 * T + K, T, 60, K)
    rows = np.random.default_rng(3).integers(1, 60, size=60)
    for args in ((10, 0.2, 0.02, 40), (1, 1.0, 0.0, 50), (30, 0.05, 0.1, 30)):
        best, dec = api.map_decide_loci(hits, count, rows, *args)
        want_best, want_dec = ref.decide_loci(hits, count, rows, *args)
        assert best.tolist() == want_best and dec.tolist() == want_dec, args


def test_map_decide_loci_equals_map_decide_with_one_hit_per_target():
    from squigglekit_amd import api
    rng = np.random.default_rng(9)
    for T in (2, 3, 5):
        m = 80
        rec = np.zeros((T, m), dtype=api.MAPREC_DTYPE)
        rec["dist"] = rng.integers(0, 8, size=(T, m)).astype(np.float64)
        rec["start"], rec["end"], rec["n"] = 3, 9, 50
        rec["rows"] = rng.integers(0, 50, size=m)[None, :]
        none = rec["rows"] == 0
        rec["dist"][none], rec["start"][none], rec["end"][none] = np.nan, -1, -1
        hits = api.map_hits(rec)[:, :, None]
        count = (~np.isnan(rec["dist"])).astype(np.int32)
        for args in ((10, 0.2, 0.02, 40), (1, 1.0, 0.0, 45), (20, 0.5, 0.1, 30)):
            want = api.map_decide(rec, *args)
            for rows in (rec["rows"], rec["rows"][0]):
                got = api.map_decide_loci(hits, count, rows, *args)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (T, args)


def test_a_lone_locus_has_an_infinite_margin_and_passes():
    from squigglekit_amd import api
    hits = np.zeros((1, 2, 2), dtype=ref.HIT)
    hits["dist"], hits["start"], hits["end"], hits["n"] = np.nan, -1, -1, 90
    hits[0, 0, 0] = (4.0, 10, 30, 90, 0)
    hits[0, 1, 0], hits[0, 1, 1] = (4.0, 10, 30, 90, 0), (4.5, 50, 70, 90, 0)
    count = np.array([[1, 2]], dtype=np.int32)
    best, rec, second = api.locus_margin(hits, count)
    assert best.tolist() == [0, 0] and second[0] == np.inf and second[1] == 4.5
    _, dec = api.map_decide_loci(hits, count, np.array([20, 20]), 10, 1.0, 0.1, 100)
    assert dec.tolist() == [1, 0]                       # the repeat's second copy is 0.025 a row away: wait
    with pytest.raises(ValueError):
        api.merge_tile_hits(hits, count, {"target": np.zeros(1, int), "origin": np.zeros(1, int), "length": np.array([90])}, 0)
