"""CPU: the references of the pair-list DTW agree with each other, and the host helpers around the call (pool and pair
packing, all-pairs matrix, best target, tiling and merging, the command line's formatting and argument checks) do what
they document -- the GPU call answered by the references where one is needed."""
import os

import numpy as np
import pytest

import pairs_ref
from conftest import GOLD
from test_cli import run_cli

MODEL = os.path.join(GOLD, "CATCTATCCAGGGTTAAATT.model")


def cases_300():
    rng = np.random.default_rng(2024)
    for k in range(300):
        N, M = int(rng.integers(1, 31)), int(rng.integers(1, 31))
        yield pairs_ref.draw(rng, N, k % 3 == 0), pairs_ref.draw(rng, M, k % 3 == 0)


def test_loop_dp_equals_the_sentinel_identity(ora):
    """300 seeded cases, one third tie-heavy integers in [-3, 3]: bits of the distance; start 0, end M + 1"""
    for x, y in cases_300():
        d, s, e = pairs_ref.dtw_global_sentinel(ora, x, y)
        assert pairs_ref.bits(d) == pairs_ref.bits(pairs_ref.dtw_global(x, y)), (x, y)
        assert (s, e) == (0, y.size + 1)


def test_global_distance_is_symmetric_bit_for_bit():
    for x, y in cases_300():
        assert pairs_ref.bits(pairs_ref.dtw_global(x, y)) == pairs_ref.bits(pairs_ref.dtw_global(y, x))


def test_global_definition_on_a_worked_case():
    # D = [[1, 3], [1, 2], [3, 1+... ]]: x = (0, 1, 3), y = (1, 2)
    #   |0-1| = 1, 1 + |0-2| = 3;  1 + |1-1| = 1, |1-2| + min(3, 1, 1) = 2;  1 + |3-1| = 3, |3-2| + min(2, 1, 3) = 2
    assert pairs_ref.dtw_global([0, 1, 3], [1, 2]) == 2.0
    assert pairs_ref.dtw_global([5], [1, 2, 3]) == 4 + 3 + 2
    assert pairs_ref.dtw_global([1, 2, 3], [5]) == 4 + 3 + 2


def test_pool_and_pair_packing():
    from squigglekit_amd import _lib, api
    assert api.PAIR_DTYPE.itemsize == 8 and (_lib.SK_PAIRS_SUBSEQUENCE, _lib.SK_PAIRS_GLOBAL) == (0, 1)
    values, off = api._as_pool([[1, 2, 3], [], np.arange(2)])
    assert values.dtype == np.float64 and values.tolist() == [1, 2, 3, 0, 1] and off.tolist() == [0, 3, 3, 5]
    v2, o2 = api._as_pool((values, off))
    assert v2 is values or v2.tolist() == values.tolist()
    assert o2.tolist() == off.tolist()
    with pytest.raises(ValueError):
        api._as_pool((values, np.array([0, 4, 3])))
    with pytest.raises(ValueError):
        api._as_pool((values, np.array([0, 9])))
    pr = api._as_pairs([(0, 2), (2, 0)])
    assert pr.dtype == api.PAIR_DTYPE and pr["query"].tolist() == [0, 2] and pr["target"].tolist() == [2, 0]
    assert api._as_pairs(np.zeros((0, 2))).shape == (0,)
    with pytest.raises(ValueError):
        api._as_pairs([(0, 2 ** 31)])
    with pytest.raises(ValueError):
        api.dtw_pairs([[1.0]], [(0, 0)], mode="banded")


@pytest.fixture
def ref_backend(monkeypatch, ora):
    """api.dtw_pairs answered by the references (tests may use them as a fake); records what was asked"""
    from squigglekit_amd import api
    asked = []

    def fake(seqs, pairs, mode="subsequence"):
        values, off = api._as_pool(seqs)
        pr = api._as_pairs(pairs)
        asked.append((pr.copy(), mode))
        pool = [values[off[i]:off[i + 1]] for i in range(off.size - 1)]
        return pairs_ref.records(ora, pool, list(zip(pr["query"].tolist(), pr["target"].tolist())), mode).astype(api.HIT_DTYPE)
    monkeypatch.setattr(api, "dtw_pairs", fake)
    return asked


def test_dtw_matrix_computes_the_upper_triangle_with_the_shorter_as_query(ref_backend, ora):
    from squigglekit_amd import api
    rng = np.random.default_rng(3)
    seqs = [rng.normal(size=n) for n in (5, 9, 3, 9, 4)]
    d = api.dtw_matrix(seqs)
    pr, mode = ref_backend[0]
    assert mode == "global" and len(pr) == 10
    lens = [len(s) for s in seqs]
    for q, t in zip(pr["query"], pr["target"]):
        assert q != t and (lens[q] < lens[t] or (lens[q] == lens[t] and q < t))
    assert np.array_equal(d, d.T) and np.all(np.diag(d) == 0.0)
    for i in range(5):
        for j in range(i + 1, 5):
            assert pairs_ref.bits(d[i, j]) == pairs_ref.bits(pairs_ref.dtw_global(seqs[i], seqs[j]))
    full = api.dtw_matrix(seqs, mode="subsequence")
    assert full.shape == (5, 5) and ref_backend[1][1] == "subsequence" and len(ref_backend[1][0]) == 25
    assert full[2, 1] == ora.dtw_subsequence(seqs[2], seqs[1])[0] and full[1, 2] == ora.dtw_subsequence(seqs[1], seqs[2])[0]


def test_map_queries_and_best_target_ties(ref_backend):
    from squigglekit_amd import api
    q = [np.array([1.0, 2.0]), np.array([0.0, 0.0, 0.0])]
    t = [np.array([9.0, 1.0, 2.0, 9.0]), np.array([1.0, 2.0]), np.zeros(0), np.array([1.0, 2.0, 7.0])]
    rec, best = api.map_queries(q, t)
    assert rec.shape == (4, 2)
    assert rec["dist"][:, 0].tolist()[:2] == [0.0, 0.0] and np.isnan(rec["dist"][2, 0]) and rec["flags"][2, 0] == 1
    assert best.tolist()[0] == 0                                   # targets 0, 1 and 3 tie at 0.0: the smallest index
    assert (rec["start"][0, 0], rec["end"][0, 0], rec["n"][0, 0]) == (1, 2, 4)
    allnan = np.zeros((2, 1), dtype=api.HIT_DTYPE)
    allnan["dist"] = np.nan
    assert api.best_targets(allnan).tolist() == [-1]
    assert api.best_targets(np.zeros((0, 3), dtype=api.HIT_DTYPE)).tolist() == [-1, -1, -1]


def test_tile_targets_geometry():
    from squigglekit_amd import api
    y = np.arange(600.0)
    pieces, tiling = api.tile_targets([y, np.arange(150.0), np.zeros(0)], 200, 120)
    assert tiling["length"].tolist() == [600, 150, 0]
    assert tiling["origin"][tiling["target"] == 0].tolist() == [0, 80, 160, 240, 320, 400]
    assert [len(p) for p in pieces[:6]] == [200] * 6 and pieces[5][-1] == 599.0
    assert tiling["target"].tolist()[6:] == [1, 2] and len(pieces[6]) == 150 and len(pieces[7]) == 0
    # every window of at most `overlap` points lies inside one piece
    for a in range(600 - 120 + 1):
        assert any(o <= a and a + 120 <= o + len(p) for o, p in zip(tiling["origin"][:6], pieces[:6])), a
    pieces, tiling = api.tile_targets([np.arange(10.0)], 4, 0)
    assert tiling["origin"].tolist() == [0, 4, 8] and [len(p) for p in pieces] == [4, 4, 2]
    for bad in ((4, 4), (4, -1), (0, 0)):
        with pytest.raises(ValueError):
            api.tile_targets([y], *bad)


def test_merge_tiles_equals_the_whole_target_on_planted_matches(ora):
    """100 planted cases (M = 600, piece 200, overlap 120): wherever the whole-target match spans at most `overlap`
    points -- at least 90 of them with this construction -- dist (bits), start and end equal the whole target's"""
    from squigglekit_amd import api
    held = 0
    for q, y in pairs_ref.planted_cases():
        whole = pairs_ref.oracle_map(ora, [q], [y])
        pieces, tiling = api.tile_targets([y], 200, 120)
        merged = api.merge_tiles(pairs_ref.oracle_map(ora, [q], pieces).astype(api.HIT_DTYPE), tiling)
        assert merged.shape == (1, 1) and merged["n"][0, 0] == 600
        assert merged["dist"][0, 0] >= whole["dist"][0, 0]          # no piece does better than the whole target
        if whole["end"][0, 0] - whole["start"][0, 0] + 1 <= 120:
            held += 1
            assert pairs_ref.same_records(merged, whole.astype(api.HIT_DTYPE)), (merged, whole)
    assert held >= 90, held


def test_merge_tiles_ties_and_empty_targets():
    from squigglekit_amd import api
    tiling = {"target": np.array([0, 0, 1]), "origin": np.array([0, 80, 0]), "length": np.array([280, 0])}
    rec = np.zeros((3, 2), dtype=api.HIT_DTYPE)
    rec[0] = [(1.5, 100, 110, 200, 0), (2.0, 5, 9, 200, 0)]
    rec[1] = [(1.5, 10, 20, 200, 0), (1.0, 150, 160, 200, 0)]       # query 0: equal dist, end 100 < 110
    rec[2] = [(np.nan, -1, -1, 0, 1)] * 2
    out = api.merge_tiles(rec, tiling)
    assert out[0, 0].tolist() == (1.5, 90, 100, 280, 0) and out[0, 1].tolist() == (1.0, 230, 240, 280, 0)
    assert np.isnan(out["dist"][1]).all() and out["start"][1].tolist() == [-1, -1] and out["flags"][1].tolist() == [1, 1]


def test_cli_argument_errors_and_lines(tmp_path):
    from squigglekit_amd import api
    from squigglekit_amd.map_cli import HEADER, load_targets, main, map_lines, zscore
    assert HEADER == ("readID", "target", "strand", "start", "end", "events", "dist", "dist_per_event", "second_target",
                      "second_dist")
    so, se, code = run_cli(main, [])
    assert code == 1 and so == "" and "usage" in se
    for argv, msg in ((["-m", MODEL], "one of -s/--signal, --blow5, --i16 is needed"),
                      (["--i16", "x.npy"], "-m/--model is needed"),
                      (["--i16", "x.npy", "-m", MODEL, "--prefix", "0"], "--prefix must be at least 1"),
                      (["--i16", "x.npy", "-m", MODEL, "--piece", "8", "--overlap", "8"], "0 <= --overlap < --piece"),
                      (["--i16", "x.npy", "-m", MODEL, "--overlap", "8"], "--overlap needs --piece"),
                      (["-s", "x.tsv", "--blow5", "y.blow5", "-m", MODEL], "not allowed with")):
        so, se, code = run_cli(main, argv)
        assert code == 2 and msg in se and (so == "" or so.startswith("usage")), (argv, se)   # (the help follows the error)
    so, se, code = run_cli(main, ["--i16", "x.npy", "-m", str(tmp_path / "missing.model")])
    assert code == 2 and so == "" and "missing.model" in se
    assert zscore([1.0]) is None and zscore([2.0, 2.0]) is None and zscore([1.0, 3.0]).tolist() == [-1.0, 1.0]
    targets = load_targets(MODEL, both=True)
    assert [(n, s) for n, s, _ in targets] == [("3_prime_end", "+"), ("3_prime_end", "-")]
    assert len(targets[0][2]) == 20 and targets[1][2].tolist() == targets[0][2][::-1].tolist()
    assert abs(targets[0][2].mean()) < 1e-12 and abs(targets[0][2].std() - 1.0) < 1e-12
    rec = np.zeros((2, 1), dtype=api.HIT_DTYPE)
    rec[:, 0] = [(3.0, 2, 9, 20, 0), (1.5, 4, 8, 20, 0)]
    lines = map_lines(["r0", "r1"], [None, np.zeros(6)], rec, targets)
    assert lines == ["r0\t.\t.\t.\t.\t.\t.\t.\t.\t.\n",
                     "r1\t3_prime_end\t-\t4\t8\t6\t1.5\t0.25\t3_prime_end+\t3.0\n"]
    assert map_lines(["r"], [np.zeros(3)], rec[:1], targets[:1]) == ["r\t3_prime_end\t+\t2\t9\t3\t3.0\t1.0\t.\t.\n"]
