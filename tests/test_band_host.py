"""CPU: the statement of the adaptive-band DTW (tests/band_ref.py) held to what it claims -- nothing here calls the
library.  Where the whole matrix lies in the band the record and the path are those of a plain double-loop matrix traced
in mlpy's path() order; elsewhere the banded distance bounds the full one from above; the spans are a path; the free end
is the first argmin; the corner alternates on ties."""
import numpy as np
import pytest

import band_ref as br

GRID = (1, 4, 7, 10, 13, 16, 19, 22, 25, 28, 31, 32)


@pytest.mark.parametrize("end", br.ENDS)
def test_whole_matrix_in_band_is_the_full_matrix_and_mlpys_path(end):
    """fact 1: N, M <= W / 2 = 32, tie-heavy integer sequences, all 144 shapes"""
    rng = np.random.default_rng(1)
    for N in GRID:
        for M in GRID:
            x, y = br.ties(rng, N), br.ties(rng, M)
            D = br.full_matrix(x, y)
            r = br.band(x, y, 64, end)
            e = M - 1 if end == "pinned" else int(np.argmin(D[-1]))
            assert (r["dist"], r["start"], r["end"], r["n"], r["flags"]) == (D[-1][e], 0, e, M, 0), (N, M)
            assert np.array_equal(r["spans"], br.full_path_spans(D, e)), (N, M)
            br.check_invariants(r["spans"], e)


def test_wider_bands_hold_larger_matrices_whole():
    rng = np.random.default_rng(2)
    for W, n in ((128, 64), (256, 128), (128, 33), (256, 65)):
        x, y = br.ties(rng, n), br.ties(rng, n - 1)
        D = br.full_matrix(x, y)
        for end in br.ENDS:
            e = len(y) - 1 if end == "pinned" else int(np.argmin(D[-1]))
            r = br.band(x, y, W, end)
            assert (r["dist"], r["end"]) == (D[-1][e], e)
            assert np.array_equal(r["spans"], br.full_path_spans(D, e))


def test_banded_distance_bounds_the_full_one_from_above():
    """fact 2: beyond N, M <= W / 2 the band may miss the optimum, never undercut it; wider bands never do worse here"""
    rng = np.random.default_rng(3)
    cases = [(rng.normal(size=700), rng.normal(size=90)), (rng.normal(size=90), rng.normal(size=700)),
             br.drift_pair(rng, 400, 0.3, 0.5, 0), br.drift_pair(rng, 400, 0.55, 0.3, 120),
             (br.ties(rng, 300), br.ties(rng, 280))]
    larger = 0
    for x, y in cases:
        last = br.full_distance(x, y)
        for W in br.WIDTHS:
            r = br.band(x, y, W, "pinned")
            assert not r["lost"] and r["dist"] >= last[-1], (len(x), len(y), W)
            larger += r["dist"] > last[-1]
            br.check_invariants(r["spans"], len(y) - 1)
            f = br.band(x, y, W, "free")
            assert f["dist"] >= last.min() and f["dist"] <= r["dist"]
            br.check_invariants(f["spans"], f["end"])
    assert larger > 0                                               # (700 x 90 at W = 64 does miss it)


def test_full_distance_by_diagonals_is_the_double_loop():
    rng = np.random.default_rng(4)
    for N, M in ((1, 1), (1, 9), (9, 1), (17, 23), (40, 12)):
        x, y = br.ties(rng, N), rng.normal(size=M)
        assert br.full_distance(x, y).tolist() == br.full_matrix(x, y)[-1]


def test_span_invariants_on_hugging_shapes():
    rng = np.random.default_rng(5)
    for N, M in ((1, 500), (500, 1), (2, 300), (300, 2), (700, 90), (90, 700)):
        x, y = rng.normal(size=N), rng.normal(size=M)
        for end in br.ENDS:
            r = br.band(x, y, 64, end)
            assert not r["lost"] and r["flags"] == 0 and r["start"] == 0 and r["n"] == M
            br.check_invariants(r["spans"], r["end"])
            assert r["end"] == M - 1 or end == "free"
            # the spans are a path whose cost is the distance, added in path order
            c = 0.0
            for i in range(N):
                for j in range(r["spans"][i, 0], r["spans"][i, 1] + 1):
                    c = abs(x[i] - y[j]) + c
            assert c == r["dist"]


def test_free_end_is_the_first_strictly_smallest_of_the_last_row():
    x = np.array([0.0, 1.0, 2.0])
    y = np.array([0.0, 1.0, 2.0, 2.0, 2.0, 5.0, 2.0])              # row 2 is 0 at columns 2, 3, 4: the first wins
    r = br.band(x, y, 64, "free")
    assert (r["dist"], r["end"]) == (0.0, 2) and r["spans"].tolist() == [[0, 0], [1, 1], [2, 2]]
    p = br.band(x, y, 64, "pinned")
    assert (p["dist"], p["end"]) == (3.0, 6) and p["spans"][-1].tolist()[1] == 6


def test_move_rule_on_an_all_ties_input():
    """constant sequences: every live cell costs 0, both band ends are equal (or both +inf) after every band, so the
    corner moves right after even bands and down after odd ones -- and the path is the diagonal"""
    x, y = np.zeros(200), np.zeros(200)
    r = br.band(x, y, 64, "pinned")
    assert r["moves"].tolist() == [b & 1 for b in range(398)]
    assert r["corners"][0].tolist() == [32, -32] and r["corners"][-1].tolist() == [32 + 199, -32 + 199]
    assert r["dist"] == 0.0 and r["spans"].tolist() == [[i, i] for i in range(200)]
    # a cheaper upper-right end pulls the corner right, a cheaper lower-left end pulls it down
    x, y = np.zeros(100), np.concatenate([np.zeros(40), np.full(300, 0.0)])
    assert br.band(x, y, 64, "pinned")["dist"] == 0.0


def test_empty_target_and_record_shape():
    r = br.band(np.ones(5), np.zeros(0), 128, "free")
    assert np.isnan(r["dist"]) and (r["start"], r["end"], r["n"], r["flags"]) == (-1, -1, 0, br.FLAG_EMPTY)
    assert np.all(r["spans"] == -1) and r["spans"].shape == (5, 2)
    rec, off, spans, lost = br.records([np.ones(5), np.zeros(0), np.arange(7.0)], [(0, 1), (0, 2), (2, 0), (0, 2)], 64, "pinned")
    assert off.tolist() == [0, 5, 10, 17, 22] and spans.shape == (22, 2) and lost == 0
    assert rec["flags"].tolist() == [1, 0, 0, 0] and rec[1] == rec[3]


def test_mismatches_counts_lost_corners_and_failed_walks_but_no_empty_target():
    """what a call with paths must count: an inf in the query loses the corner; an empty target has no path and is not
    counted; `records` goes on returning the lost pairs alone"""
    rng = np.random.default_rng(6)
    x = br.ties(rng, 90)
    seqs = [x, br.ties(rng, 80), np.zeros(0), br.lay_non_finite(rng, x, x, "+inf in a query")[0]]
    pairs = [(0, 1), (0, 2), (3, 1), (3, 1), (1, 0)]
    rec, off, spans, lost = br.records(seqs, pairs, 64, "pinned")
    assert lost == 2 and rec["flags"].tolist() == [0, br.FLAG_EMPTY, br.FLAG_BAND_LOST, br.FLAG_BAND_LOST, 0]
    assert br.mismatches(seqs, pairs, off, spans) == 2
    spans[off[4]:off[5]] = -1                                       # a walk that failed: counted, though not lost
    assert br.mismatches(seqs, pairs, off, spans) == 3
    assert np.isinf(seqs[3]).sum() == 1 and np.isfinite(x).all()    # lay_non_finite works on a copy


def test_every_non_finite_kind_lays_a_value_even_into_one_point():
    rng = np.random.default_rng(7)
    for kind in br.NONFINITE:
        for _ in range(20):
            x, y = br.lay_non_finite(rng, np.zeros(1), np.zeros(1), kind)
            assert np.isfinite(x).all() != np.isfinite(y).all(), kind
    # a pair without rows has no first row to look at: not counted, and the next pair's rows are not read for it
    off = np.array([0, 0, 3], dtype=np.int64)
    spans = np.full((3, 2), -1, dtype=np.int32)
    assert br.mismatches([np.zeros(0), np.zeros(3)], [(0, 1), (1, 1)], off, spans) == 1
