"""Warping paths over a pair list, host side: the references of tests/pair_paths_ref.py held to each other, the span
invariants, the ragged layout (span_off), spans <-> path in both modes, the --align table's lines."""
import numpy as np
import pytest

import pair_paths_ref as ppr
import pairs_ref


def small_cases(count=200, seed=41):
    """(x, y): N and M from 1 to 40 (N > M included), every other case tie-heavy integers"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        N, M = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        if k < 8:
            N, M = ((1, 1), (1, 40), (40, 1), (2, 1), (1, 2), (40, 3), (3, 40), (40, 40))[k]
        out.append((pairs_ref.draw(rng, N, k % 2 == 0), pairs_ref.draw(rng, M, k % 2 == 0)))
    return out


def test_sentinel_path_is_the_plain_global_path(ora):
    """the oracle's path of [B] + x + [-B] in [B] + y + [-B], stripped and shifted, is mlpy's path() over the plain
    double-loop matrix -- and that matrix's corner has the bits of the sentinel distance"""
    cases = small_cases()
    assert sum(len(x) > len(y) for x, y in cases) > 40
    for x, y in cases:
        dist, px, py = ppr.global_path_plain(x, y)
        sx, sy = ppr.global_path_sentinel(ora, x, y)
        assert np.array_equal(px, sx) and np.array_equal(py, sy), (x, y)
        assert pairs_ref.bits(dist) == pairs_ref.bits(pairs_ref.dtw_global_sentinel(ora, x, y)[0])
        assert pairs_ref.bits(dist) == pairs_ref.bits(pairs_ref.dtw_global(x, y))


def test_span_invariants_in_both_modes(ora):
    for x, y in small_cases(120, seed=42):
        sp = ppr.spans(ora, x, y, "global", plain=True)
        ppr.check_invariants(sp, "global", 0, len(y) - 1)
        assert np.array_equal(sp, ppr.spans(ora, x, y, "global"))
        _, s, e = ora.dtw_subsequence(x, y)
        ppr.check_invariants(ppr.spans(ora, x, y, "subsequence"), "subsequence", s, e)


def test_global_path_of_single_rows_and_columns(ora):
    x, y = np.array([1.0]), np.array([3.0, 1.0, 2.0])
    assert ppr.spans(ora, x, y, "global", plain=True).tolist() == [[0, 2]]               # row 0 covers the whole target
    assert ppr.spans(ora, y, x, "global", plain=True).tolist() == [[0, 0], [0, 0], [0, 0]]
    assert ppr.spans(ora, x, np.zeros(0), "global").tolist() == [[-1, -1]]


def test_span_off_counts_a_repeated_query_once_per_pair():
    from squigglekit_amd import api
    seqs = [np.zeros(3), np.zeros(10), np.zeros(5), np.zeros(0)]
    _, off = api._as_pool(seqs)
    pairs = [(0, 1), (2, 1), (0, 2), (0, 0), (2, 3), (1, 0)]
    so = api.pair_span_off(off, pairs)
    assert so.dtype == np.int64 and so.tolist() == [0, 3, 8, 11, 14, 19, 29]
    assert api.pair_span_off(off, []).tolist() == [0]
    off7 = off + 7                                                  # a pool that does not start at 0
    assert np.array_equal(api.pair_span_off(off7, pairs), so)


def test_list_spans_layout(ora):
    rng = np.random.default_rng(2)
    seqs = [rng.normal(size=n) for n in (4, 9, 6)]
    pairs = [(0, 1), (2, 1), (0, 2), (0, 1)]
    for mode in ("subsequence", "global"):
        off, sp = ppr.list_spans(ora, seqs, pairs, mode)
        assert off.tolist() == [0, 4, 10, 14, 18] and sp.shape == (18, 2)
        assert np.array_equal(sp[0:4], sp[14:18])
        assert np.array_equal(sp[4:10], ppr.spans(ora, seqs[2], seqs[1], mode))


def test_expand_path_round_trips_in_both_modes(ora):
    from squigglekit_amd import api
    for x, y in small_cases(60, seed=43):
        _, px, py = ppr.global_path_plain(x, y)
        sp = ppr.spans_of(px, py, len(x))
        ex, ey = api.expand_path(sp)
        assert np.array_equal(ex, px) and np.array_equal(ey, py)                       # row 0's run [0, b_0] included
        assert (ex[0], ey[0]) == (0, 0) and (ex[-1], ey[-1]) == (len(x) - 1, len(y) - 1)
        assert np.array_equal(api.spans_of_path(ex, ey, len(x)), sp)
        qx, qy = ora.dtw_subsequence_path(x, y)
        sq = ppr.spans_of(qx, qy, len(x))
        ex, ey = api.expand_path(sq)
        assert np.array_equal(ex, qx) and np.array_equal(ey, qy)
    ex, ey = api.expand_path(np.full((5, 2), -1, dtype=np.int32))
    assert ex.size == 0 and ey.size == 0


def test_align_lines_format():
    from squigglekit_amd import api
    from squigglekit_amd.map_cli import ALIGN_HEADER, align_lines
    assert ALIGN_HEADER == ("readID", "target", "strand", "event", "sample_start", "sample_length", "level", "z",
                            "ref_first", "ref_last")
    ev = np.zeros(3, dtype=api.DET_EVENT_DTYPE)
    ev["start"], ev["length"] = [0, 7, 19], [7, 12, 5]
    lev = np.array([401.5, 1.0 / 3.0, 388.0])
    z = np.array([1.25, -0.1, 1e-17])
    spans = np.array([[4, 4], [4, 6], [7, 7]], dtype=np.int32)
    lines = align_lines("r1", ("recA", "-", None), ev, lev, z, spans)
    assert lines == ["r1\trecA\t-\t0\t0\t7\t401.5\t1.25\t4\t4\n",
                     "r1\trecA\t-\t1\t7\t12\t{}\t-0.1\t4\t6\n".format(1.0 / 3.0),
                     "r1\trecA\t-\t2\t19\t5\t388.0\t1e-17\t7\t7\n"]
    assert align_lines("r1", ("recA", "+", None), ev, lev, z, np.full((3, 2), -1)) == []
    assert align_lines("r1", ("recA", "+", None), ev[:0], lev[:0], z[:0], np.zeros((0, 2))) == []


def test_cli_knows_align():
    from squigglekit_amd.map_cli import build_parser
    args = build_parser().parse_args(["--i16", "a.npy", "-m", "m", "--align", "out.tsv"])
    assert args.align == "out.tsv"
    assert build_parser().parse_args(["--i16", "a.npy", "-m", "m"]).align is None
