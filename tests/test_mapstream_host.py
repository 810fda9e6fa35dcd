"""CPU: the identity a mapping session rests on, shown on the reference itself -- the row-chained recurrence of
tests/mapstream_ref.py, carrying only the last row (D, S) between chunks, gives the oracle's one-shot record whatever the
cuts, bits of dist included -- and the host-only parts: map_decide, map_hits, the Python-side refusals, the flags of the
replay tool."""
import numpy as np
import pytest

import mapstream_ref as ref
import pairs_ref


@pytest.mark.parametrize("ties", [True, False], ids=["integers", "normal"])
def test_chained_rows_equal_the_oracle_one_shot(ora, ties):
    rng = np.random.default_rng(11 + ties)
    for N, M in ((2, 1), (3, 7), (9, 40), (31, 23), (40, 90)):
        x, y = pairs_ref.draw(rng, N, ties), pairs_ref.draw(rng, M, ties)
        want = ora.dtw_subsequence(x, y)
        one = ref.chained_record([x], y)
        assert (pairs_ref.bits(one[0]), one[1], one[2]) == (pairs_ref.bits(want[0]), want[1], want[2]), (N, M)
        for name, lens in ref.splits_of(N).items():
            got = ref.chained_record(ref.cut(x, lens), y)
            assert (pairs_ref.bits(got[0]), got[1], got[2]) == (pairs_ref.bits(want[0]), want[1], want[2]), (N, M, name)


def test_chained_record_after_every_chunk_is_the_prefix_record(ora):
    rng = np.random.default_rng(3)
    x, y = pairs_ref.draw(rng, 30, True), pairs_ref.draw(rng, 50, True)
    state, seen = None, 0
    for n in (1, 4, 1, 9, 15):
        state = ref.chained_rows(x[seen:seen + n], y, state)
        seen += n
        d, s, e = ref.record_of(state)
        want = ora.dtw_subsequence(x[:seen], y)
        assert (pairs_ref.bits(d), s, e) == (pairs_ref.bits(want[0]), want[1], want[2]), seen


def rec_of(dist, rows):
    from squigglekit_amd import api
    dist = np.asarray(dist, dtype=np.float64)
    rec = np.zeros(dist.shape, dtype=api.MAPREC_DTYPE)
    rec["dist"] = dist
    rec["rows"] = np.broadcast_to(np.asarray(rows), dist.shape)
    return rec


def test_map_decide_truth_table():
    from squigglekit_amd import api
    nan = np.nan
    #                 accept      margin small  too few rows  dist too high  give up      NaN col   tie -> target 0
    dist = np.array([[10.0,       10.0,         10.0,         90.0,          90.0,        nan,      20.0],
                     [40.0,       12.0,         40.0,         99.0,          99.0,        nan,      20.0]])
    rows = np.array([20,          20,           5,            20,            200,         0,        20])
    best, dec = api.map_decide(rec_of(dist, rows), min_rows=10, max_dist_per_row=1.0, min_margin=0.5, give_up_rows=100)
    assert best.tolist() == [0, 0, 0, 0, 0, -1, 0]
    assert dec.tolist() == [1, 0, 0, 0, -1, 0, 0] and dec.dtype == np.int8
    # one NaN target beside a good one: the margin to "nothing" is infinite
    best, dec = api.map_decide(rec_of([[nan], [10.0]], [20]), 10, 1.0, 0.5, 100)
    assert (best.tolist(), dec.tolist()) == ([1], [1])
    # one target: no margin test
    best, dec = api.map_decide(rec_of([[10.0, 90.0, 190.0, nan]], [20, 20, 100, 500]), 10, 1.0, 1e9, 100)
    assert (best.tolist(), dec.tolist()) == ([0, 0, 0, -1], [1, 0, -1, 0])
    # the boundaries are inclusive: rows == min_rows, dist / rows == the bound, margin == min_margin
    best, dec = api.map_decide(rec_of([[10.0], [15.0]], [10]), 10, 1.0, 0.5, 10)
    assert dec.tolist() == [1]
    best, dec = api.map_decide(rec_of([[10.0], [14.0]], [10]), 10, 1.0, 0.5, 10)
    assert dec.tolist() == [-1]                                         # not accepted, and rows == give_up_rows
    best, dec = api.map_decide(np.zeros((2, 0), dtype=api.MAPREC_DTYPE), 1, 1.0, 0.0, 1)
    assert best.shape == dec.shape == (0,)


def test_map_hits_feeds_merge_tiles():
    from squigglekit_amd import api
    rec = np.zeros((3, 2), dtype=api.MAPREC_DTYPE)
    rec["dist"] = [[5.0, 1.0], [2.0, 1.0], [7.0, 0.5]]
    rec["start"], rec["end"], rec["n"], rec["rows"] = 3, 9, 100, 44
    pieces, tiling = api.tile_targets([np.zeros(150), np.zeros(100)], 100, 50)
    assert len(pieces) == 3
    hits = api.map_hits(rec)
    assert hits.dtype == api.HIT_DTYPE and hits.shape == rec.shape
    merged = api.merge_tiles(hits, tiling)
    assert merged["dist"].tolist() == [[2.0, 1.0], [7.0, 0.5]]
    assert merged["start"].tolist() == [[53, 3], [3, 3]] and merged["n"].tolist() == [[150, 150], [100, 100]]


def test_python_validation_needs_no_device():
    from squigglekit_amd import api
    for targets, nslots, word in (([np.zeros(4), np.zeros(0)], 4, "target 1 is empty"), ([], 4, "targets"),
                                  ([np.zeros(4)], 0, "nslots"), ([np.zeros(4)], 65537, "nslots"),
                                  ([np.zeros(50000)], 65536, "row state of 39321600000 bytes")):
        with pytest.raises(ValueError, match=word):
            api.MapStream(targets, nslots)


@pytest.mark.parametrize("argv", [["--chunk", "0"], ["--channels", "0"], ["--channels", "70000"], ["--calib", "-1"],
                                  ["--min_events", "-2"], ["--give_up", "0"], ["--piece", "100", "--overlap", "100"],
                                  ["--overlap", "10"]])
def test_cli_rejects_bad_flags_before_the_header(argv, tmp_path, capsys):
    from squigglekit_amd import mapstream_cli
    sig = tmp_path / "s.i16"
    sig.write_bytes(b"")
    model = tmp_path / "m.model"
    model.write_text("pos\tbase\tcurrent\tsd\tdwell\n0\tA\t1.0\t0.1\t8\n")
    with pytest.raises(SystemExit) as e:
        mapstream_cli.main(["--i16", str(sig), "-m", str(model)] + argv)
    assert e.value.code != 0
    out = capsys.readouterr()
    assert "readID\t" not in out.out                                    # rejected before the header is printed
    assert argv[0].lstrip("-") in out.err
