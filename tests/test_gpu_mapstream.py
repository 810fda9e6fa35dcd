"""GPU: mapping sessions (sk_map_*, api.MapStream, squiggle_map_stream) against the oracle's dtw_subsequence on the
concatenation of everything a slot has been given -- after EVERY push, bits of dist included.  The reference is never
the code under test: tests/mapstream_ref.Shadow keeps the points per slot and asks the oracle."""
import numpy as np
import pytest

import detect_ref
import mapstream_ref as ref
import pairs_ref

pytestmark = pytest.mark.gpu

LENS = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
TARGET_LENS = (1, 2, 17, 200, 777, 1500)


def check_push(ms, sh, slots, chunks, tag):
    got, want = ms.push(slots, chunks), sh.push(slots, chunks)
    diff = ref.first_difference(got, want)
    assert diff is None, "%s: %s" % (tag, diff)
    return got


def test_split_grid_in_one_session(gpu, ora):
    """every chunk length as a slot's first chunk and as a later one, all slots pushed together: every (L, R) group is
    live, fresh and continuing entries share wavefronts, chunks above 1 024 points are swept in pieces"""
    from squigglekit_amd import api
    rng = np.random.default_rng(41)
    targets = [pairs_ref.draw(rng, M, t % 2 == 0) for t, M in enumerate(TARGET_LENS)]
    S = len(LENS)
    sh = ref.Shadow(ora, targets, S)
    with api.MapStream(targets, S) as ms:
        for step, shift in enumerate((0, 7, 11)):
            chunks = [pairs_ref.draw(rng, LENS[(k + shift) % S], k % 2 == 0) for k in range(S)]
            got = check_push(ms, sh, list(range(S)), chunks, "push %d" % step)
            assert got["pushes"].min() == got["pushes"].max() == step + 1
        plan = api.last_map_plan()
        assert plan["state_bytes"] == S * sum(TARGET_LENS) * 12
        assert plan["entries"] == (S + 3) * len(TARGET_LENS)             # 1 025 and 2 049 have a second, 2 049 a third piece
        assert plan["launches"] > 3


@pytest.mark.parametrize("S", [1, 3, 4, 5, 15, 16, 17, 33])
def test_wave_mates_fresh_and_continuing(gpu, ora, S):
    """one shape group (chunks of 10 points: L = 16, four entries per wavefront), slots alternately fresh and continuing,
    target lengths alternating between {1, 2, 3} and 1 500 .. 2 000"""
    from squigglekit_amd import api
    rng = np.random.default_rng(100 + S)
    targets = [pairs_ref.draw(rng, M, t % 2 == 1) for t, M in enumerate((1, 1500, 2, 1750, 3, 2000))]
    sh = ref.Shadow(ora, targets, S)
    with api.MapStream(targets, S) as ms:
        odd = list(range(1, S, 2))
        if odd:
            check_push(ms, sh, odd, [pairs_ref.draw(rng, 10, s % 4 == 1) for s in odd], "odd slots")
        every = list(range(S))
        check_push(ms, sh, every, [pairs_ref.draw(rng, 10, s % 4 == 1) for s in every], "all slots")
        check_push(ms, sh, every, [pairs_ref.draw(rng, 10, s % 4 == 1) for s in every], "all slots again")


def test_row_state_in_place_long_target_and_single_points(gpu, ora):
    """chunks of 1 024 points (L = 64, R = 16) three times against a target of 5 000 points: the stored row is read a block
    ahead of where it is rewritten; and chunks of 1 point 40 times"""
    from squigglekit_amd import api
    rng = np.random.default_rng(7)
    targets = [pairs_ref.draw(rng, 5000, False)]
    sh = ref.Shadow(ora, targets, 2)
    with api.MapStream(targets, 2) as ms:
        for step in range(3):
            check_push(ms, sh, [0], [pairs_ref.draw(rng, 1024, False)], "1 024 points, push %d" % step)
        for step in range(40):
            check_push(ms, sh, [1], [pairs_ref.draw(rng, 1, step % 2 == 0)], "1 point, push %d" % step)
        check_push(ms, sh, [0, 1], [pairs_ref.draw(rng, 1024, True), pairs_ref.draw(rng, 1, True)], "both")


def test_past_the_old_limit_of_1024_points(gpu, ora):
    from squigglekit_amd import api
    rng = np.random.default_rng(9)
    targets = [pairs_ref.draw(rng, 400, True), pairs_ref.draw(rng, 1300, False)]
    x = pairs_ref.draw(rng, 3000, False)
    sh = ref.Shadow(ora, targets, 1)
    with api.MapStream(targets, 1) as ms:
        for a in range(0, 3000, 700):
            got = check_push(ms, sh, [0], [x[a:a + 700]], "points %d .." % a)
        assert got["rows"].tolist() == [[3000], [3000]] and got["pushes"].tolist() == [[5], [5]]


def test_bookkeeping(gpu, ora):
    from squigglekit_amd import _lib, api
    rng = np.random.default_rng(13)
    targets = [pairs_ref.draw(rng, 90, True), pairs_ref.draw(rng, 300, False), pairs_ref.draw(rng, 5, True)]
    draw = lambda n: pairs_ref.draw(rng, n, False)                      # noqa: E731
    sh = ref.Shadow(ora, targets, 4)
    with api.MapStream(targets, 4) as ms:
        empty = ms.peek([2, 0])                                         # no points yet
        assert ref.first_difference(empty, sh.push([2, 0], [np.zeros(0)] * 2)) is None
        assert np.isnan(empty["dist"]).all() and (empty["start"] == -1).all() and (empty["rows"] == 0).all()
        assert empty["n"].tolist() == [[90, 90], [300, 300], [5, 5]]
        # interleaved subsets: slot 0 in pushes 1, 3, 5; slot 1 in pushes 2, 4
        for step in range(5):
            s = step % 2
            got = check_push(ms, sh, [s], [draw(20 + step)], "interleaved push %d" % step)
            assert got["pushes"][0, 0] == step // 2 + 1
        # a peek returns the last record, and changes nothing
        last = ms.push([1, 0], [draw(0), draw(0)])
        assert ref.first_difference(last, sh.push([1, 0], [np.zeros(0)] * 2)) is None
        assert ms.peek([1, 0]).tobytes() == last.tobytes()
        assert last["rows"].tolist() == [[21 + 23, 20 + 22 + 24]] * 3 and last["pushes"].tolist() == [[2, 3]] * 3
        # a chunk and a peek in one push
        check_push(ms, sh, [3, 0, 1], [draw(7), draw(0), draw(40)], "mixed push")
        # a reset mid-read: the new read's records, the other slots' unchanged
        before = ms.peek([1, 3])
        ms.reset([0])
        sh.reset([0])
        assert (ms.peek([0])["rows"] == 0).all() and np.isnan(ms.peek([0])["dist"]).all()
        got = check_push(ms, sh, [0], [draw(33)], "after the reset")
        assert got["rows"].tolist() == [[33]] * 3 and got["pushes"].tolist() == [[1]] * 3
        assert ms.peek([1, 3]).tobytes() == before.tobytes()
        # two sessions at once do not share state
        other_targets = [pairs_ref.draw(rng, 60, True)]
        sh2 = ref.Shadow(ora, other_targets, 4)
        with api.MapStream(other_targets, 4) as ms2:
            assert ms2.handle != ms.handle
            check_push(ms2, sh2, [0, 1], [draw(12), draw(300)], "second session")
            check_push(ms, sh, [0, 1], [draw(5), draw(6)], "first session beside it")
            check_push(ms2, sh2, [1, 0], [draw(2), draw(2)], "second session again")
            h2 = ms2.handle
        # what the session alone can refuse
        L = _lib.load()
        for slots, word in (([4], "slot 4 is outside [0, 4)"),):
            sl = np.array(slots, dtype=np.int32)
            out = np.zeros((3, 1), dtype=api.MAPREC_DTYPE)
            rc = L.sk_map_push(ms.handle, _lib.ptr(sl), 1, _lib.ptr(np.zeros(1)), _lib.ptr(np.array([0, 1], dtype=np.int64)),
                               _lib.ptr(out))
            assert rc == _lib.SK_ERR_INVALID and word in L.sk_last_error().decode()
        assert L.sk_map_close(h2) == _lib.SK_ERR_INVALID and "unknown mapping session handle" in L.sk_last_error().decode()
        check_push(ms, sh, [0, 1], [draw(3), draw(3)], "after the refusals")
        h1 = ms.handle
    # open, close, open reuses cleanly: the handle comes back, the state does not
    with api.MapStream(targets, 4) as ms3:
        assert ms3.handle == h1
        assert (ms3.peek([0, 1, 2, 3])["rows"] == 0).all()
        sh3 = ref.Shadow(ora, targets, 4)
        check_push(ms3, sh3, [0], [draw(9)], "reopened")


def test_tiled_session_merges_to_whole_target_coordinates(gpu, ora):
    from squigglekit_amd import api
    queries, targets = pairs_ref.mapping_case(nq=24)
    pieces, tiling = api.tile_targets(targets, 1024, 512)
    Q = len(queries)
    with api.MapStream(pieces, Q) as ms:
        for part in (0, 1):
            chunks = [q[:len(q) // 2] if part == 0 else q[len(q) // 2:] for q in queries]
            sofar = [q[:len(q) // 2] if part == 0 else q for q in queries]
            rec = ms.push(list(range(Q)), chunks)
            want = api.merge_tiles(pairs_ref.oracle_map(ora, sofar, pieces).astype(api.HIT_DTYPE), tiling)
            got = api.merge_tiles(api.map_hits(rec), tiling)
            assert pairs_ref.same_records(got, want), part
    whole = pairs_ref.oracle_map(ora, queries, targets)                 # the planted matches span far less than the overlap
    best = api.best_targets(got)
    assert np.array_equal(best, api.best_targets(whole))
    col = np.arange(Q)
    assert pairs_ref.same_records(got[best, col], whole[best, col])


def test_device_entry_gives_the_bytes_of_the_host_entry(gpu):
    from squigglekit_amd import _lib, api
    L = _lib.load()
    rng = np.random.default_rng(21)
    targets = [pairs_ref.draw(rng, 333, False), pairs_ref.draw(rng, 40, True)]
    S, T = 6, 2
    d_vals, d_slots, d_out = L.sk_dev_alloc(S * 1100 * 8), L.sk_dev_alloc(S * 4), L.sk_dev_alloc(T * S * 32)
    try:
        with api.MapStream(targets, S) as host, api.MapStream(targets, S) as dev:
            for step in range(4):
                m = int(rng.integers(1, S + 1))
                slots = rng.permutation(S)[:m].astype(np.int32)
                lens = rng.choice([0, 1, 9, 70, 300, 1100], size=m)
                values = pairs_ref.draw(rng, int(lens.sum()) + 3, False)     # (the chunks start at off[0] = 3)
                off = (3 + np.concatenate([[0], np.cumsum(lens)])).astype(np.int64)
                want = host.push(slots, (values, off))
                _lib.check(L.sk_dev_upload(d_vals, _lib.ptr(values[3:] if lens.sum() else np.zeros(1)), max(8, int(lens.sum()) * 8)))
                _lib.check(L.sk_dev_upload(d_slots, _lib.ptr(slots), slots.nbytes))
                _lib.check(L.sk_map_push_dev(dev.handle, d_slots, m, d_vals, _lib.ptr(off), d_out))
                got = np.zeros((T, m), dtype=api.MAPREC_DTYPE)
                _lib.check(L.sk_dev_download(_lib.ptr(got), d_out, got.nbytes))
                assert got.tobytes() == want.tobytes(), step
            # the device form checks the slot numbers it reads back
            bad = np.array([1, 1], dtype=np.int32)
            _lib.check(L.sk_dev_upload(d_slots, _lib.ptr(bad), bad.nbytes))
            rc = L.sk_map_push_dev(dev.handle, d_slots, 2, d_vals, _lib.ptr(np.array([0, 1, 2], dtype=np.int64)), d_out)
            assert rc == _lib.SK_ERR_INVALID and "slot 1 appears twice" in L.sk_last_error().decode()
    finally:
        for p in (d_vals, d_slots, d_out):
            L.sk_dev_free(p)


# ---- command line ----------------------------------------------------------------------------------------------------
def run_cli(main, argv):
    import contextlib
    import io
    out, err = io.StringIO(), io.StringIO()
    code = 0
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            main(argv)
        except SystemExit as e:
            code = e.code if isinstance(e.code, int) else 1
    return out.getvalue(), err.getvalue(), code


def synthetic_input(tmp_path):
    """(reads.npy, ref.model, reads int16 [8, 9000], targets as load_targets makes them): six reads of 60 levels cut from
    two reference records, one constant read, one read of 1 200 short levels (more than 1 024 events)"""
    rng = np.random.default_rng(77)
    model = tmp_path / "ref.model"
    levels = {}
    with open(model, "w") as fh:
        for name, n in (("recA", 150), ("recB", 90)):
            levels[name] = np.array([float("%.3f" % v) for v in rng.uniform(60, 130, size=n)])   # (as the text reads back)
            fh.write("#%s\npos\tbase\tcurrent\tsd\tdwell\n" % name)
            for i, v in enumerate(levels[name]):
                fh.write("%d\tA\t%.3f\t1.5\t8.0\n" % (i, v))
    W = 9000
    reads = np.zeros((8, W), dtype=np.int16)
    for r in range(6):
        src = levels[("recA", "recB")[r % 2]]
        src = src[::-1] if r % 3 == 0 else src
        a = int(rng.integers(0, len(src) - 60))
        lev = np.repeat(src[a:a + 60] * 5.0, rng.integers(18, 32, size=60))
        reads[r, :len(lev)] = np.round(lev + rng.normal(scale=2.0, size=len(lev)))
        reads[r, len(lev):] = reads[r, len(lev) - 1]
    reads[6] = 7                                                        # one event: `.` fields in both tools
    long_lev = np.repeat(rng.permutation(np.tile(levels["recA"], 9))[:1200] * 5.0, 7)   # 1 200 levels of 7 samples
    reads[7, :len(long_lev)] = np.round(long_lev + rng.normal(scale=1.0, size=len(long_lev)))
    reads[7, len(long_lev):] = reads[7, len(long_lev) - 1]
    path = tmp_path / "reads.npy"
    np.save(path, reads)
    targets = []
    for name in ("recA", "recB"):
        z = pairs_ref.zscore(levels[name])
        targets += [(name, "+", z), (name, "-", z[::-1].copy())]
    return path, model, reads, targets


def event_levels(row):
    ev = detect_ref.events(row)
    return ev["sum"].astype(np.float64) / ev["length"].astype(np.float64)


def test_cli_replay_ends_on_the_lines_of_squiggle_map(gpu, ora, tmp_path):
    """squiggle_map_stream with --calib 0 and decision flags that never accept on synthetic int16 reads: every read ends
    with `end` and its first ten columns are the line squiggle_map prints (whole targets, then --piece / --overlap); the
    one read with more than 1 024 events, where squiggle_map prints `.`, is mapped -- its line is the oracle's record"""
    from squigglekit_amd import api
    from squigglekit_amd.map_cli import main as map_main
    from squigglekit_amd.map_cli import map_lines
    from squigglekit_amd.mapstream_cli import HEADER, main
    path, model, reads, targets = synthetic_input(tmp_path)
    W = reads.shape[1]
    q_long = event_levels(reads[7])
    assert len(q_long) > 1024                                           # past squiggle_map's limit
    q_long = (q_long - q_long.mean()) / q_long.std()
    ys = [t[2] for t in targets]

    base = ["--i16", str(path), "-m", str(model), "--both", "--prefix", str(W)]
    never = ["--calib", "0", "--chunk", "37", "--channels", "3", "--min_events", "1000000", "--give_up", "1000000"]
    for extra, pieces in (([], None), (["--piece", "64", "--overlap", "40"], (64, 40))):
        so, se, code = run_cli(map_main, base + extra)
        assert code == 0, se
        want = {ln.split("\t")[0]: ln.split("\t") for ln in so.split("\n")[1:-1]}
        assert len(want) == 8 and want["7"][1] == "." and want["6"][1] == "." and want["0"][1] != "."
        if pieces:
            cut, tiling = api.tile_targets(ys, *pieces)
            hits = api.merge_tiles(pairs_ref.oracle_map(ora, [q_long], cut).astype(api.HIT_DTYPE), tiling)
        else:
            hits = pairs_ref.oracle_map(ora, [q_long], ys).astype(api.HIT_DTYPE)
        want["7"] = map_lines(["7"], [q_long], hits, targets)[0][:-1].split("\t")
        so, se, code = run_cli(main, base + extra + never)
        assert code == 0, se
        lines = so.split("\n")
        assert lines[0] == "\t".join(HEADER) and lines[-1] == ""
        got = {ln.split("\t")[0]: ln.split("\t") for ln in lines[1:-1]}
        assert sorted(got) == sorted(want) and len(lines) == 10
        for rid, cols in got.items():
            assert len(cols) == 13 and cols[:10] == want[rid], (extra, rid, cols, want[rid])
            if rid == "6":
                assert cols[10:] == [".", "0", "0"]
                continue
            events = int(cols[5])
            assert cols[10] == "end" and int(cols[12]) == events and int(cols[11]) == -(-events // 37), (rid, cols)
        assert int(got["7"][5]) == len(q_long)


def test_cli_decides_at_the_first_record_that_accepts_or_gives_up(gpu, ora, tmp_path):
    """decision flags that accept at once, and flags that never accept and give up at 74 events, under --calib 0 and
    --calib 100: the line is printed at that push, with the oracle's record of the events seen so far"""
    from squigglekit_amd.map_cli import map_lines
    from squigglekit_amd.mapstream_cli import main, normalise
    path, model, reads, targets = synthetic_input(tmp_path)
    ys = [t[2] for t in targets]
    base = ["--i16", str(path), "-m", str(model), "--both", "--prefix", str(reads.shape[1]), "--chunk", "37", "--channels", "4"]
    accept = ["--min_events", "30", "--max_dist_per_event", "1e9", "--min_margin", "0", "--give_up", "1000000"]
    reject = ["--min_events", "1000000", "--give_up", "74"]
    for calib in (0, 100):
        for flags, word, pushes in ((accept, "accept", 1), (reject, "reject", 1 if calib == 100 else 2)):
            so, se, code = run_cli(main, base + ["--calib", str(calib)] + flags)
            assert code == 0, se
            got = {ln.split("\t")[0]: ln.split("\t") for ln in so.split("\n")[1:-1]}
            assert sorted(got) == [str(r) for r in range(8)]
            assert got["6"][1:] == ["."] * 10 + ["0", "0"]
            for r in (0, 1, 2, 3, 4, 5, 7):
                z = normalise(event_levels(reads[r]), calib)
                seen = max(37, calib) + 37 * (pushes - 1)
                hits = pairs_ref.oracle_map(ora, [z[:seen]], ys)
                want = map_lines([str(r)], [z[:seen]], hits, targets)[0][:-1].split("\t") + [word, str(pushes), str(seen)]
                assert got[str(r)] == want, (calib, word, r, got[str(r)], want)
