"""GPU: DTW over a pair list (sk_dtw_pairs, k_sdtw's MODE_PAIRS / MODE_PAIRS_GLOBAL) against references that are never
the code under test: the oracle's dtw_subsequence for the subsequence mode; for the global mode the oracle through the
sentinel identity that tests/test_pairs_host.py holds to the double-loop DP.  Bits of dist; start, end, n, flags equal."""
import ctypes as C
import os

import numpy as np
import pytest

import detect_ref
import pairs_ref
from test_cli import run_cli

pytestmark = pytest.mark.gpu
MODES = ("subsequence", "global")


def check(got, want, what=""):
    assert got.dtype.itemsize == 24
    assert pairs_ref.same_records(got, want.astype(got.dtype)), (what, [
        (p, got[p].tolist(), want[p].tolist()) for p in range(len(got))
        if not pairs_ref.same_records(got[p:p + 1], want[p:p + 1].astype(got.dtype))][:5])


# ---- shape grid ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid(ora):
    seqs, pairs = pairs_ref.shape_grid()
    return seqs, pairs, {m: pairs_ref.records(ora, seqs, pairs, m) for m in MODES}


@pytest.mark.parametrize("no_small", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_shape_grid_in_one_call(gpu, grid, monkeypatch, mode, no_small):
    """every query length around the lane and row boundaries against five target lengths, all in ONE call so that every
    (L, R) group is live and the scatter is exercised; as is, and with queries of up to 256 points at L = 16 too; the
    same list shuffled and with duplicates gives the same records"""
    from squigglekit_amd import api
    if no_small:
        monkeypatch.setenv("SK_DTW_NO_SMALL", "1")
    seqs, pairs, want = grid
    got = api.dtw_pairs(seqs, pairs, mode)
    check(got, want[mode], (mode, no_small))
    rng = np.random.default_rng(1)
    idx = np.concatenate([rng.permutation(len(pairs)), rng.integers(0, len(pairs), size=40)])
    again = api.dtw_pairs(seqs, [pairs[i] for i in idx], mode)
    check(again, want[mode][idx], (mode, no_small, "shuffled"))


# ---- wave-mates ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mates(ora):
    """one shape group (N = 10, L = 16): target lengths alternate between {1, 2, 3} and 1 500 .. 2 000"""
    rng = np.random.default_rng(8)
    seqs, pairs = [], []
    for p in range(33):
        M = (1, 2, 3)[(p // 2) % 3] if p % 2 == 0 else int(rng.integers(1500, 2001))
        seqs += [pairs_ref.draw(rng, 10, p % 4 < 2), pairs_ref.draw(rng, M, p % 4 < 2)]
        pairs.append((2 * p, 2 * p + 1))
    return seqs, pairs, {m: pairs_ref.records(ora, seqs, pairs, m) for m in MODES}


@pytest.mark.parametrize("mode", MODES)
def test_wave_mates_of_very_different_lengths(gpu, mates, mode):
    from squigglekit_amd import api
    seqs, pairs, want = mates
    for count in (1, 3, 4, 5, 15, 16, 17, 33):
        check(api.dtw_pairs(seqs, pairs[:count], mode), want[mode][:count], (mode, count))


# ---- mapping shape ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mapping(ora):
    queries, targets = pairs_ref.mapping_case()
    return queries, targets, pairs_ref.oracle_map(ora, queries, targets)


def test_map_queries_best_target_is_the_oracles_argmin(gpu, mapping):
    from squigglekit_amd import api
    queries, targets, want = mapping
    rec, best = api.map_queries(queries, targets)
    assert rec.shape == (2, 300)
    check(rec.reshape(-1), want.reshape(-1))
    assert np.array_equal(best, np.argmin(want["dist"], axis=0))


def test_tiled_mapping_equals_merged_oracle_pieces(gpu, ora, mapping):
    from squigglekit_amd import api
    queries, targets, _ = mapping
    pieces, tiling = api.tile_targets(targets, 1024, 512)
    assert len(pieces) == 10                                        # 3 000 points: origins 0, 512 .. 2 048, per strand
    rec, _ = api.map_queries(queries, pieces)
    want = pairs_ref.oracle_map(ora, queries, pieces)
    check(rec.reshape(-1), want.reshape(-1))
    merged = api.merge_tiles(rec, tiling)
    check(merged.reshape(-1), api.merge_tiles(want.astype(api.HIT_DTYPE), tiling).reshape(-1))


# ---- ties to the rest of the library ---------------------------------------------------------------------------------
def test_one_query_equals_dtw_subsequence_batch_byte_for_byte(gpu):
    from squigglekit_amd import api
    rng = np.random.default_rng(4)
    x = rng.normal(size=163)
    ys = [rng.normal(size=int(n)) for n in rng.integers(1, 900, size=64)]
    got = api.dtw_pairs([x] + ys, [(0, 1 + r) for r in range(64)])
    assert got.tobytes() == api.dtw_subsequence_batch(x, ys).tobytes()


def test_a_sequence_against_itself_is_zero_in_both_modes(gpu):
    from squigglekit_amd import api
    rng = np.random.default_rng(6)
    seqs = [pairs_ref.draw(rng, n, n % 2 == 0) for n in (1, 2, 17, 64, 300, 1024)]
    pairs = [(i, i) for i in range(len(seqs))]
    for mode in MODES:
        got = api.dtw_pairs(seqs, pairs, mode)
        assert np.all(got["dist"] == 0.0) and np.all(got["flags"] == 0), mode
        assert got["n"].tolist() == [len(s) for s in seqs]
        assert got["end"].tolist() == [len(s) - 1 for s in seqs] and np.all(got["start"] == 0), mode


def test_dtw_matrix(gpu, ora):
    """40 sequences of 20 .. 300 points: symmetric, zero diagonal, upper triangle equal to the reference"""
    from squigglekit_amd import api
    rng = np.random.default_rng(12)
    seqs = [pairs_ref.draw(rng, int(n), k % 2 == 0) for k, n in enumerate(rng.integers(20, 301, size=40))]
    d = api.dtw_matrix(seqs)
    assert d.shape == (40, 40) and np.array_equal(d, d.T) and np.all(np.diag(d) == 0.0)
    iu = [(i, j) for i in range(40) for j in range(i + 1, 40)]
    want = pairs_ref.records(ora, seqs, iu, "global")["dist"]
    assert np.array_equal(pairs_ref.bits(d[tuple(zip(*iu))]), pairs_ref.bits(want))
    sub = api.dtw_matrix(seqs[:6], mode="subsequence")
    for i in range(6):
        for j in range(6):
            assert pairs_ref.bits(sub[i, j]) == pairs_ref.bits(ora.dtw_subsequence(seqs[i], seqs[j])[0])


# ---- edge cases ------------------------------------------------------------------------------------------------------
def raw_call(gpu, values, off, pairs, mode, out):
    L = gpu.load()
    pr = np.zeros(len(pairs), dtype=[("query", "<i4"), ("target", "<i4")])
    if len(pairs):
        pr["query"], pr["target"] = zip(*pairs)
    rc = L.sk_dtw_pairs(gpu.ptr(values), gpu.ptr(off), off.size - 1, gpu.ptr(pr), len(pr), mode, gpu.ptr(out))
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
    for pairs, code, words in (([(0, 3), (1, 3)], gpu.SK_ERR_INVALID, ("pair 1", "empty query")),
                               ([(0, 4)], gpu.SK_ERR_INVALID, ("pair 0", "target index 4")),
                               ([(0, 3), (0, 3), (-1, 0)], gpu.SK_ERR_INVALID, ("pair 2", "query index -1")),
                               ([(3, 0), (2, 3)], gpu.SK_ERR_UNSUPPORTED, ("pair 1", "1025 points"))):
        out = np.full(len(pairs) * 24, 0xAB, dtype=np.uint8)
        rc, msg = raw_call(gpu, values, off, pairs, mode, out)
        assert rc == code and all(w in msg for w in words), (pairs, rc, msg)
        assert np.all(out == 0xAB), pairs                           # no record was written
        check(raw_records(gpu, values, off, good, mode), want, "a valid call after a refused one")
    out = np.full(24, 0xAB, dtype=np.uint8)
    assert raw_call(gpu, values, off, [], mode, out)[0] == 0 and np.all(out == 0xAB)     # npairs == 0
    rc, msg = raw_call(gpu, values, off, [(0, 3)], 2, out)
    assert rc == gpu.SK_ERR_INVALID and "mode" in msg and np.all(out == 0xAB)
    # an empty target is a record, not an error
    got = raw_records(gpu, values, off, [(0, 1), (0, 3)], mode)
    check(got, pairs_ref.records(ora, seqs, [(0, 1), (0, 3)], name))
    assert np.isnan(got["dist"][0]) and got[0].tolist()[1:] == (-1, -1, 0, 1)


def raw_records(gpu, values, off, pairs, mode):
    out = np.zeros(len(pairs), dtype=gpu.HIT_DTYPE)
    rc, msg = raw_call(gpu, values, off, pairs, mode, out)
    assert rc == 0, msg
    return out


def test_too_many_pairs_is_unsupported(gpu):
    L = gpu.load()
    one = np.zeros(1)
    off = np.array([0, 1], dtype=np.int64)
    pr = np.zeros(1, dtype=[("query", "<i4"), ("target", "<i4")])
    out = np.zeros(1, dtype=gpu.HIT_DTYPE)
    for fn in (L.sk_dtw_pairs, L.sk_dtw_pairs_dev):                  # (refused before any pointer is followed)
        assert fn(gpu.ptr(one), gpu.ptr(off), 1, gpu.ptr(pr), 2 ** 27 + 1, 0, gpu.ptr(out)) == gpu.SK_ERR_UNSUPPORTED
        assert "134217728" in L.sk_last_error().decode()


@pytest.mark.parametrize("mode", MODES)
def test_device_resident_form_equals_the_host_form(gpu, grid, mode):
    from squigglekit_amd import api
    L = gpu.load()
    seqs, pairs, want = grid
    values, off = api._as_pool(seqs)
    pad = np.concatenate([np.full(7, np.nan), values])                # the pool need not start at off = 0
    off7 = off + 7
    pr = api._as_pairs(pairs)
    host = api.dtw_pairs((pad, off7), pr, mode)
    check(host, want[mode])
    d_val, d_out = L.sk_dev_alloc(pad.nbytes), L.sk_dev_alloc(len(pr) * 24)
    try:
        gpu.check(L.sk_dev_upload(d_val, gpu.ptr(pad), pad.nbytes))
        gpu.check(L.sk_dtw_pairs_dev(d_val, gpu.ptr(off7), off7.size - 1, gpu.ptr(pr), len(pr), api.PAIRS_MODES[mode], d_out))
        gpu.check(L.sk_sync())
        dev = np.zeros(len(pr), dtype=gpu.HIT_DTYPE)
        gpu.check(L.sk_dev_download(gpu.ptr(dev), d_out, dev.nbytes))
    finally:
        L.sk_dev_free(d_val)
        L.sk_dev_free(d_out)
    assert dev.tobytes() == host.tobytes()


# ---- command line ----------------------------------------------------------------------------------------------------
def test_cli_on_synthetic_reads(gpu, ora, tmp_path):
    """squiggle_map on 24 synthetic reads (--i16, two model records, --both, a prefix that cuts the reads): stdout equals
    the composition of tests/detect_ref.py, numpy, the oracle and the same formatting; then the same tiled"""
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
    reads[22] = 7                                                   # one event: a line of dots
    reads[23, :] = np.repeat([300, 500], 750)                       # cut by the prefix to its first level: dots as well
    path = tmp_path / "reads.npy"
    np.save(path, reads)

    targets = []
    for name in ("recA", "recB"):
        z = pairs_ref.zscore(levels[name])
        targets += [(name, "+", z), (name, "-", z[::-1].copy())]

    def expected(pieces=None):
        lines = ["readID\ttarget\tstrand\tstart\tend\tevents\tdist\tdist_per_event\tsecond_target\tsecond_dist\n"]
        from squigglekit_amd import api
        for r in range(24):
            rec = detect_ref.events(reads[r, :700])
            lev = rec["sum"].astype(np.float64) / rec["length"].astype(np.float64)
            if len(lev) < 2 or not lev.std() > 0:
                lines.append("%d\t.\t.\t.\t.\t.\t.\t.\t.\t.\n" % r)
                continue
            q = (lev - lev.mean()) / lev.std()
            ys = [t[2] for t in targets]
            if pieces:
                cut, tiling = api.tile_targets(ys, *pieces)
                hits = api.merge_tiles(pairs_ref.oracle_map(ora, [q], cut).astype(api.HIT_DTYPE), tiling)[:, 0]
            else:
                hits = pairs_ref.oracle_map(ora, [q], ys)[:, 0]
            order = sorted(range(4), key=lambda t: (hits["dist"][t], t))
            b, s = order[0], order[1]
            lines.append("{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\n".format(
                r, targets[b][0], targets[b][1], int(hits["start"][b]), int(hits["end"][b]), len(q), float(hits["dist"][b]),
                float(hits["dist"][b]) / len(q), targets[s][0] + targets[s][1], float(hits["dist"][s])))
        return "".join(lines)

    argv = ["--i16", str(path), "-m", str(model), "--both", "--prefix", "700", "--batch", "10"]
    so, se, code = run_cli(main, argv)
    assert code == 0, se
    assert so == expected()
    assert se.count("fewer than 2 events") == 2 and "read 22" in se and "read 23" in se
    assert sum(ln.split("\t")[1] != "." for ln in so.split("\n")[1:-1]) == 22
    so, se, code = run_cli(main, argv + ["--piece", "64", "--overlap", "40"])
    assert code == 0 and so == expected((64, 40))
