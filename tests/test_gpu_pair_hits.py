"""GPU: hit lists over a pair list (sk_dtw_pairs_hits*) and from a mapping session's stored rows (sk_map_hits*) against the
statement in tests/pair_hits_ref.py.  Records are compared by the bits of dist plus every other field."""
import ctypes as C

import numpy as np
import pytest

import mapstream_ref
import pair_hits_ref as ref

pytestmark = pytest.mark.gpu

INF = float("inf")
TARGET_M = (1, 63, 64, 65, 4095, 4096, 4097, 8191, 16385, 70001)      # the cache limit, the stripe edges, 2^16
QUERY_N = (1, 16, 17, 64, 65, 257, 1024)                              # one per (L, R) family, against M = 777


def draw(rng, n, ties):
    return rng.integers(-3, 4, size=n).astype(np.float64) if ties else rng.normal(size=n)


def check_lists(ora, api, seqs, pairs, K, max_dist=INF):
    hits, count = api.dtw_pairs_hits(seqs, pairs, K, max_dist)
    want_h, want_c, _ = ref.pair_hits(ora, seqs, pairs, K, max_dist)
    assert ref.same(hits, want_h) is None, ref.same(hits, want_h)
    assert np.array_equal(count, want_c)
    return hits, count


@pytest.mark.parametrize("ties", [True, False])
@pytest.mark.parametrize("M", TARGET_M)
def test_target_lengths(gpu, ora, M, ties):
    from squigglekit_amd import api
    rng = np.random.default_rng([M, ties])
    N = 8 if M > 20000 else int(rng.integers(8, 41))
    seqs = [draw(rng, N, ties), draw(rng, M, ties)]
    for K in (1, 2, 8, 64) if M < 20000 else (1, 8):
        hits, count = check_lists(ora, api, seqs, [(0, 1)], K)
        assert hits[:, 0].tobytes() == api.dtw_pairs(seqs, [(0, 1)]).tobytes()
    assert api.last_pair_hits_plan()["long_rows"] == (1 if M > 4096 else 0)


@pytest.mark.parametrize("ties", [True, False])
def test_query_lengths_and_one_query_shared_by_many_pairs(gpu, ora, ties):
    from squigglekit_amd import api
    rng = np.random.default_rng([5, ties])
    seqs = [draw(rng, N, ties) for N in QUERY_N] + [draw(rng, 777, ties), draw(rng, 300, ties), np.zeros(0), draw(rng, 5000, ties)]
    nq = len(QUERY_N)
    pairs = [(q, nq) for q in range(nq)] + [(1, nq + 1), (1, nq + 2), (1, nq + 3), (1, nq), (2, nq + 2), (1, nq + 1)]
    for K in (1, 2, 8, 64):
        hits, count = check_lists(ora, api, seqs, pairs, K)
        assert hits[:, 0].tobytes() == api.dtw_pairs(seqs, pairs).tobytes()
    # the empty target: count 0, n 0 and SK_FLAG_EMPTY in every slot
    e = pairs.index((1, nq + 2))
    assert count[e] == 0 and (hits["n"][e] == 0).all() and (hits["flags"][e] == gpu.SK_FLAG_EMPTY).all()


def test_finite_max_dist(gpu, ora):
    from squigglekit_amd import api
    rng = np.random.default_rng(77)
    seqs = [draw(rng, 20, True), draw(rng, 30, False), draw(rng, 900, True), draw(rng, 6000, False)]
    pairs = [(0, 2), (1, 3), (1, 2)]
    K = 8
    cuts = []
    for q, t in pairs:
        d, s = ref.pair_rows(ora, seqs[q], seqs[t])
        full, _ = ref.greedy(d, s, K)
        cuts.append(full[2][0])                                    # admits three ranks at least, of the eight
    md = cuts[1]                                                   # normal draws: three columns of that row and no more
    hits, count = check_lists(ora, api, seqs, pairs, K, md)
    assert count[1] == 3, count
    hits, count = check_lists(ora, api, seqs, pairs, K, -1.0)      # below every d_j
    assert (count == 0).all() and np.isnan(hits["dist"]).all() and (hits["n"][:, 0] == [900, 6000, 900]).all()
    hits, count = check_lists(ora, api, seqs, pairs, K, 0.0)


def test_a_query_planted_four_times_comes_back_at_the_planted_loci(gpu, ora):
    from squigglekit_amd import api
    rng = np.random.default_rng(12)
    q = rng.normal(size=50)
    for M in (3000, 9000):
        y = rng.normal(size=M) * 0.3 + 4.0
        at = [200, 900, M - 1300, M - 80]
        for a in at:
            y[a:a + 50] = q
        hits, count = check_lists(ora, api, [q, y], [(0, 1)], 6)
        got = sorted((int(h["start"]), int(h["end"])) for h in hits[0, :4])
        assert got == [(a, a + 49) for a in at] and (hits["dist"][0, :4] == 0.0).all() and count[0] == 6
        assert hits["end"][0, :4].tolist() == sorted(hits["end"][0, :4].tolist())     # equal dists: the smallest j first


def test_row_budget_slices_keep_the_lists(gpu, ora, monkeypatch):
    from squigglekit_amd import api
    rng = np.random.default_rng(3)
    seqs = [draw(rng, 12, True), draw(rng, 33, False)] + [draw(rng, M, k % 2 == 0) for k, M in enumerate((500, 64, 4500, 1, 700, 300, 0, 65))]
    pairs = [(k % 2, 2 + k) for k in range(8)] + [(0, 4), (1, 2)]
    base_h, base_c = check_lists(ora, api, seqs, pairs, 4)
    assert api.last_pair_hits_plan()["slices"] == 1
    lens = [len(seqs[t]) for _, t in pairs]

    def slices_of(budget):
        """consecutive pairs while their columns fit budget // 12, at least one pair a slice"""
        n, cols = 0, None
        for M in lens:
            if cols is None or cols + M > budget // 12:
                n, cols = n + 1, M
            else:
                cols += M
        return n

    seen = []
    for budget in (12 * sum(lens) // 3, 12 * 4500, 12 * 100, 1):    # thirds; one long row; below a single row, twice
        monkeypatch.setenv("SK_HITS_ROW_BYTES", str(budget))
        hits, count = api.dtw_pairs_hits(seqs, pairs, 4)
        plan = api.last_pair_hits_plan()
        assert hits.tobytes() == base_h.tobytes() and count.tobytes() == base_c.tobytes(), budget
        assert plan["long_rows"] == 2 and plan["slices"] == slices_of(budget), (budget, plan)
        seen.append(plan["slices"])
    assert seen[0] >= 3 and seen[2] >= len(pairs) - 1 and seen[3] == len(pairs), seen      # (an empty target adds no columns)


def test_paths_of_the_first_three_ranks(gpu, ora):
    from squigglekit_amd import api
    rng = np.random.default_rng(8)
    seqs = [draw(rng, 25, False), draw(rng, 40, True), draw(rng, 800, False), draw(rng, 5000, True)]
    pairs = [(0, 2), (1, 3), (0, 3), (1, 2)]
    hits, count = check_lists(ora, api, seqs, pairs, 3)
    assert (count == 3).all()
    for k in range(3):
        rec, soff, spans = api.dtw_pairs_paths(seqs, pairs, records=hits[:, k])
        assert api.last_path_mismatches() == 0
        for p in range(len(pairs)):
            sp = spans[soff[p]:soff[p + 1]]
            assert sp[0, 0] == hits["start"][p, k] and sp[-1, 1] == hits["end"][p, k], (p, k)
            assert (sp[:, 0] <= sp[:, 1]).all() and (sp[1:, 0] >= sp[:-1, 1]).all()


def upload(L, a):
    p = C.c_void_p(L.sk_dev_alloc(max(a.nbytes, 8)))
    assert p.value, L.sk_last_error()
    if a.nbytes:
        assert L.sk_dev_upload(p, a.ctypes.data_as(C.c_void_p), a.nbytes) == 0, L.sk_last_error()
    return p


def download(L, p, like):
    out = np.empty_like(like)
    assert L.sk_dev_download(out.ctypes.data_as(C.c_void_p), p, out.nbytes) == 0, L.sk_last_error()
    return out


def test_the_device_forms_equal_the_host_forms(gpu, ora):
    from squigglekit_amd import api
    L = gpu.load()
    rng = np.random.default_rng(21)
    seqs = [draw(rng, 30, True), draw(rng, 1000, True), draw(rng, 4200, False)]
    pairs = [(0, 1), (0, 2)]
    K = 5
    hits, count = check_lists(ora, api, seqs, pairs, K, 30.0)
    values, off = api._as_pool(seqs)
    pr = api._as_pairs(pairs)
    d_val, d_out, d_cnt = upload(L, values), upload(L, np.zeros_like(hits)), upload(L, np.zeros_like(count))
    assert L.sk_dtw_pairs_hits_dev(d_val, gpu.ptr(off), 3, gpu.ptr(pr), 2, K, 30.0, d_out, d_cnt) == 0, L.sk_last_error()
    assert L.sk_sync() == 0
    assert download(L, d_out, hits).tobytes() == hits.tobytes() and download(L, d_cnt, count).tobytes() == count.tobytes()
    with api.MapStream(seqs[1:], 3) as ms:
        ms.push([2, 0], [seqs[0], seqs[0][:7]])
        h_hits, h_count = ms.hits([0, 1, 2], K, 30.0)
        slots = np.array([0, 1, 2], dtype=np.int32)
        d_slots, d_o, d_c = upload(L, slots), upload(L, np.zeros_like(h_hits)), upload(L, np.zeros_like(h_count))
        assert L.sk_map_hits_dev(ms.handle, d_slots, 3, K, 30.0, d_o, d_c) == 0, L.sk_last_error()
        assert L.sk_sync() == 0
        assert download(L, d_o, h_hits).tobytes() == h_hits.tobytes() and download(L, d_c, h_count).tobytes() == h_count.tobytes()
        assert ref.same(h_hits[:, 2], hits) is None                 # slot 2 holds the whole query: the one-shot lists
        for p in (d_slots, d_o, d_c):
            L.sk_dev_free(p)
    for p in (d_val, d_out, d_cnt):
        L.sk_dev_free(p)


# ---- sessions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", ["1|N-1", "N-1|1", "thirds", "ones"])
def test_session_hits_after_every_push(gpu, ora, split):
    from squigglekit_amd import api
    rng = np.random.default_rng(31)
    targets = [draw(rng, 300, True), draw(rng, 65, False), draw(rng, 4500, True)]       # one beyond 4 096 columns
    x = [draw(rng, 12, True), draw(rng, 9, False)]
    cuts = [mapstream_ref.cut(q, mapstream_ref.splits_of(len(q))[split]) for q in x]
    K = 3
    with api.MapStream(targets, 4) as ms, api.MapStream(targets, 4) as twin:
        for step in range(max(len(c) for c in cuts)):
            live = [i for i in range(2) if step < len(cuts[i])]
            slots = [3, 1]
            rec = ms.push([slots[i] for i in live], [cuts[i][step] for i in live])
            trec = twin.push([slots[i] for i in live], [cuts[i][step] for i in live])
            assert rec.tobytes() == trec.tobytes()                   # asking changed nothing: the twin never asks
            for md in (INF, 6.0):
                hits, count = ms.hits([3, 1, 0], K, md)
                want_h, want_c = ref.session_hits([cuts[0][:step + 1], cuts[1][:step + 1], []], targets, K, md)
                assert ref.same(hits, want_h) is None, (step, md, ref.same(hits, want_h))
                assert np.array_equal(count, want_c)
            hits, count = ms.hits([s for s in (slots[i] for i in live)], 1)
            assert ref.same(hits[:, :, 0], api.map_hits(rec)) is None    # hit 1 is the push record
        plan = api.last_pair_hits_plan()
        assert plan["slices"] == 1 and plan["long_rows"] == len(live)
        ms.reset([3])
        hits, count = ms.hits([3, 0], 2)
        assert (count == 0).all() and np.isnan(hits["dist"]).all() and (hits["start"] == -1).all() and (hits["flags"] == 0).all()
        assert hits["n"][:, 0, 0].tolist() == [300, 65, 4500]


def test_session_query_beyond_1024_points(gpu, ora):
    from squigglekit_amd import api
    rng = np.random.default_rng(32)
    targets = [draw(rng, 150, True), draw(rng, 90, False)]
    x = draw(rng, 1100, True)
    chunks = [x[:700], x[700:]]
    with api.MapStream(targets, 2) as ms:
        for k in range(2):
            rec = ms.push([1], [chunks[k]])
            hits, count = ms.hits([1], 4)
            want_h, want_c = ref.session_hits([chunks[:k + 1]], targets, 4)
            assert ref.same(hits, want_h) is None and np.array_equal(count, want_c)
            assert ref.same(hits[:, :, 0], api.map_hits(rec)) is None


def test_session_refusals_leave_out_untouched(gpu):
    from squigglekit_amd import api
    L = gpu.load()
    out = np.full(4 * 2 * 24, 0xAB, dtype=np.uint8)
    cnt = np.full(16, 0xAB, dtype=np.uint8)
    with api.MapStream([np.arange(10.0)], 2) as ms:
        ms.push([0], [np.arange(3.0)])
        closed = [h for h in range(gpu.SK_MAP_MAX_SESSIONS) if h != ms.handle][0]
        for handle, slots, words in ((closed, [0], "unknown mapping session handle"), (ms.handle, [0, 2], "slot 2 is outside [0, 2)")):
            sl = np.array(slots, dtype=np.int32)
            rc = L.sk_map_hits(handle, gpu.ptr(sl), sl.size, 2, INF, gpu.ptr(out), gpu.ptr(cnt))
            assert rc == gpu.SK_ERR_INVALID and words in L.sk_last_error().decode(), L.sk_last_error()
            assert np.all(out == 0xAB) and np.all(cnt == 0xAB)
        with pytest.raises(ValueError):
            ms.hits([0], 0)
        with pytest.raises(ValueError):
            ms.hits([0], 2, float("nan"))
