"""The statement of the hit lists over a pair list (include/squigglekit_hip.h, "Hit lists over a pair list") in plain
Python, and the helpers its tests share.  Nothing here calls the library.

For a query x and a target y: d_j = D[N-1][j] of the oracle's dtw_subsequence(x, y) (its cost matrix), s_j = the column
where the back-trace from (N-1, j) ends -- walked cell by cell, diagonal first, then left, then up -- and K greedy rounds:
the smallest admissible d_j, ties to the smallest j; admissible = d_j <= max_dist and [s_j, j] disjoint from every interval
taken before.  For a session the last row is mapstream_ref.chained_rows' over the slot's chunks."""
import numpy as np

import mapstream_ref

HIT = np.dtype([("dist", "<f8"), ("start", "<i4"), ("end", "<i4"), ("n", "<i4"), ("flags", "<i4")])
FLAG_EMPTY = 1
INF = float("inf")


def starts_of(cost):
    """s_j of every column of the last row: the back-trace start of each cell, row by row (a cell takes the start of
    the neighbour its back-trace steps to: diagonal if that value is the minimum, else left, else up)"""
    N, M = cost.shape
    S = list(range(M))
    for i in range(1, N):
        nS = [0] * M
        for j in range(M):
            dg = cost[i - 1, j - 1] if j else INF
            lf = cost[i, j - 1] if j else INF
            up = cost[i - 1, j]
            m = min(dg, lf, up)
            nS[j] = S[j - 1] if dg == m else nS[j - 1] if lf == m else S[j]
        S = nS
    return S


def last_row(ora, x, y):
    """(d, s) of the last row of dtw_subsequence(x, y), as lists"""
    _, _, _, cost = ora.dtw_subsequence(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), want_cost=True)
    return [float(v) for v in cost[-1]], starts_of(cost)


def greedy(d, s, K, max_dist=INF):
    """[(dist, start, end)] in rank order, and whether some round was decided by a tie on dist"""
    taken, tie = [], False
    open_ = [j for j in range(len(d)) if d[j] <= max_dist]       # the columns still admissible, in increasing j
    for _ in range(K):
        best, ties = None, 0
        for j in open_:
            if best is None or d[j] < d[best]:
                best, ties = j, 0
            elif d[j] == d[best]:
                ties += 1
        if best is None:
            break
        tie |= ties > 0
        a, e = int(s[best]), best
        taken.append((d[best], a, e))
        open_ = [j for j in open_ if j < a or s[j] > e]         # disjoint from [s_j, j] of the hit just taken
    return taken, tie


def as_records(lists, K, n, flags=0):
    """hits HIT [len(lists), K] and count of lists of (dist, start, end); n / flags: one value or one per list"""
    out = np.zeros((len(lists), K), dtype=HIT)
    out["dist"], out["start"], out["end"] = np.nan, -1, -1
    out["n"] = np.asarray(n).reshape(-1, 1)
    out["flags"] = np.asarray(flags).reshape(-1, 1)
    count = np.zeros(len(lists), dtype=np.int32)
    for p, hits in enumerate(lists):
        count[p] = len(hits)
        for k, (d, a, e) in enumerate(hits):
            out[p, k]["dist"], out[p, k]["start"], out[p, k]["end"] = d, a, e
    return out, count


_ROWS = {}


def pair_rows(ora, x, y):
    """last_row, remembered per (x, y): the tests ask for several K and max_dist of the same pair"""
    key = (np.asarray(x, dtype=np.float64).tobytes(), np.asarray(y, dtype=np.float64).tobytes())
    if key not in _ROWS:
        _ROWS[key] = last_row(ora, x, y)
    return _ROWS[key]


def pair_hits(ora, seqs, pairs, K, max_dist=INF):
    """(hits HIT [npairs, K], count int32 [npairs], tie) of a pair list by the statement"""
    lists, ns, fl, tie = [], [], [], False
    for q, t in pairs:
        y = np.asarray(seqs[t], dtype=np.float64)
        ns.append(y.size)
        fl.append(FLAG_EMPTY if y.size == 0 else 0)
        if y.size == 0:
            lists.append([])
            continue
        d, s = pair_rows(ora, seqs[q], y)
        hits, tied = greedy(d, s, K, max_dist)
        tie |= tied
        lists.append(hits)
    out, count = as_records(lists, K, ns, fl)
    return out, count, tie


def session_hits(chunks_of, targets, K, max_dist=INF):
    """(hits HIT [T, m, K], count [T, m]) of slots that have been given the chunk lists chunks_of[i] (an empty list: no
    points), by chained_rows over every cut and the greedy rule"""
    T, m = len(targets), len(chunks_of)
    out = np.zeros((T, m, K), dtype=HIT)
    count = np.zeros((T, m), dtype=np.int32)
    for t, y in enumerate(targets):
        lists = []
        for chunks in chunks_of:
            state = None
            for ch in chunks:
                if len(ch):
                    state = mapstream_ref.chained_rows(ch, y, state)
            lists.append([] if state is None else greedy(state[0], state[1], K, max_dist)[0])
        out[t], count[t] = as_records(lists, K, len(y))
    return out, count


def same(got, want):
    """None, or a text naming the first record that differs (bits of dist; two NaNs agree)"""
    return mapstream_ref.first_difference(got, want)


# ---- the host helpers restated ---------------------------------------------------------------------------------------
def merge_tile_hits(hits, count, tiling, K):
    """per (target, query): the pieces' hits pooled in whole-target coordinates, ordered by (dist, end, start), taken
    greedily while disjoint"""
    tgt, org, length = tiling["target"], tiling["origin"], tiling["length"]
    T, Q = len(length), hits.shape[1]
    out = np.zeros((T, Q, K), dtype=HIT)
    cnt = np.zeros((T, Q), dtype=np.int32)
    for t in range(T):
        pieces = [p for p in range(len(tgt)) if tgt[p] == t]
        for q in range(Q):
            pool = []
            for p in pieces:
                for k in range(count[p, q]):
                    h = hits[p, q, k]
                    pool.append((float(h["dist"]), int(h["end"]) + int(org[p]), int(h["start"]) + int(org[p]), int(h["flags"])))
            pool.sort(key=lambda c: c[:3])
            taken = []
            for d, e, s, fl in pool:
                if len(taken) < K and all(e < a0 or s > e0 for a0, e0, _, _ in taken):
                    taken.append((s, e, d, fl))
            for k in range(K):
                if k < len(taken):
                    out[t, q, k] = (taken[k][2], taken[k][0], taken[k][1], length[t], taken[k][3])
                else:
                    out[t, q, k] = (np.nan, -1, -1, length[t], hits[pieces[0], q, 0]["flags"])
            cnt[t, q] = len(taken)
    return out, cnt


def locus_margin(hits, count):
    """(best_target, (dist, start, end) or None, second_dist) per query, over all listed loci of all targets"""
    T, Q = count.shape
    out = []
    for q in range(Q):
        loci = [(float(hits[t, q, k]["dist"]), t, int(hits[t, q, k]["end"]), k) for t in range(T) for k in range(count[t, q])]
        if not loci:
            out.append((-1, None, INF))
            continue
        loci.sort()
        d, t, e, k = loci[0]
        out.append((t, (d, int(hits[t, q, k]["start"]), e), loci[1][0] if len(loci) > 1 else INF))
    return out


def decide_loci(hits, count, rows, min_rows, max_dist_per_row, min_margin, give_up_rows):
    """(best, decision) per query: 1 accept, -1 give up, 0 wait -- map_decide's rule with the margin to the next locus"""
    best, dec = [], []
    for q, (t, rec, second) in enumerate(locus_margin(hits, count)):
        best.append(t)
        if t < 0:
            dec.append(0)
            continue
        r = float(rows[q])
        ok = r >= min_rows and rec[0] / r <= max_dist_per_row and (second == INF or (second - rec[0]) / r >= min_margin)
        dec.append(1 if ok else -1 if r >= give_up_rows else 0)
    return best, dec


# ---- drawn cases: the seeded random tests and tools/fuzz_gpu.py --------------------------------------------------------
LONG_M = (4097, 5000, 8191, 9000)


def draw_pairs_case(rng):
    """a drawn pair list as plain data: seqs, pairs, K, max_dist (inf, or a value from inside a pair's last row, or one
    below every row), and the row budget (None, or bytes that cut the list into slices)"""
    ties = rng.random() < 0.5
    nq, nt = int(rng.integers(1, 5)), int(rng.integers(1, 5))
    seqs = []
    for _ in range(nq):
        n = int(rng.choice([1, 2, 7, 16, 17, 30, 64, 65]))
        seqs.append(rng.integers(-3, 4, size=n).astype(np.float64) if ties else rng.normal(size=n))
    for k in range(nt):
        M = int(rng.choice(LONG_M)) if rng.random() < 0.2 else int(rng.choice([0, 1, 63, 64, 65, 300, 777, 1500]))
        seqs.append(rng.integers(-3, 4, size=M).astype(np.float64) if ties else rng.normal(size=M))
    pairs = [(int(rng.integers(0, nq)), nq + int(rng.integers(0, nt))) for _ in range(int(rng.integers(1, 9)))]
    K = int(rng.choice([1, 2, 3, 8, 64]))
    cut = ("inf", "inside", "below")[int(rng.choice([0, 0, 1, 1, 2]))]
    cols = sum(len(seqs[t]) for _, t in pairs)
    budget = None if rng.random() < 0.4 else max(12, 12 * cols // int(rng.integers(2, 5)))
    return {"seqs": seqs, "pairs": pairs, "K": K, "cut": cut, "budget": budget, "frac": float(rng.random())}


def max_dist_of(ora, case):
    """the case's max_dist: +inf; a value between the smallest and the largest d_j of its first non-empty pair; or -1"""
    if case["cut"] == "inf":
        return INF
    if case["cut"] == "below":
        return -1.0
    for q, t in case["pairs"]:
        if len(case["seqs"][t]):
            d, _ = pair_rows(ora, case["seqs"][q], case["seqs"][t])
            lo, hi = min(d), max(d)
            return lo + (hi - lo) * 0.25 * case["frac"]
    return 0.0


def draw_session_case(rng):
    """a drawn session: targets (one may pass 4 096 columns), slots, per slot a list of chunks, K and the cut"""
    ties = rng.random() < 0.5
    T = int(rng.integers(1, 4))
    targets = []
    for _ in range(T):
        M = int(rng.choice(LONG_M[:2])) if rng.random() < 0.2 else int(rng.choice([1, 2, 64, 65, 200, 513]))
        targets.append(rng.integers(-3, 4, size=M).astype(np.float64) if ties else rng.normal(size=M))
    nslots = int(rng.integers(1, 5))
    pushes = []
    for _ in range(int(rng.integers(1, 4))):
        pushes.append([rng.integers(-3, 4, size=n).astype(np.float64) if ties else rng.normal(size=n)
                       for n in (int(rng.choice([0, 1, 5, 16, 17, 40])) for _ in range(nslots))])
    return {"targets": targets, "nslots": nslots, "pushes": pushes, "K": int(rng.choice([1, 2, 8])),
            "max_dist": INF if rng.random() < 0.6 else float(rng.uniform(0.0, 12.0))}


def run_pairs_case(api, ora, case, env):
    """the drawn pair list through api.dtw_pairs_hits (env: where its row budget is set) against the statement.  None, or
    a text naming the first record that differs"""
    md = max_dist_of(ora, case)
    want_h, want_c, _ = pair_hits(ora, case["seqs"], case["pairs"], case["K"], md)
    if case["budget"] is not None:
        env["SK_HITS_ROW_BYTES"] = str(case["budget"])
    try:
        hits, count = api.dtw_pairs_hits(case["seqs"], case["pairs"], case["K"], md)
    finally:
        env.pop("SK_HITS_ROW_BYTES", None)
    what = "K %d, max_dist %r, budget %r, pairs %s, lengths %s" % (
        case["K"], md, case["budget"], case["pairs"], [len(s) for s in case["seqs"]])
    if same(hits, want_h) is not None:
        return "%s (%s)" % (same(hits, want_h), what)
    return None if np.array_equal(count, want_c) else "counts %s, want %s (%s)" % (count, want_c, what)


def run_session_case(api, sess):
    """the drawn session script through api.MapStream: hits() after every push against the statement on what the slots
    have been given.  None, or a text naming the push and the first record that differs"""
    every = list(range(sess["nslots"]))
    given = [[] for _ in every]
    with api.MapStream(sess["targets"], sess["nslots"]) as ms:
        for k, chunks in enumerate(sess["pushes"]):
            ms.push(every, chunks)
            for i, ch in enumerate(chunks):
                given[i].append(ch)
            hits, count = ms.hits(every, sess["K"], sess["max_dist"])
            want_h, want_c = session_hits(given, sess["targets"], sess["K"], sess["max_dist"])
            what = "push %d: K %d, max_dist %r, targets %s, chunks %s" % (
                k, sess["K"], sess["max_dist"], [len(t) for t in sess["targets"]], [[len(c) for c in g] for g in given])
            if same(hits, want_h) is not None:
                return "%s (%s)" % (same(hits, want_h), what)
            if not np.array_equal(count, want_c):
                return "counts %s, want %s (%s)" % (count, want_c, what)
    return None
