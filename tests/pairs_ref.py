"""The statement of DTW over a pair list (include/squigglekit_hip.h, "DTW over a pair list") in plain Python, and the
cases the pair-list tests share.  Nothing here calls the library.

Subsequence mode is the oracle's dtw_subsequence.  Global mode is the double loop below; for large cases the C oracle
serves through the sentinel identity

    global(x, y).dist == dtw_subsequence([B] + x + [-B], [B] + y + [-B]).dist          (B = 1e9 > any path cost)

whose start comes out 0 and whose end comes out M + 1: the first row matches the first column only, the last row the
last column only, and adding 0.0 changes no bit."""
import numpy as np

HIT = np.dtype([("dist", "<f8"), ("start", "<i4"), ("end", "<i4"), ("n", "<i4"), ("flags", "<i4")])
B = 1e9
FLAG_EMPTY = 1


def dtw_global(x, y):
    """D[N-1][M-1] of D[0][0] = |x0 - y0|, D[0][j] = D[0][j-1] + |x0 - yj|, D[i][0] = D[i-1][0] + |xi - y0|,
    D[i][j] = |xi - yj| + min(D[i-1][j], D[i-1][j-1], D[i][j-1]): one correctly rounded add per cell"""
    x = [float(v) for v in x]
    y = [float(v) for v in y]
    N, M = len(x), len(y)
    D = [[0.0] * M for _ in range(N)]
    for i in range(N):
        for j in range(M):
            c = abs(x[i] - y[j])
            if i == 0 and j == 0:
                D[i][j] = c
            elif i == 0:
                D[i][j] = D[i][j - 1] + c
            elif j == 0:
                D[i][j] = D[i - 1][j] + c
            else:
                D[i][j] = c + min(D[i - 1][j], D[i - 1][j - 1], D[i][j - 1])
    return D[N - 1][M - 1]


def dtw_global_sentinel(ora, x, y):
    """(dist, start, end) of the sentinel form: dist is the global distance, start 0, end M + 1"""
    xs = np.concatenate([[B], np.asarray(x, dtype=np.float64), [-B]])
    ys = np.concatenate([[B], np.asarray(y, dtype=np.float64), [-B]])
    return ora.dtw_subsequence(xs, ys)


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def draw(rng, n, ties):
    """n values: tie-heavy integers in [-3, 3], or normal draws"""
    if ties:
        return rng.integers(-3, 4, size=n).astype(np.float64)
    return rng.normal(size=n)


def records(ora, seqs, pairs, mode):
    """the records of a pair list by the references: HIT [npairs]"""
    out = np.zeros(len(pairs), dtype=HIT)
    for p, (q, t) in enumerate(pairs):
        x, y = np.asarray(seqs[q], dtype=np.float64), np.asarray(seqs[t], dtype=np.float64)
        if y.size == 0:
            out[p] = (np.nan, -1, -1, 0, FLAG_EMPTY)
        elif mode == "global":
            d, s, e = dtw_global_sentinel(ora, x, y)
            assert s == 0 and e == y.size + 1
            out[p] = (d, 0, y.size - 1, y.size, 0)
        else:
            d, s, e = ora.dtw_subsequence(x, y)
            out[p] = (d, s, e, y.size, 0)
    return out


def same_records(got, want):
    """bits of dist (two NaNs agree); start, end, n, flags equal"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return False
    gd, wd = got["dist"], want["dist"]
    ok = (bits(gd) == bits(wd)) | (np.isnan(gd) & np.isnan(wd))
    for f in ("start", "end", "n", "flags"):
        ok &= got[f] == want[f]
    return bool(ok.all())


def zscore(v):
    v = np.asarray(v, dtype=np.float64)
    return (v - v.mean()) / v.std()


# ---- the shape grid: every (L, R) group in one call ------------------------------------------------------------------
GRID_N = (1, 2, 3, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 511, 513, 1023, 1024)


def shape_grid(seed=5):
    """(seqs, pairs): each query length of GRID_N against targets of {1, max(1, N - 1), N + 1, 200, 777} points; every
    other query (and its targets) tie-heavy integers, the rest normal draws"""
    rng = np.random.default_rng(seed)
    seqs, pairs = [], []
    for k, N in enumerate(GRID_N):
        ties = k % 2 == 0
        q = len(seqs)
        seqs.append(draw(rng, N, ties))
        for M in (1, max(1, N - 1), N + 1, 200, 777):
            pairs.append((q, len(seqs)))
            seqs.append(draw(rng, M, ties))
    return seqs, pairs


# ---- the mapping shape: queries cut from a reference -----------------------------------------------------------------
def mapping_case(nq=300, M=3000, seed=17):
    """(queries, targets): targets = a z-scored reference of M points and its reversal; each query a window of 20 .. 40
    reference points (from either strand), every point repeated 1 .. 3 times, noise added, z-scored"""
    rng = np.random.default_rng(seed)
    ref = zscore(rng.normal(size=M))
    targets = [ref, np.ascontiguousarray(ref[::-1])]
    queries = []
    for _ in range(nq):
        src = targets[int(rng.integers(0, 2))]
        w = int(rng.integers(20, 41))
        a = int(rng.integers(0, M - w))
        q = np.repeat(src[a:a + w], rng.integers(1, 4, size=w))
        queries.append(zscore(q + rng.normal(scale=0.05, size=q.size)))
    return queries, targets


# ---- planted matches for the tiling helpers --------------------------------------------------------------------------
def planted_cases(count=100, M=600, seed=23):
    """(query, target) per case: a target of M normal draws and a query that is 40 .. 80 of its points, each repeated
    once or twice, with a little noise -- the whole-target match spans about the window"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        y = rng.normal(size=M)
        w = int(rng.integers(40, 81))
        a = int(rng.integers(0, M - w))
        q = np.repeat(y[a:a + w], rng.integers(1, 3, size=w))
        out.append((q + rng.normal(scale=0.02, size=q.size), y))
    return out


def oracle_map(ora, queries, targets):
    """records [T, Q] of every query in every target by the oracle"""
    out = np.zeros((len(targets), len(queries)), dtype=HIT)
    for t, y in enumerate(targets):
        out[t] = records(ora, list(queries) + [y], [(q, len(queries)) for q in range(len(queries))], "subsequence")
    return out
