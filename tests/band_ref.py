"""The statement of the adaptive-band DTW (include/squigglekit_hip.h, "Adaptive-band DTW over a pair list") in plain
numpy, one anti-diagonal per loop turn, and the cases the band tests share.  Nothing here calls the library.

Band b = 0 .. N + M - 2 has a lower-left corner (I_b, J_b), (I_0, J_0) = (h, -h), h = W / 2; offset o = 0 .. W - 1 of band
b is the cell (I_b - o, J_b + o).  A cell outside the matrix holds +inf.  Predecessors come from bands b - 1 (up, left)
and b - 2 (diag) at the offsets of those cells, +inf when the offset is outside [0, W).  Selection and direction are
k_sdtw's: m1 = left < diag ? left : diag; m = up < m1 ? up : m1; UP if up < m1, else LEFT if left < diag, else DIAG.
After band b the corner moves right when D_b[W-1] < D_b[0], down when D_b[0] < D_b[W-1], otherwise right for even b and
down for odd b.  Distances use float64 add, subtract, abs and compare only."""
import numpy as np

DIAG, LEFT, UP = 0, 1, 2
FLAG_EMPTY, FLAG_BAND_LOST = 1, 16
WIDTHS = (64, 128, 256)
ENDS = ("pinned", "free")
INF = np.inf


def _shift(prev, s):
    """prev[o + s] for o = 0 .. W - 1, +inf outside (s in -1, 0, 1)"""
    pad = np.concatenate([[INF], prev, [INF]])
    return pad[1 + s:1 + s + prev.size]


def band(x, y, W, end="pinned", trace=True):
    """One pair by the statement.  Returns a dict: dist, start, end, n, flags, spans int32 [N, 2] (all -1 without a path),
    moves (the corner move after every band but the last: 0 right, 1 down), corners int64 [steps, 2], lost (bool)."""
    assert W in WIDTHS and end in ENDS
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    N, M = x.size, y.size
    assert N >= 1
    none = np.full((N, 2), -1, dtype=np.int32)
    if M == 0:
        return dict(dist=np.nan, start=-1, end=-1, n=0, flags=FLAG_EMPTY, spans=none, moves=np.zeros(0, np.uint8),
                    corners=np.zeros((0, 2), np.int64), lost=False)
    h = W // 2
    steps = N + M - 1
    o = np.arange(W)
    I, J = h, -h
    corners = np.zeros((steps, 2), dtype=np.int64)
    moves = np.zeros(max(steps - 1, 0), dtype=np.uint8)
    dirs = np.zeros((steps, W), dtype=np.uint8)
    D1 = D2 = None                                      # bands b - 1 and b - 2
    I1 = I2 = 0
    best, best_end, best_b = INF, -1, -1
    with np.errstate(invalid="ignore"):
        for b in range(steps):
            corners[b] = (I, J)
            i, j = I - o, J + o
            live = (i >= 0) & (i < N) & (j >= 0) & (j < M)
            if b == 0:
                D = np.full(W, INF)
                D[h] = abs(x[0] - y[0])
            else:
                up = _shift(D1, I1 - I + 1)
                left = _shift(D1, I1 - I)
                diag = _shift(D2, I2 - I + 1) if b >= 2 else np.full(W, INF)
                c = np.abs(x[np.clip(i, 0, N - 1)] - y[np.clip(j, 0, M - 1)])
                lt1 = left < diag
                m1 = np.where(lt1, left, diag)
                lt2 = up < m1
                m = np.where(lt2, up, m1)
                D = np.where(live, c + m, INF)
                dirs[b] = np.where(lt2, UP, np.where(lt1, LEFT, DIAG))
            if end == "free":
                oo = I - (N - 1)
                if 0 <= oo < W and live[oo] and D[oo] < best:
                    best, best_end, best_b = D[oo], b - (N - 1), b
            if b < steps - 1:
                ll, ur = D[0], D[W - 1]
                if ur < ll:
                    down = 0
                elif ll < ur:
                    down = 1
                else:
                    down = b & 1
                moves[b] = down
                I2, D2 = I1, D1
                I1, D1 = I, D
                if down:
                    I += 1
                else:
                    J += 1
        if end == "pinned":
            oo = I - (N - 1)
            best = D[oo] if 0 <= oo < W else INF
            best_end, best_b = M - 1, steps - 1
    if not best < INF and not np.isnan(best):
        return dict(dist=INF, start=-1, end=-1, n=M, flags=FLAG_BAND_LOST, spans=none, moves=moves, corners=corners,
                    lost=True)
    out = dict(dist=float(best), start=0, end=int(best_end), n=M, flags=0, spans=none, moves=moves, corners=corners,
               lost=False)
    if trace:
        out["spans"] = _trace(dirs, corners, N, int(best_end), W)
    return out


def _trace(dirs, corners, N, end, W):
    """the stored directions from (N - 1, end) to (0, 0), as spans; all -1 if the walk leaves the band or the matrix"""
    sp = np.full((N, 2), -1, dtype=np.int32)
    i, j, hi = N - 1, end, end
    while i > 0 or j > 0:
        b = i + j
        oo = corners[b, 0] - i
        if not 0 <= oo < W:
            return np.full((N, 2), -1, dtype=np.int32)
        d = dirs[b, oo]
        if d == LEFT:
            if j == 0:
                return np.full((N, 2), -1, dtype=np.int32)
            j -= 1
            continue
        if i == 0 or (d == DIAG and j == 0):
            return np.full((N, 2), -1, dtype=np.int32)
        sp[i] = (j, hi)
        i -= 1
        if d == DIAG:
            j -= 1
        hi = j
    sp[0] = (0, hi)
    return sp


# ---- the full matrix (fact 1 and "banded >= full") --------------------------------------------------------------------
def full_matrix(x, y):
    """D[N][M] of the global DTW by a plain double loop over Python floats: D[0][0] = |x0 - y0|, the borders +inf, every
    cell by the statement's selects"""
    x = [float(v) for v in x]
    y = [float(v) for v in y]
    N, M = len(x), len(y)
    D = [[INF] * M for _ in range(N)]
    for i in range(N):
        for j in range(M):
            c = abs(x[i] - y[j])
            if i == 0 and j == 0:
                D[i][j] = c
                continue
            up = D[i - 1][j] if i > 0 else INF
            left = D[i][j - 1] if j > 0 else INF
            diag = D[i - 1][j - 1] if i > 0 and j > 0 else INF
            m1 = left if left < diag else diag
            D[i][j] = c + (up if up < m1 else m1)
    return D


def full_path_spans(D, end):
    """mlpy's path() order from (N - 1, end) over a kept matrix: at i == 0 left, at j == 0 up, else diagonal if it equals
    min3, else left if it does, else up; as spans"""
    N = len(D)
    sp = np.full((N, 2), -1, dtype=np.int32)
    i, j, hi = N - 1, end, end
    while i > 0 or j > 0:
        if i == 0:
            j -= 1
            continue
        if j == 0:
            d = UP
        else:
            up, dg, lf = D[i - 1][j], D[i - 1][j - 1], D[i][j - 1]
            mc = min(up, dg, lf)
            d = DIAG if dg == mc else (LEFT if lf == mc else UP)
        if d == LEFT:
            j -= 1
            continue
        sp[i] = (j, hi)
        i -= 1
        if d == DIAG:
            j -= 1
        hi = j
    sp[0] = (0, hi)
    return sp


def full_distance(x, y):
    """D[N-1][:] of the global DTW for long inputs: numpy over anti-diagonals, the same selects (last row only)"""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    N, M = x.size, y.size
    last = np.full(M, INF)
    P1 = P2 = None                                      # anti-diagonals b - 1, b - 2, indexed by i (length N, +inf outside)
    for b in range(N + M - 1):
        i = np.arange(N)
        j = b - i
        live = (j >= 0) & (j < M)
        if b == 0:
            D = np.full(N, INF)
            D[0] = abs(x[0] - y[0])
        else:
            up = np.concatenate([[INF], P1[:-1]])       # (i - 1, j) lies on b - 1 at index i - 1
            left = P1                                   # (i, j - 1) on b - 1 at index i
            diag = np.concatenate([[INF], P2[:-1]]) if b >= 2 else np.full(N, INF)
            c = np.abs(x - y[np.clip(j, 0, M - 1)])
            m1 = np.where(left < diag, left, diag)
            m = np.where(up < m1, up, m1)
            D = np.where(live, c + m, INF)
        if 0 <= b - (N - 1) < M:
            last[b - (N - 1)] = D[N - 1]
        P2, P1 = P1, D
    return last


# ---- records and lists -------------------------------------------------------------------------------------------------
HIT = np.dtype([("dist", "<f8"), ("start", "<i4"), ("end", "<i4"), ("n", "<i4"), ("flags", "<i4")])


def records(seqs, pairs, W, end, trace=True):
    """(records HIT [npairs], span_off int64 [npairs + 1], spans int32 [sum N, 2], lost pairs) of a list by the statement;
    a pair that occurs twice is computed once"""
    rec = np.zeros(len(pairs), dtype=HIT)
    parts, memo, lost = [], {}, 0
    for p, (q, t) in enumerate(pairs):
        if (q, t) not in memo:
            memo[(q, t)] = band(seqs[q], seqs[t], W, end, trace)
        r = memo[(q, t)]
        rec[p] = (r["dist"], r["start"], r["end"], r["n"], r["flags"])
        parts.append(r["spans"])
        lost += bool(r["lost"])
    off = np.zeros(len(pairs) + 1, dtype=np.int64)
    if parts:
        off[1:] = np.cumsum([len(s) for s in parts])
    return rec, off, (np.concatenate(parts) if parts else np.zeros((0, 2), dtype=np.int32)), lost


def mismatches(seqs, pairs, off, spans):
    """the pairs sk_last_path_mismatches() counts after a call with paths, from what `records` returned: a target of at
    least one point and spans of -1 -- the band lost the corner, or the walk left the band or the matrix.  (A path has
    a_0 = 0, so the first row tells; a pair without rows -- an empty query, which the library refuses -- is not counted.)"""
    return sum(1 for p, (q, t) in enumerate(pairs)
               if len(seqs[t]) > 0 and off[p] < off[p + 1] and spans[off[p], 0] == -1)


def check_invariants(sp, end):
    """a_i <= b_i, a_{i+1} is b_i or b_i + 1, a_0 = 0, b_{N-1} = end"""
    sp = np.asarray(sp)
    assert np.all(sp[:, 0] <= sp[:, 1])
    step = sp[1:, 0] - sp[:-1, 1]
    assert np.all((step == 0) | (step == 1))
    assert sp[0, 0] == 0 and sp[-1, 1] == end


def ties(rng, n):
    """integer-valued points in -3 .. 3: many equal costs"""
    return rng.integers(-3, 4, size=n).astype(np.float64)


def drift_pair(rng, M=400, p=0.55, noise=0.3, stall=120, extra=0):
    """(query, target): every target level repeated geometric(p) times plus N(0, noise) noise, one level repeated `stall`
    times instead (0: none); `extra` more points appended to the target (free-end cases)"""
    y = rng.normal(size=M)
    rep = rng.geometric(p, size=M)
    if stall:
        rep[int(rng.integers(M // 4, 3 * M // 4))] = stall
    x = np.repeat(y, rep) + rng.normal(scale=noise, size=int(rep.sum()))
    if extra:
        y = np.concatenate([y, rng.normal(size=extra)])
    return x, y


# the non-finite kinds the band tests lay into a pair (the header: "equal, both +inf, a NaN" move the band by parity; a
# NaN never wins a `<`, so it is never the free end; an inf in a row or a column costs +inf along it)
NONFINITE = ("nan in a query", "+inf in a query", "-inf in a query", "nan in a target", "+inf in a target",
             "-inf in a target", "nan at x[0]", "nan in the target's last point", "nan in 20 % of a target")


def lay_non_finite(rng, x, y, kind):
    """(x, y) with one kind of NONFINITE laid into a copy of the query or of the target (one of the two is returned as
    it came)"""
    query = "query" in kind or "x[0]" in kind
    v = np.array(x if query else y, dtype=np.float64)
    if v.size:
        bad = np.nan if "nan" in kind else (-np.inf if "-inf" in kind else np.inf)
        if "x[0]" in kind:
            v[0] = bad
        elif "last point" in kind:
            v[-1] = bad
        elif "20 %" in kind:
            mask = rng.random(v.size) < 0.2
            if not mask.any():                                  # (a short target: one point at least)
                mask[int(rng.integers(v.size))] = True
            v[mask] = bad
        else:
            v[int(rng.integers(v.size))] = bad
    return (v, y) if query else (x, v)
