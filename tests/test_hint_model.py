"""CPU: the start hint the tagged screening sweep carries (csrc/sk_sdtwq.hip: k_sdtw_qh), by brute force
against a Python restatement of the recurrence.  No GPU, no library.

The tagged sweep is pass Q's fixed-point recurrence with two changes: every sample and motif image is truncated to a
multiple of 2^T units, and the virtual row -1 (all zeros in k_sdtw_q) holds tag(j) = (j >> G) & (2^T - 1) in column j.
|x - y| of two multiples of 2^T is one, so neither the saturating add nor min3 touches the low T bits of a cost word: a
cell arrives with the tag of the granule (2^G columns) in which its own path left row -1.  What has to hold:
  (a) the tagged matrix is still within E' = 2^T (N + n + 2) + 2^T - 1 units of the exact one in every cell (truncation
      moves a local cost by at most 2^T - 1 units, the images' rounding by one more, the tag adds at most 2^T - 1 once),
      so the candidate rule and the lower bounds of the window pass hold with E' in E's place;
  (b) the low bits of a last-row word ARE the tag of the granule its own path (by back-trace) started in;
  (c) decoding that tag to the latest granule at or before the word's column gives a column at or before the path's
      start, and the start's own granule whenever the path is narrower than the tag range of 2^(T+G) columns."""
import numpy as np
import pytest

QSCALE = 4194304.0            # 2^22           (csrc/sk_sdtw_dev.h)
QINF = 0xFFFFFFFF
QSAFE = 0xF0000000


def qimg(t, T):
    """the kernel's image: rint, biased to unsigned, truncated to a multiple of 2^T"""
    return (int(np.rint(t)) + 0x80000000) & ~((1 << T) - 1)


def tag(j, T, G):
    return ((j >> G) & ((1 << T) - 1)) if j >= 0 else 0


def tagged_matrix(xq, yq, T, G):
    """k_sdtw_qh: nw = min(|xq - yq| + min3(diag, left, up), 2^32 - 1); row -1 holds tag(j); nothing left of column 0.
    Returns the cost words and, per cell, the predecessor the back-trace takes: (i, j) or ('row-1', column)."""
    N, n = len(xq), len(yq)
    D = [[0] * n for _ in range(N)]
    B = [[None] * n for _ in range(N)]
    for j in range(n):
        for i in range(N):
            c = abs(xq[i] - yq[j])
            if i == 0:
                prev = [(tag(j - 1, T, G), ("row-1", j - 1)), (tag(j, T, G), ("row-1", j))]
                if j > 0:
                    prev.append((D[0][j - 1], (0, j - 1)))
            elif j == 0:
                prev = [(D[i - 1][0], (i - 1, 0))]
            else:
                prev = [(D[i - 1][j - 1], (i - 1, j - 1)), (D[i][j - 1], (i, j - 1)), (D[i - 1][j], (i - 1, j))]
            best, B[i][j] = min(prev, key=lambda p: p[0])
            D[i][j] = min(c + best, QINF)
    return D, B


def exact_matrix(x, y):
    """mlpy's subsequence cost matrix in float64 (oracle/sk_oracle.c restates it)"""
    N, n = len(x), len(y)
    D = np.zeros((N, n))
    for j in range(n):
        for i in range(N):
            c = abs(x[i] - y[j])
            if i == 0:
                D[i, j] = c
            elif j == 0:
                D[i, j] = c + D[i - 1, 0]
            else:
                D[i, j] = c + min(D[i - 1, j - 1], D[i, j - 1], D[i - 1, j])
    return D


def decode(j, word, T, G):
    """the epilogue's decode: first column of the latest granule at or before column j whose tag is the word's"""
    m = (1 << T) - 1
    gj = j >> G
    return (gj - ((gj - (word & m)) & m)) << G


def cases(seed, count):
    rng = np.random.default_rng(seed)
    for case in range(count):
        N, n = int(rng.integers(1, 13)), int(rng.integers(1, 41))
        kind = case % 4
        if kind == 0:                                                     # a few units apart: truncation matters most
            s = float(rng.choice([1, 3, 37]))
            x = rng.integers(-200, 200, N) * s / QSCALE
            y = rng.integers(-200, 200, n) * s / QSCALE
        elif kind == 1:                                                   # ties: many equal costs, equal paths
            x, y = rng.integers(-3, 4, N).astype(float), rng.integers(-3, 4, n).astype(float)
        elif kind == 2:                                                   # half units: every image rounds by 1/2
            x = (rng.integers(-2000, 2000, N) + 0.5) / QSCALE
            y = (rng.integers(-2000, 2000, n) + 0.5) / QSCALE
        else:                                                             # a constant read, a constant motif
            x, y = np.full(N, float(rng.integers(-2, 3))), np.full(n, float(rng.integers(-2, 3)))
        yield case, x, y


@pytest.mark.parametrize("T,G", [(2, 1), (3, 2), (2, 0), (5, 4)])
def test_tagged_cells_stay_within_E_prime_and_carry_their_start_granule(T, G):
    worst = 0.0
    wraps = 0
    for case, x, y in cases(11 + T * 8 + G, 240):
        N, n = len(x), len(y)
        Ep = (N + n + 2) * (1 << T) + (1 << T) - 1
        xq = [qimg(v * QSCALE, T) for v in x]
        yq = [qimg(v * QSCALE, T) for v in y]
        Dq, B = tagged_matrix(xq, yq, T, G)
        D = exact_matrix(x, y)
        # (a) every cell within E' of the exact one: lower bounds and the candidate rule as before
        for i in range(N):
            for j in range(n):
                assert Dq[i][j] < QSAFE
                d = abs(Dq[i][j] - D[i, j] * QSCALE)
                assert d <= Ep, (case, N, n, i, j, Dq[i][j], D[i, j] * QSCALE)
                worst = max(worst, d / Ep)
        last = np.array(Dq[N - 1], dtype=np.int64)
        assert last[int(np.argmin(D[N - 1]))] <= last.min() + 2 * Ep, (case, "the exact argmin is not a candidate column")
        # (b), (c) per last-row word
        for j in range(n):
            cell = (N - 1, j)
            while cell[0] != "row-1":
                cell = B[cell[0]][cell[1]]
            js = cell[1]                                                  # the column of row -1 the path left from
            assert (Dq[N - 1][j] & ((1 << T) - 1)) == tag(js, T, G), (case, j, js)
            dec = decode(j, Dq[N - 1][j], T, G)
            g0 = (max(js, 0) >> G) << G                                   # first column of the start's granule
            assert dec <= j and (dec - g0) % (1 << (T + G)) == 0, (case, j, js, dec)
            if j - g0 < (1 << (T + G)):
                assert dec == g0 <= max(js, 0), (case, j, js, dec)
            else:                                                         # wider than the range: the hint is too short, and
                assert dec > g0                                           # the window pass finds out (S = -1: second tier)
                wraps += 1
    assert worst > 0.1                                                    # E' is no loose formality
    if T + G <= 3:
        assert wraps > 0                                                  # paths wider than the tag range did occur
