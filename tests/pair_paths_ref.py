"""The statement of the warping paths over a pair list (include/squigglekit_hip.h, "Warping paths of a pair list") in plain
Python, and the cases the pair-path tests share.  Nothing here calls the library.

Spans: int32 [N][2], query point i covers the target points [a_i, b_i].

Subsequence mode is the oracle's dtw_subsequence_path (mlpy's subsequence_path).  Global mode is the full matrix of
pairs_ref.dtw_global, kept, and mlpy's path() written out below; for large cases the C oracle serves through the sentinel
form of pairs_ref: the path of [B] + x + [-B] in [B] + y + [-B] is (0, 0), then the global path shifted by one in both
coordinates, then (N + 1, M + 1) -- tests/test_pair_paths_host.py holds that identity to the plain statement."""
import numpy as np

import pairs_ref


def spans_of(px, py, N):
    """(a_i, b_i) per query point of a path"""
    sp = np.full((N, 2), -1, dtype=np.int32)
    for i, j in zip(px, py):
        if sp[i, 0] < 0:
            sp[i, 0] = j
        sp[i, 1] = j
    return sp


def global_matrix(x, y):
    """D of pairs_ref.dtw_global, every cell kept (lists of Python floats)"""
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
    return D


def global_path_plain(x, y):
    """mlpy's path() from (N-1, M-1): while i > 0 or j > 0 -- at i == 0 left, at j == 0 up, else diagonal if it equals
    min3(up, diag, left), else left if it does, else up.  Returns (dist, px, py), ascending."""
    D = global_matrix(x, y)
    i, j = len(D) - 1, len(D[0]) - 1
    px, py = [i], [j]
    while i > 0 or j > 0:
        if i == 0:
            j -= 1
        elif j == 0:
            i -= 1
        else:
            up, dg, lf = D[i - 1][j], D[i - 1][j - 1], D[i][j - 1]
            mc = min(up, dg, lf)
            if dg == mc:
                i, j = i - 1, j - 1
            elif lf == mc:
                j -= 1
            else:
                i -= 1
        px.append(i)
        py.append(j)
    return D[-1][-1], np.array(px[::-1]), np.array(py[::-1])


def global_path_sentinel(ora, x, y):
    """(px, py) of the global path by the oracle: the sentinel form's path with its first and last cell stripped and the
    indices shifted by one"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    B = pairs_ref.B
    px, py = ora.dtw_subsequence_path(np.concatenate([[B], x, [-B]]), np.concatenate([[B], y, [-B]]))
    px, py = np.asarray(px, dtype=np.int64), np.asarray(py, dtype=np.int64)
    assert (px[0], py[0]) == (0, 0) and (px[-1], py[-1]) == (x.size + 1, y.size + 1)
    px, py = px[1:-1] - 1, py[1:-1] - 1
    assert px.min() == 0 and py.min() == 0 and px.max() == x.size - 1 and py.max() == y.size - 1
    return px, py


def spans(ora, x, y, mode, plain=False):
    """the spans [N, 2] of one pair by the references; all -1 for an empty target"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if y.size == 0:
        return np.full((x.size, 2), -1, dtype=np.int32)
    if mode == "global":
        px, py = global_path_plain(x, y)[1:] if plain else global_path_sentinel(ora, x, y)
    else:
        px, py = ora.dtw_subsequence_path(x, y)
    return spans_of(px, py, x.size)


def list_spans(ora, seqs, pairs, mode):
    """(span_off int64 [npairs + 1], spans int32 [sum N, 2]) of a pair list by the references"""
    parts = [spans(ora, seqs[q], seqs[t], mode) for q, t in pairs]
    off = np.zeros(len(pairs) + 1, dtype=np.int64)
    if parts:
        off[1:] = np.cumsum([len(p) for p in parts])
    return off, (np.concatenate(parts) if parts else np.zeros((0, 2), dtype=np.int32))


def check_invariants(sp, mode, start, end):
    """a_i <= b_i, a_{i+1} is b_i or b_i + 1, and the ends of the mode"""
    sp = np.asarray(sp)
    assert np.all(sp[:, 0] <= sp[:, 1])
    step = sp[1:, 0] - sp[:-1, 1]
    assert np.all((step == 0) | (step == 1))
    assert sp[0, 0] == start and sp[-1, 1] == end
    if mode == "subsequence":
        assert sp[0, 1] == start


# ---- the shape grid of the GPU test ----------------------------------------------------------------------------------
def path_grid(seed=5):
    """(seqs, pairs, global_only): pairs_ref.shape_grid() plus N = 3 against M in {1023, 1024, 1025} (the LDS column
    limit in global mode), N = 200 against 512 and 513 points (6 400 and 6 600 direction words in global mode: either
    side of the LDS word limit) and one tie-heavy N = 3 x M = 5 000 pair (a window wider than 4 096 in global mode)"""
    seqs, pairs = pairs_ref.shape_grid(seed)
    rng = np.random.default_rng(seed + 100)

    def add(N, M, ties):
        pairs.append((len(seqs), len(seqs) + 1))
        seqs.extend([pairs_ref.draw(rng, N, ties), pairs_ref.draw(rng, M, ties)])

    for M in (1023, 1024, 1025):
        add(3, M, M % 2 == 0)
    for M in (512, 513):
        add(200, M, False)
    add(3, 5000, True)
    return seqs, pairs
