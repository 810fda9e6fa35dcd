"""MotifSeq alignment paths, host side: a numpy statement of the contract (include/squigglekit_hip.h,
sk_motifseq_paths_i16) checked against the oracle; spans <-> path; the window identity the kernel rests on; the base
table of a scrappie model; the CLI's flag checks.

The path of a hit (dist, start, end): subsequence_path's back-trace in the full N x n cost matrix from (N-1, end) --
while i > 0: at j == 0 up, else diagonal if it equals min3(up, diag, left), else left if it does, else up -- reversed.
"""
import os
import re
import subprocess

import numpy as np
import pytest
from hypothesis import given, settings, HealthCheck, strategies as st

from test_hits_host import greedy, normalised, row_starts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "squigglekit_amd", "libsquigglekit_hip.so")
HEADER = os.path.join(ROOT, "include", "squigglekit_hip.h")
MODEL = os.path.join(ROOT, "tests", "golden", "CATCTATCCAGGGTTAAATT.model")
NEW_SYMBOLS = ("sk_motifseq_paths_i16", "sk_motifseq_paths_f64", "sk_motifseq_paths_centi", "sk_motifseq_paths_dev_i16",
               "sk_dtw_subsequence_path", "sk_last_path_mismatches")


# ---- the reference -----------------------------------------------------------------------------------------------
def trace(cost, end):
    """mlpy's subsequence_path from (N-1, end) over a full cost matrix: (px, py), ascending."""
    i, j = cost.shape[0] - 1, int(end)
    px, py = [i], [j]
    while i > 0:
        if j == 0:
            i -= 1
        else:
            up, dg, lf = cost[i - 1, j], cost[i - 1, j - 1], cost[i, j - 1]
            mc = min(up, dg, lf)
            if dg == mc:
                i, j = i - 1, j - 1
            elif lf == mc:
                j -= 1
            else:
                i -= 1
        px.append(i)
        py.append(j)
    return np.array(px[::-1]), np.array(py[::-1])


def spans_of(px, py, N):
    """(a_i, b_i) per motif point of a path."""
    sp = np.full((N, 2), -1, dtype=np.int32)
    for i, j in zip(px, py):
        if sp[i, 0] < 0:
            sp[i, 0] = j
        sp[i, 1] = j
    return sp


def full_cost(ora, x, y):
    return ora.dtw_subsequence(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), want_cost=True)[3]


def reference_paths(ora, reads, motif, K, max_dist=np.inf, scale="medmad", lo=0, hi=1200):
    """Per read: None (nothing survives the filter, or MAD = 0), else the list of ((dist, start, end), spans[N, 2]) of
    its hit list in rank order."""
    out = []
    for raw in reads:
        y = normalised(ora, raw, scale, lo, hi)
        if not y.size or not np.all(np.isfinite(y)):
            out.append(None)
            continue
        cost = full_cost(ora, motif, y)
        hits = greedy(cost[-1].copy(), row_starts(cost), K, max_dist)
        out.append([(h, spans_of(*trace(cost, h[2]), len(motif))) for h in hits])
    return out


def window_dtw(x, y):
    """Subsequence DTW restricted to the columns of y (a window): the cost matrix, cell by cell as mlpy fills it."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    N, W = x.size, y.size
    D = np.empty((N, W))
    D[0] = np.abs(x[0] - y)
    for i in range(1, N):
        D[i, 0] = np.abs(x[i] - y[0]) + D[i - 1, 0]
        for j in range(1, W):
            D[i, j] = np.abs(x[i] - y[j]) + min(D[i - 1, j], D[i - 1, j - 1], D[i, j - 1])
    return D


def check_spans_shape(sp, start, end):
    assert sp[0, 0] == start and sp[0, 1] == start and sp[-1, 1] == end
    assert np.all(sp[:, 0] <= sp[:, 1])
    step = sp[1:, 0] - sp[:-1, 1]
    assert np.all((step == 0) | (step == 1))


# ---- the contract against the oracle -----------------------------------------------------------------------------
small = st.lists(st.integers(0, 3), min_size=1, max_size=9)


@settings(max_examples=150, deadline=None, suppress_health_check=[HealthCheck.too_slow])
@given(x=small, y=st.lists(st.integers(0, 3), min_size=1, max_size=40))
def test_trace_from_the_argmin_is_the_oracles_path(ora, x, y):
    x, y = np.array(x, float), np.array(y, float)
    d, s, e, cost = ora.dtw_subsequence(x, y, want_cost=True)
    px, py = trace(cost, e)
    opx, opy = ora.dtw_subsequence_path(x, y)
    assert np.array_equal(px, opx) and np.array_equal(py, opy)
    assert py[0] == s and py[-1] == e and px[0] == 0 and px[-1] == x.size - 1
    check_spans_shape(spans_of(px, py, x.size), s, e)


def test_trace_equals_the_oracle_on_gaussian_data(ora):
    rng = np.random.default_rng(11)
    for _ in range(40):
        x = rng.normal(size=int(rng.integers(1, 40)))
        y = rng.normal(size=int(rng.integers(1, 300)))
        _, _, e, cost = ora.dtw_subsequence(x, y, want_cost=True)
        px, py = trace(cost, e)
        opx, opy = ora.dtw_subsequence_path(x, y)
        assert np.array_equal(px, opx) and np.array_equal(py, opy)


# ---- spans <-> path -------------------------------------------------------------------------------------------------
@settings(max_examples=150, deadline=None, suppress_health_check=[HealthCheck.too_slow])
@given(x=small, y=st.lists(st.integers(0, 3), min_size=1, max_size=40), data=st.data())
def test_spans_and_expand_path_are_inverses(ora, x, y, data):
    from squigglekit_amd import api
    cost = full_cost(ora, x, y)
    end = data.draw(st.integers(0, len(y) - 1))
    px, py = trace(cost, end)
    sp = spans_of(px, py, len(x))
    gx, gy = api.expand_path(sp)
    assert np.array_equal(gx, px) and np.array_equal(gy, py)
    assert np.array_equal(api.spans_of_path(px, py, len(x)), sp)
    check_spans_shape(sp, py[0], end)


def test_expand_path_of_no_path_is_empty():
    from squigglekit_amd import api
    px, py = api.expand_path(np.full((7, 2), -1, dtype=np.int32))
    assert px.size == 0 and py.size == 0


# ---- the window identity -----------------------------------------------------------------------------------------------
def window_identity(ora, x, y, end):
    cost = full_cost(ora, x, y)
    px, py = trace(cost, end)
    start = int(py[0])
    Dw = window_dtw(x, np.asarray(y, dtype=np.float64)[start:end + 1])
    wx, wy = trace(Dw, end - start)
    assert np.array_equal(wx, px) and np.array_equal(wy + start, py), (x, y, end)
    assert np.float64(Dw[-1, -1]).tobytes() == np.float64(cost[-1, end]).tobytes(), (x, y, end)
    assert wy[0] == 0


@settings(max_examples=200, deadline=None, suppress_health_check=[HealthCheck.too_slow])
@given(x=small, y=st.lists(st.integers(0, 3), min_size=1, max_size=40), data=st.data())
def test_window_identity_on_tie_heavy_integers(ora, x, y, data):
    window_identity(ora, x, y, data.draw(st.integers(0, len(y) - 1)))


def test_window_identity_on_gaussian_constant_and_edge_shapes(ora):
    rng = np.random.default_rng(3)
    for _ in range(60):
        x = rng.normal(size=int(rng.integers(1, 30)))
        y = rng.normal(size=int(rng.integers(1, 120)))
        window_identity(ora, x, y, int(rng.integers(0, y.size)))
    window_identity(ora, [1.0], [2.0], 0)                                # N = 1, n = 1
    window_identity(ora, [1.0], [3.0, 1.0, 2.0], 1)                      # N = 1
    window_identity(ora, [1.0, 2.0, 3.0], [2.0], 0)                      # n = 1: the column-0 rule all the way
    window_identity(ora, [1.0, 2.0, 3.0], [1.0, 5.0, 5.0, 5.0], 0)       # an end at column 0
    window_identity(ora, [1.0, 2.0], [1.0, 2.0, 9.0, 9.0], 1)            # start = 0
    for n in (1, 5, 33):                                                 # constant inputs: every comparison a tie
        for N in (1, 4, 9):
            for end in {0, n // 2, n - 1}:
                window_identity(ora, np.full(N, 2.0), np.full(n, 2.0), end)


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    head = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, head), name
    syms = subprocess.run(["nm", "-D", "--defined-only", SO], capture_output=True, text=True, check=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    from squigglekit_amd import _lib
    L = _lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(L, name).argtypes is not None


def test_api_rejects_bad_arguments():
    from squigglekit_amd import api
    for K in (0, 65):
        with pytest.raises(ValueError):
            api.motifseq_paths([np.arange(10)], [np.zeros(3)], max_hits=K)
    with pytest.raises(ValueError):
        api.motifseq_paths([np.arange(10)], [np.zeros(3)], max_dist=float("nan"))


@pytest.mark.parametrize("width", [1, 2])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("n", [1, 5])
def test_flat_buffer_unpacks_as_the_header_lays_it_out(width, K, n):
    """include/squigglekit_hip.h: motif k's block of spans begins at 2 * max_hits * nreads * motif_off[k] int32, inside it
    [read][hit][N_k][2]; events follow that layout with one record where the spans have two ints.  A buffer that holds
    its own indices: every element of every per-motif array must be the index the header gives it."""
    from squigglekit_amd import api
    sizes = (1, 4, 2)
    moff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    buf = np.arange(width * K * n * int(moff[-1]), dtype=np.int32)
    got = api._unpack_blocks(buf, moff, K, n, width)
    assert len(got) == len(sizes)
    seen = 0
    for k, N in enumerate(sizes):
        assert got[k].shape == ((n, K, N, 2) if width == 2 else (n, K, N))
        for r in range(n):
            for h in range(K):
                for i in range(N):
                    for w in range(width):
                        want = width * K * n * int(moff[k]) + ((r * K + h) * N + i) * width + w
                        assert (got[k][r, h, i, w] if width == 2 else got[k][r, h, i]) == want, (k, r, h, i, w)
                        seen += 1
    assert seen == buf.size                                              # (every element of the buffer has a place)


# ---- the base table of a scrappie model ----------------------------------------------------------------------------------
def test_base_table_of_the_shipped_model():
    from squigglekit_amd import tsvio
    models, order, lens, bases = tsvio.read_scrappie_model_bases(MODEL)
    m0, o0, l0 = tsvio.read_scrappie_model(MODEL)
    assert (models, order, lens) == (m0, o0, l0) and len(order) == 1
    name = order[0]
    vec, table = np.array(models[name]), bases[name]
    assert len(table) == 20 and vec.size == 163
    assert "".join(b[1] for b in table) == "CATCTATCCAGGGTTAAATT"
    assert [b[0] for b in table] == list(range(20))
    at, cat = 0, []
    for pos, base, current, first, count in table:
        assert first == at
        cat += [current] * count
        at += count
    assert at == 163 and cat == list(models[name])                     # the concatenation is the model's vector


def test_base_table_keeps_a_base_without_points(tmp_path):
    from squigglekit_amd import tsvio
    p = tmp_path / "m.model"
    p.write_text("#m\npos\tbase\tcurrent\tsd\tdwell\n0\tA\t1.5\t0.1\t2.2\n1\tC\t-0.5\t0.1\t0.3\n2\tG\t0.25\t0.1\t1.0\n"
                 "#k\npos\tbase\tcurrent\tsd\tdwell\n0\tT\t2.0\t0.1\t1.0\n")
    models, order, lens, bases = tsvio.read_scrappie_model_bases(str(p))
    assert order == ["m", "k"] and models["m"] == [1.5, 1.5, 0.25]
    assert bases["m"] == [(0, "A", 1.5, 0, 2), (1, "C", -0.5, 2, 0), (2, "G", 0.25, 2, 1)]
    assert bases["k"] == [(0, "T", 2.0, 0, 1)]


# ---- CLI flags -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [["--paths"], ["--paths", "p.tsv", "--after_stall"],
                                  ["--paths", "p.tsv", "--hits", "3", "--after_stall"]])
def test_cli_rejects_bad_path_flags(argv, tmp_path, capsys):
    from squigglekit_amd import motifseq_cli
    sig = tmp_path / "s.tsv"
    sig.write_text("f.fast5\tid0\t1\t2\t3\n")
    model = tmp_path / "m.model"
    model.write_text("pos\tbase\tcurrent\tsd\tdwell\n0\tA\t1.0\t0.1\t8\n")
    argv = [str(tmp_path / a) if a == "p.tsv" else a for a in argv]
    with pytest.raises(SystemExit) as e:
        motifseq_cli.main(["-s", str(sig), "-m", str(model)] + argv)
    assert e.value.code != 0
    out = capsys.readouterr()
    assert "readID\t" not in out.out                                    # rejected before the header is printed
    assert "paths" in out.err
    assert not (tmp_path / "p.tsv").exists()                            # ... and before the file is made
