"""MotifSeq hit lists, host side: a numpy statement of the contract (include/squigglekit_hip.h, sk_motifseq_hits_i16),
checked against the oracle; the ABI symbols; the CLI's flag checks; the exact DTW kernels' resources.

The reference: d_j = cost[-1, j] of the oracle's full cost matrix, s_j = the column where subsequence_path's back-trace
from (N-1, j) reaches row 0 (diagonal, then j-1, then i-1), then K greedy rounds: the smallest admissible d_j (ties:
the smallest j), admissible = d_j <= max_dist and [s_j, j] disjoint from every interval taken.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from hypothesis import given, settings, HealthCheck, strategies as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "squigglekit_amd", "libsquigglekit_hip.so")
HEADER = os.path.join(ROOT, "include", "squigglekit_hip.h")
NEW_SYMBOLS = ("sk_motifseq_hits_i16", "sk_motifseq_hits_f64", "sk_motifseq_hits_centi", "sk_motifseq_hits_dev_i16")


# ---- the reference -----------------------------------------------------------------------------------------------
def row_starts(cost):
    """s_j for every column of the last row, row by row: a cell's back-trace goes diagonal if that value is the
    minimum, else left if that is, else up; a run of `left` cells takes the start of the cell where it ends
    (pointer jumping with a running maximum of the non-left columns)."""
    N, n = cost.shape
    S = np.arange(n, dtype=np.int64)
    inf = np.inf
    cols = np.arange(n)
    for i in range(1, N):
        up = cost[i - 1]
        dg = np.concatenate([[inf], cost[i - 1, :-1]])
        lf = np.concatenate([[inf], cost[i, :-1]])
        m = np.minimum(np.minimum(dg, lf), up)
        take_dg = dg == m
        take_lf = ~take_dg & (lf == m)
        val = np.where(take_dg, np.concatenate([[-1], S[:-1]]), S)      # diagonal: S[i-1][j-1]; up: S[i-1][j]
        last = np.maximum.accumulate(np.where(take_lf, -1, cols))
        S = val[last]
    return S


def plain_starts(cost):
    """s_j by a back-trace per column, the way mlpy's subsequence_path walks it."""
    N, n = cost.shape
    out = np.empty(n, dtype=np.int64)
    for j0 in range(n):
        i, j = N - 1, j0
        while i > 0:
            dg = cost[i - 1, j - 1] if j > 0 else np.inf
            lf = cost[i, j - 1] if j > 0 else np.inf
            up = cost[i - 1, j]
            m = min(dg, lf, up)
            if dg == m:
                i, j = i - 1, j - 1
            elif lf == m:
                j -= 1
            else:
                i -= 1
        out[j0] = j
    return out


def last_row(ora, x, y):
    """(d, s) of the last row of mlpy.dtw_subsequence(x, y)."""
    _, _, _, cost = ora.dtw_subsequence(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64),
                                        want_cost=True)
    return cost[-1].copy(), row_starts(cost)


def greedy(d, s, K, max_dist=np.inf):
    """[(dist, start, end)] in rank order."""
    d = np.asarray(d, dtype=np.float64)
    s = np.asarray(s)
    ok = d <= max_dist
    cols = np.arange(d.size)
    hits = []
    for _ in range(K):
        cand = np.flatnonzero(ok)
        if not cand.size:
            break
        j = int(cand[np.argmin(d[cand])])              # argmin: the first of equal values = the smallest j
        hits.append((float(d[j]), int(s[j]), j))
        ok &= (cols < s[j]) | (s > j)                  # disjoint from [s_j, j]
    return hits


def normalised(ora, raw, scale="medmad", lo=0, hi=1200):
    f = ora.scale_outliers(np.asarray(raw, dtype=np.float64), lo, hi)
    if not f.size:
        return f
    return ora.medmad(f)[0] if scale == "medmad" else ora.zscale(f)[0]


def reference_hits(ora, reads, motif, K, max_dist=np.inf, scale="medmad", lo=0, hi=1200):
    """Per read the list of (dist, start, end) -- None for a read whose filter leaves nothing or whose MAD is 0."""
    out = []
    for raw in reads:
        y = normalised(ora, raw, scale, lo, hi)
        if not y.size or not np.all(np.isfinite(y)):
            out.append(None)
            continue
        d, s = last_row(ora, motif, y)
        out.append(greedy(d, s, K, max_dist))
    return out


# ---- the reference against the oracle ----------------------------------------------------------------------------
tie_signals = st.lists(st.integers(0, 3), min_size=1, max_size=40)


@settings(max_examples=150, deadline=None, suppress_health_check=[HealthCheck.too_slow])
@given(x=st.lists(st.integers(0, 3), min_size=1, max_size=9), y=tie_signals)
def test_row_starts_equal_a_backtrace_per_column(ora, x, y):
    _, _, _, cost = ora.dtw_subsequence(np.array(x, float), np.array(y, float), want_cost=True)
    assert np.array_equal(row_starts(cost), plain_starts(cost))


@settings(max_examples=150, deadline=None, suppress_health_check=[HealthCheck.too_slow])
@given(x=st.lists(st.integers(0, 3), min_size=1, max_size=9), y=tie_signals, K=st.integers(1, 8),
       cut=st.floats(0, 20))
def test_greedy_properties(ora, x, y, K, cut):
    d, s = last_row(ora, x, y)
    hits = greedy(d, s, K)
    want = ora.dtw_subsequence(np.array(x, float), np.array(y, float))
    assert hits[0] == (want[0], want[1], want[2])                       # hit 1 = mlpy's (dist, start, end)
    dists = [h[0] for h in hits]
    assert dists == sorted(dists)                                       # never decreases with rank
    for a in range(len(hits)):                                          # pairwise disjoint
        for b in range(a + 1, len(hits)):
            assert hits[a][2] < hits[b][1] or hits[b][2] < hits[a][1]
    capped = greedy(d, s, K, cut)                                       # a finite max_dist: a prefix
    assert capped == hits[:len(capped)]
    assert all(h[0] <= cut for h in capped)
    assert len(capped) == len(hits) or hits[len(capped)][0] > cut


def test_planted_copies_come_back_in_order(ora):
    rng = np.random.default_rng(7)
    motif = rng.normal(size=30)
    y = rng.normal(size=600) * 3.0
    places = [40, 170, 330, 480]
    for k, p in enumerate(places):
        y[p:p + 30] = motif + 0.01 * (k + 1)
    d, s = last_row(ora, motif, y)
    hits = greedy(d, s, 4)
    assert [(h[1], h[2]) for h in hits] == [(p, p + 29) for p in places]


# ---- ABI -------------------------------------------------------------------------------------------------------------
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
        assert getattr(L, name).argtypes


def test_api_rejects_bad_arguments():
    from squigglekit_amd import api
    for K in (0, 65):
        with pytest.raises(ValueError):
            api.motifseq_hits([np.arange(10)], [np.zeros(3)], max_hits=K)
    with pytest.raises(ValueError):
        api.motifseq_hits([np.arange(10)], [np.zeros(3)], max_dist=float("nan"))


def test_wide_outlier_limits_take_the_float64_route(monkeypatch):
    """Limits wider than the int16 histogram: integer reads go to the float64 entry point (once, no recursion), as the
    same values; the packed block form likewise."""
    from squigglekit_amd import api
    seen = []

    def fake(values, off, motifs, max_hits, max_dist, scale, scale_low, scale_hi, devices=None):
        seen.append((np.array(values), np.array(off), scale_low, scale_hi))
        R = len(off) - 1
        return [(np.zeros((R, max_hits), dtype=api.HIT_DTYPE), np.zeros(R, dtype=np.int32)) for _ in motifs]
    monkeypatch.setattr(api, "motifseq_hits_ragged_f64", fake)
    reads = [np.arange(100, dtype=np.int16), np.arange(50, 80, dtype=np.int16)]
    api.motifseq_hits(reads, [np.zeros(5)], 4, scale_low=-10000, scale_hi=30000)
    assert len(seen) == 1
    values, off, lo, hi = seen[0]
    assert values.dtype == np.float64 and off.tolist() == [0, 100, 130] and (lo, hi) == (-10000, 30000)
    assert np.array_equal(values, np.concatenate(reads).astype(np.float64))
    sig = np.zeros((2, 104), dtype=np.int16)
    sig[0, :100], sig[1, :30] = reads
    api.motifseq_hits_batch(sig, [100, 30], [np.zeros(5)], 4, scale_low=-10000, scale_hi=30000)
    assert len(seen) == 2 and np.array_equal(seen[1][0], values) and seen[1][1].tolist() == [0, 100, 130]


# ---- CLI flags ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [["--hits", "0"], ["--hits", "65"], ["--min_hit_p", "5"],
                                  ["--hits", "3", "--after_stall"]])
def test_cli_rejects_bad_hit_flags(argv, tmp_path, capsys):
    from squigglekit_amd import motifseq_cli
    sig = tmp_path / "s.tsv"
    sig.write_text("f.fast5\tid0\t1\t2\t3\n")
    model = tmp_path / "m.model"
    model.write_text("pos\tbase\tcurrent\tsd\tdwell\n0\tA\t1.0\t0.1\t8\n")
    with pytest.raises(SystemExit) as e:
        motifseq_cli.main(["-s", str(sig), "-m", str(model)] + argv)
    assert e.value.code != 0
    out = capsys.readouterr()
    assert "readID\t" not in out.out                                    # rejected before the header is printed
    assert "hits" in out.err


# ---- the exact kernels stay as they were ------------------------------------------------------------------------------
def test_existing_exact_kernels_keep_their_resources():
    """The row-writing mode is a new instantiation of k_sdtw; every existing one compiles as before (VGPR, SGPR, spills,
    LDS, scratch as recorded from the build before hit lists existed)."""
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "k_sdtw_resources.json")))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), SO, "k_sdtw"],
                         capture_output=True, text=True, check=True).stdout
    got = {}
    for line in out.splitlines()[1:]:
        m = re.match(r"(k_sdtw\w*<[^>]*>)\s+(.*)$", line)
        if m:
            got[m.group(1)] = [int(v) for v in m.group(2).split()]
    assert len(want) > 1000
    missing = [k for k in want if k not in got]
    assert not missing, missing[:5]
    changed = {k: (want[k], got[k]) for k in want if got[k] != want[k]}
    assert not changed, list(changed.items())[:5]
