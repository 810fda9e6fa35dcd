"""MotifSeq read background, host side: the numpy statement of the contract (include/squigglekit_hip.h, sk_bg_rec),
checked on hand-made rows and against the oracle's restatement of numpy's summation order; the ABI symbols and the
record's size; the CLI's flag checks; local_scores.

The reference: d = cost[-1, :] of the oracle's full cost matrix (the row view_region draws, MotifSeq.py:507-513), then
np.mean, np.std, np.median, np.median(np.abs(d - median)) and the count of d < mean - std, all by numpy itself.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_hits_host import normalised

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "squigglekit_hip.h")
NEW_SYMBOLS = ("sk_motifseq_background_i16", "sk_motifseq_background_f64", "sk_motifseq_background_centi",
               "sk_motifseq_background_dev_i16")
FIELDS = ("mean", "std", "median", "mad", "below", "n")


# ---- the reference -----------------------------------------------------------------------------------------------
def row_background(d):
    """The record of one row, by numpy: (mean, std, median, mad, below, n)."""
    d = np.ascontiguousarray(d, dtype=np.float64)
    mean, std, med = np.mean(d), np.std(d), np.median(d)
    mad = np.median(np.abs(d - med))
    return (float(mean), float(std), float(med), float(mad), int(np.count_nonzero(d < mean - std)), int(d.size))


def reference_background(x, y):
    """The record of motif x against the normalised read y: numpy on the oracle's last row."""
    from oracle import oracle as ora
    _, _, _, cost = ora.dtw_subsequence(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), want_cost=True)
    return row_background(cost[-1])


def reference_background_reads(ora, reads, motif, scale="medmad", lo=0, hi=1200):
    """Per raw read its record -- None for a read the reference flags (nothing left by the filter, MAD 0)."""
    out = []
    for raw in reads:
        y = normalised(ora, raw, scale, lo, hi)
        out.append(reference_background(motif, y) if y.size and np.all(np.isfinite(y)) else None)
    return out


def usable(recs):
    """Share of the reads that are unflagged with std > 0 and mad > 0 in the reference (the condition on test inputs)."""
    good = sum(1 for w in recs if w is not None and w[1] > 0 and w[3] > 0)
    return good / max(1, len(recs))


def same_bits(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


# ---- hand-made rows ------------------------------------------------------------------------------------------------
def test_constant_row():
    mean, std, med, mad, below, n = row_background(np.full(100, 3.25))
    assert (mean, std, med, mad, below, n) == (3.25, 0.0, 3.25, 0.0, 0, 100)


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 128, 129, 8191, 8192, 8193, 20000])
def test_tree_corners_against_the_oracle_order(ora, n):
    """np.mean / np.std on a row are the oracle's restatement of numpy's order (serial below 8, eight accumulators up to
    128, split at n / 2 rounded down to a multiple of 8, chunks of 8 192 added serially)."""
    rng = np.random.default_rng(n)
    d = rng.random(n) * 40.0 + rng.random(n)
    mean, std, med, mad, below, cols = row_background(d)
    assert same_bits(mean, ora.mean(d)) and same_bits(std, ora.std(d)) and cols == n
    assert same_bits(std, np.sqrt(ora.np_sum((d - mean) * (d - mean)) / n))
    assert below == sum(1 for v in d if v < mean - std)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 9, 10])
def test_median_and_mad_even_and_odd(n):
    rng = np.random.default_rng(100 + n)
    d = rng.random(n) * 10.0
    s = np.sort(d)
    want = s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2
    _, _, med, mad, _, _ = row_background(d)
    assert same_bits(med, want)
    a = np.sort(np.abs(d - want))
    assert same_bits(mad, a[n // 2] if n % 2 else (a[n // 2 - 1] + a[n // 2]) / 2)


def test_reference_background_is_numpy_on_the_last_row(ora):
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal(20), rng.standard_normal(300)
    _, _, _, cost = ora.dtw_subsequence(x, y, want_cost=True)
    d = cost[-1]
    assert np.all(d >= 0)
    got = reference_background(x, y)
    assert got[5] == 300 and same_bits(got[0], np.mean(d)) and same_bits(got[1], np.std(d))
    assert same_bits(got[2], np.median(d)) and same_bits(got[3], np.median(np.abs(d - np.median(d))))
    assert got[4] == int((d < np.mean(d) - np.std(d)).sum())


def test_pairwise_tree_geometry_the_kernel_relies_on():
    """What wave_pairwise_leaves (csrc/sk_prepw_dev.h) assumes of numpy's split tree of one chunk: leaves of 64 .. 128
    terms (unless the chunk is one leaf) starting at multiples of 8, heap ids below 128 for chunks of up to 4 096 terms
    and below 256 up to 8 192, and every leaf found exactly once by the probes at 64 l (+ 4 096)."""
    def leaves(m):
        out = []

        def rec(s, ln, i):
            if ln > 128:
                n2 = ln // 2 - (ln // 2) % 8
                rec(s, n2, 2 * i)
                rec(s + n2, ln - n2, 2 * i + 1)
            else:
                out.append((i, s, ln))
        rec(0, m, 1)
        return sorted(out)

    def probed(m, probes):
        got = []
        for p in range(0, 4096 * probes, 64):
            s, ln, i = 0, m, 1
            for _ in range(7):
                if ln > 128:
                    n2 = ln // 2 - (ln // 2) % 8
                    if p < s + n2:
                        ln, i = n2, 2 * i
                    else:
                        s, ln, i = s + n2, ln - n2, 2 * i + 1
            if p < m and (p == 0 or s > p - 64):
                got.append((i, s, ln))
        return sorted(got)
    for m in list(range(8, 600)) + list(range(4000, 4200)) + list(range(8100, 8193)) + [2048, 4096, 6000, 8147]:
        lv = leaves(m)
        assert all(s % 8 == 0 and ln <= 128 for _, s, ln in lv) and (len(lv) == 1 or min(ln for _, _, ln in lv) >= 64)
        assert max(i for i, _, _ in lv) < (128 if m <= 4096 else 256), m
        assert probed(m, 2) == lv and (m > 4096 or probed(m, 1) == lv), m
    assert max(i for i, _, _ in leaves(8147)) >= 128                    # seven levels do occur


# ---- ABI -------------------------------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_the_entry_points():
    from squigglekit_amd import _lib
    text = open(HEADER).read()
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        assert name in _lib.ABI, name
        assert len(_lib.ABI[name][1]) == len(m.group(1).split(",")), name
        twin = name.replace("background", "hits")
        assert len(_lib.ABI[name][1]) == len(_lib.ABI[twin][1]) + 1, name
    assert "MotifSeq.py:507-513" in text and "typedef struct sk_bg_rec" in text


def test_record_is_48_bytes():
    from squigglekit_amd import _lib
    assert C.sizeof(_lib.BgRec) == 48 and _lib.BG_DTYPE.itemsize == 48
    assert tuple(f[0] for f in _lib.BgRec._fields_)[:6] == FIELDS == _lib.BG_DTYPE.names
    for name in FIELDS:
        assert getattr(_lib.BgRec, name).offset == _lib.BG_DTYPE.fields[name][1]


# ---- CLI flags -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv, word", [(["--max_local_Z", "-1"], "background"),
                                        (["--background", "BG", "--panel"], "background"),
                                        (["--background", "BG", "--after_stall"], "background")])
def test_cli_rejects_bad_background_flags(argv, word, tmp_path, capsys):
    from squigglekit_amd import motifseq_cli
    sig = tmp_path / "s.tsv"
    sig.write_text("f.fast5\tid0\t1\t2\t3\n")
    model = tmp_path / "m.model"
    model.write_text("pos\tbase\tcurrent\tsd\tdwell\n0\tA\t1.0\t0.1\t8\n")
    argv = [str(tmp_path / a) if a == "BG" else a for a in argv]
    with pytest.raises(SystemExit) as e:
        motifseq_cli.main(["-s", str(sig), "-m", str(model)] + argv)
    assert e.value.code != 0
    out = capsys.readouterr()
    assert "readID\t" not in out.out and word in out.err
    assert not (tmp_path / "BG").exists()


# ---- scores ----------------------------------------------------------------------------------------------------------
def test_local_scores_table():
    from squigglekit_amd import _lib, api
    bg = np.zeros(4, dtype=_lib.BG_DTYPE)
    bg["mean"], bg["std"] = [10.0, 10.0, 5.0, np.nan], [2.0, 0.0, 0.0, np.nan]
    bg["median"], bg["mad"] = [9.0, 9.0, 5.0, np.nan], [1.0, 0.0, 0.0, np.nan]
    dist = np.array([4.0, 4.0, 5.0, 1.0])
    lz, rz = api.local_scores(dist, bg)
    assert lz[0] == (4.0 - 10.0) / 2.0 and rz[0] == (4.0 - 9.0) / (1.0 * 1.4826)
    assert lz[1] == -np.inf and rz[1] == -np.inf                     # std == 0 / mad == 0: the IEEE result
    assert np.isnan(lz[2]) and np.isnan(rz[2]) and np.isnan(lz[3]) and np.isnan(rz[3])
    lz2, rz2 = api.local_scores(np.array([[4.0, 12.0]]), bg[:1, None])   # [R, K] hits against [R, 1] records
    assert lz2.shape == (1, 2) and lz2[0, 1] == 1.0 and rz2[0, 0] == rz[0]
