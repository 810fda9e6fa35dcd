"""MotifSeq panel inside a search region, host side (no GPU): the slice rule, the ranking rule, the parser's refusals,
the ABI structs -- and the reference composition the GPU tests (test_gpu_panel.py) compare against: Python slices of the
raw reads, the oracle's filter + normalisation + dtw_subsequence on each slice, numpy's (dist - mean) / sd, ranked."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLD

MODEL = os.path.join(GOLD, "CATCTATCCAGGGTTAAATT.model")
SLOPE, INTERCEPT, STD_CONST = 2.90, -9.6, 0.08468                 # MotifSeq.py's defaults (:441-442)


# ---- the reference composition -------------------------------------------------------------------------------------
def model_terms(motifs):
    """mean[k] = slope * L_k + intercept, sd[k] = mean[k] * std_const (MotifSeq.py:441-442)."""
    mean = np.array([(SLOPE * len(m)) + INTERCEPT for m in motifs], dtype=np.float64)
    return mean, mean * STD_CONST


def rank_scores(scores):
    """The ranking rule on a [K, R] score table: best = the smallest score (ties: the smallest k), second = the best of
    the rest, NaN never ranked.  Returns (best[R], second[R], score_best[R], score_second[R]); -1 / NaN where none."""
    scores = np.asarray(scores, dtype=np.float64)
    K, R = scores.shape

    def sweep(skip):
        idx = np.full(R, -1, dtype=np.int32)
        val = np.full(R, np.nan)
        for k in range(K):
            s = scores[k]
            with np.errstate(invalid="ignore"):
                take = ~np.isnan(s) & (k != skip) & ((idx < 0) | (s < val))
            idx[take] = k
            val[take] = s[take]
        return idx, val
    best, sb = sweep(np.full(R, -2))
    second, ss = sweep(best)
    return best, second, sb, ss


def brute_rank(col):
    """One read's scores -> (best, second) by sorting (score, k) pairs."""
    order = sorted((float(s), k) for k, s in enumerate(col) if not np.isnan(s))
    return (order[0][1] if order else -1), (order[1][1] if len(order) > 1 else -1)


def slices_of(reads, region, win):
    """[(window, raw begin)] per read: raw[a:b] as Python cuts it."""
    out = []
    for r, raw in enumerate(reads):
        a, b = (int(win[r][0]), int(win[r][1])) if win is not None else region
        lo = slice(a, b).indices(len(raw))[0]
        out.append((np.asarray(raw)[slice(a, b)], lo))
    return out


def oracle_records(ora, windows, motifs, scale, lo=0, hi=1200):
    """[K][R] records of the oracle on the sliced reads, with the two flags the library documents added: 1 = nothing
    survives the filter, 2 = medmad with MAD 0 (the reference divides by zero: dist is then not compared)."""
    from conftest import oracle_motifseq_threaded
    R = len(windows)
    mode = 0 if scale == "medmad" else 1
    ints = all(np.asarray(w).dtype.kind in "iu" for w in windows)
    recs = np.zeros((len(motifs), R), dtype=ora.HIT_DTYPE)
    if ints:
        stride = max(8, max((len(w) for w in windows), default=0))
        rows = np.zeros((R, stride), dtype=np.int16)
        lens = np.array([len(w) for w in windows], dtype=np.int32)
        for r, w in enumerate(windows):
            rows[r, :len(w)] = w
        for k, m in enumerate(motifs):
            recs[k] = oracle_motifseq_threaded(ora, rows, lens, m, scale_mode=mode) if R else recs[k]
    else:
        for r, w in enumerate(windows):
            f = ora.scale_outliers(np.asarray(w, dtype=np.float64), lo, hi)
            y = f if not f.size else (ora.medmad(f)[0] if mode == 0 else ora.zscale(f)[0])
            for k, m in enumerate(motifs):
                recs[k][r] = ((np.nan, -1, -1, 0, 0) if not f.size else
                              ora.dtw_subsequence(m, y) + (f.size, 0)) if np.all(np.isfinite(y)) else (np.nan, -1, -1, f.size, 0)
    flags = np.zeros(R, dtype=np.int32)
    for r, w in enumerate(windows):
        w = np.asarray(w, dtype=np.float64)
        f = w[(w > lo) & (w < hi)]
        if not f.size:
            flags[r] = 1
        elif mode == 0 and np.median(np.abs(f - np.median(f))) == 0:
            flags[r] = 2
    return recs, flags


def reference_panel(ora, reads, motifs, region=(0, None), win=None, scale="medmad"):
    """(records [K][R], flags [R], from [R], best, second, score_best, score_second) by the reference alone."""
    cut = slices_of(reads, region, win)
    recs, flags = oracle_records(ora, [w for w, _ in cut], motifs, scale)
    mean, sd = model_terms(motifs)
    with np.errstate(all="ignore"):
        scores = (recs["dist"] - mean[:, None]) / sd[:, None]
    scores[:, flags != 0] = np.nan
    return (recs, flags, np.array([lo for _, lo in cut], dtype=np.int32)) + rank_scores(scores)


# ---- the test data of the GPU tests (checked here, where no GPU is needed) ---------------------------------------------
def relevel(model, rng):
    """The model's dwell structure (its runs of equal values) with new seeded levels of the model's own spread."""
    edges = np.flatnonzero(np.diff(model) != 0) + 1
    runs = np.diff(np.concatenate([[0], edges, [model.size]]))
    return np.repeat(rng.normal(0.0, float(np.std(model)), size=runs.size), runs)


def panel_motifs(model, seed=2024):
    """12 motifs from the 163-point example model: the model, eight seeded perturbations (its dwell structure with other
    levels: eight other k-mer sequences), two truncations of different length (other shape groups) and one of more than
    1 024 points (seven perturbed copies end to end)."""
    rng = np.random.default_rng(seed)
    pert = [relevel(model, rng) for _ in range(8)]
    long = np.concatenate([relevel(model, rng) for _ in range(7)])
    return [model] + pert + [pert[2][:100].copy(), pert[5][:60].copy(), long]


def panel_reads(motifs, R=64, M=6000, seed=77):
    """Seeded synthetic int16 reads by the project's recipe (synth.squiggle_batch, behind its stall); every second read carries round(motif_k * 93.4 + 511) of a
    random k inside its first 2 000 samples and again inside its last 3 000.  Returns (reads [R, M], implanted k or -1).
    Reads R-3 .. R-1: a constant first window (MAD 0 there), nothing inside the limits anywhere, a short read's worth of
    zeros at the front."""
    from squigglekit_amd import synth
    rng = np.random.default_rng(seed)
    # (the recipe opens every read with a stall plateau of up to 660 samples; it is cut off here, or the tight plateau
    # would set the MAD of the first window and no implant would sit at the scale it was written in)
    sig = np.ascontiguousarray(synth.squiggle_batch(R, M + 700, seed)[:, 700:])
    planted = np.full(R, -1, dtype=np.int32)
    for r in range(0, R - 3, 2):
        k = int(rng.integers(0, len(motifs)))
        img = np.round(motifs[k] * 93.4 + 511).astype(np.int16)
        a = int(rng.integers(0, 2000 - img.size))
        b = int(rng.integers(M - 3000, M - img.size))
        sig[r, a:a + img.size] = img
        sig[r, b:b + img.size] = img
        planted[r] = k
    sig[R - 3, :2000] = 500
    sig[R - 2, :] = 2000
    sig[R - 1, :700] = 0
    return sig, planted


# ---- slice rule ------------------------------------------------------------------------------------------------------
def test_resolve_region_equals_slice_indices():
    from squigglekit_amd import api
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 60, size=4000)
    lens[:50] = 0
    for _ in range(60):
        a, b = (None if rng.random() < 0.15 else int(v) for v in rng.integers(-90, 90, size=2))
        got = api.resolve_region(lens, a, b)
        want = np.array([slice(a, b).indices(int(n))[:2] for n in lens])
        assert np.array_equal(got, want), (a, b)
    got = api.resolve_region([10, 0, 3], -3000, None)                   # far out of range, and the "to the end" form
    assert got.tolist() == [[0, 10], [0, 0], [0, 3]]
    assert api.resolve_region([10], 500, 500).tolist() == [[10, 10]]    # empty
    assert api.resolve_region([10], 7, 2).tolist() == [[7, 2]]          # stop < start: empty, as slice.indices says
    assert api.resolve_region([100], 0, 2 ** 31 - 1).tolist() == [[0, 100]]


# ---- ranking rule ----------------------------------------------------------------------------------------------------
def test_ranking_rule_against_brute_force():
    rng = np.random.default_rng(9)
    for K in (1, 2, 3, 7, 12):
        s = rng.integers(-2, 3, size=(K, 500)).astype(np.float64)        # tie heavy
        s[rng.random(s.shape) < 0.3] = np.nan
        s[rng.random(s.shape) < 0.05] = np.inf
        s[:, :5] = np.nan                                                # nothing to rank
        best, second, sb, ss = rank_scores(s)
        for r in range(s.shape[1]):
            b, c = brute_rank(s[:, r])
            assert (best[r], second[r]) == (b, c), (K, r, s[:, r])
            assert (np.isnan(sb[r]) if b < 0 else sb[r] == s[b, r]) and (np.isnan(ss[r]) if c < 0 else ss[r] == s[c, r])
        if K == 1:
            assert np.all(second == -1) and np.all(np.isnan(ss))


# ---- parser ----------------------------------------------------------------------------------------------------------
def _exit_code(argv):
    import contextlib
    import io
    from squigglekit_amd.motifseq_cli import main
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            main(argv)
        except SystemExit as e:
            return e.code, err.getvalue()
    return 0, err.getvalue()


def test_parser_refusals(tmp_path):
    sigfile = tmp_path / "none.tsv"
    sigfile.write_text("")
    code, err = _exit_code(["-s", str(sigfile), "-m", MODEL, "--region", "0:2000", "--after_stall"])
    assert code == 2 and "--region does not combine with --after_stall" in err
    code, err = _exit_code(["-s", str(sigfile), "-m", MODEL, "--panel"])                # the model file holds one motif
    assert code == 2 and "--panel needs two or more motifs" in err
    for bad in ("12", "a:b", "1:2:3"):
        code, err = _exit_code(["-s", str(sigfile), "-m", MODEL, "--region", bad])
        assert code == 2 and "--region takes A:B" in err, bad
    from squigglekit_amd.motifseq_cli import build_parser, check_hit_flags
    p = build_parser()
    for text, want in (("0:2000", (0, 2000)), ("-3000:", (-3000, None)), (":", (0, None)), (":-5", (0, -5))):
        args = p.parse_args(["--region=" + text])
        check_hit_flags(p, args)
        assert args.region == want


# ---- ABI -------------------------------------------------------------------------------------------------------------
def test_panel_struct_sizes():
    from squigglekit_amd import _lib
    assert ctypes.sizeof(_lib.PanelRec) == 48 and _lib.PANEL_DTYPE.itemsize == 48
    assert _lib.PanelRec.hit.offset == 24 and _lib.PANEL_DTYPE.fields["hit"][1] == 24
    assert _lib.PanelRec.score_best.offset == 8 and _lib.PanelRec.score_second.offset == 16
    for name in ("sk_motifseq_panel_i16", "sk_motifseq_panel_dev_i16", "sk_motifseq_panel_f64", "sk_region_rows_i16"):
        assert name in _lib.ABI


# ---- the GPU tests' data under the oracle ----------------------------------------------------------------------------
def test_oracle_composition_handles_the_test_data(ora, example_model):
    """No exception on the empty slice, MAD = 0 rows flagged, and the implants are found: at least 40 % of the implanted
    reads rank their implanted motif first (a condition on the data, not on the code under test)."""
    motifs = panel_motifs(example_model)
    assert len(motifs) == 12 and len({len(m) for m in motifs}) >= 4 and max(len(m) for m in motifs) > 1024
    sig, planted = panel_reads(motifs)
    reads = list(sig)
    recs, flags, frm, best, second, sb, ss = reference_panel(ora, reads, motifs, (500, 500))
    assert np.all(flags == 1) and np.all(best == -1) and np.all(frm == 500) and np.all(np.isnan(recs["dist"]))
    recs, flags, frm, best, second, sb, ss = reference_panel(ora, reads, motifs, (0, 2000))
    R = len(reads)
    assert flags[R - 3] == 2 and flags[R - 2] == 1 and np.count_nonzero(flags) == 2
    assert best[R - 3] == -1 and best[R - 2] == -1 and np.all(recs["n"][:, R - 1] <= 1300) and np.all(recs["n"][:, R - 1] > 1200)
    imp = planted >= 0
    share = float(np.mean(best[imp] == planted[imp]))
    assert share >= 0.4, share
    ok = flags == 0
    assert np.all(best[ok] >= 0) and np.all(second[ok] >= 0) and np.all(sb[ok] <= ss[ok])
