"""GPU: every lane layout and row count of the fixed-point screening scheme (csrc/sk_sdtwq.hip) against the oracle.

Passes Q, P and W, and the tagged sweep k_sdtw_qh with its pre-roll k_sdtw_ph, are one compiled kernel per lanes per
read L and rows per lane R: L = 8 and 16 with R = 1 .. 32, L = 64 with R = 1 .. 16.  qcolumn works in blocks of four
cells plus a remainder, pass Q has a second instantiation without the short-lane select (P = L R - N = 0, R >= 2), the
spills change with R, and the hint has a lane mask per L.  One test per (L, R), forced with SK_DTW_QL, and in it two
motif lengths: N = L R and N = L R - p with p from 1, L / 2 and L - 1 in turn (randcases.screen_grid_lengths), so both
instantiations of pass Q run.  The batch is the smallest the scheme accepts -- 256 reads, rows of
randcases.screen_min_len(N) samples -- built by randcases.screen_batch: planted synthetic rows and 21 rows picked to
mislead the scheme (tests/test_random_cases.py checks the builder on the CPU).

Per N: every record equals the oracle's bit for bit; the guard counters are zero; under L of 8 and 16 the call runs
with the hint asked for (SK_DTW_HINT_MIN=1) and without (SK_DTW_NOHINT=1), and the two results are the same bytes.
Where the library's gate refuses the hint -- more than 25 rows per lane, a motif of fewer than 16 points -- the two runs
report the same work.  A mistake that only costs reads the second tier or the exact retry leaves the records right, so
where the hint applies the test also holds the work down: the hinted windows ask for no more read-steps than the plain
ones (fewer from 128 points on: the only evidence that the hinted kernels ran), the hint sends at most 5 % of the plain
synthetic rows more to the second tier, and fewer than a quarter of the reads take the exact retry in any run.  The
oracle's records of a length are computed once and shared by the layouts that reach it."""
import ctypes as C

import numpy as np
import pytest

import randcases as rc

pytestmark = pytest.mark.gpu

READS = rc.SCREEN_MIN_READS
SWITCHES = [k for k in rc.SWITCHES if k.startswith("SK_DTW_")]
_WANT = {}                                        # N -> the oracle's records of screen_batch(READS, M, N, 70000 + N)


def _same(got, want, label):
    bad = np.nonzero((got["start"] != want["start"]) | (got["end"] != want["end"]) | (got["n"] != want["n"])
                     | ~((rc._bits(got["dist"]) == rc._bits(want["dist"])) | (np.isnan(got["dist"]) & np.isnan(want["dist"]))))[0]
    assert bad.size == 0, "%s: %d reads differ, first %s: got %s want %s" % (
        label, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


class Run:
    """One call and what the library reports about it."""

    def __init__(self, lib, api, sig, lens, motif, label):
        self.hits = api.motifseq_batch(sig, lens, motif)
        launches, ws = C.c_int32(), (C.c_uint64 * 2)()
        lib.sk_last_dtw_profile(None, C.byref(launches), None, None, None)
        assert launches.value >= 1, "%s: the batch did not take the screening scheme" % label
        assert lib.sk_last_dtw_window_steps(ws) == 0
        self.steps = int(ws[1])                   # read-steps the window pass was asked for, all tiers
        self.tier2, self.retries = int(lib.sk_last_dtw_tier2()), int(lib.sk_last_dtw_retries())
        guard = api.last_dtw_guard()
        assert guard["premise_violations"] == 0 and guard["audit_mismatches"] == 0 and guard["alarm"] == 0, (label, guard)
        # a crippled look-back sends more than a quarter of the reads to the exact retry (tests/test_gpu_chunks.py)
        assert 4 * self.retries < len(lens), "%s: %d of %d reads took the exact retry" % (label, self.retries, len(lens))


def _one_length(lib, api, ora, monkeypatch, L, R, N):
    M = rc.screen_min_len(N)
    sig, lens, motif = rc.screen_batch(READS, M, N, 70000 + N)
    assert rc.screen_shape(N, READS, M, str(L)) == (L, R) and int(lens.max()) == M
    h = READS - rc.SCREEN_HOSTILE
    hinted_shape = rc.screen_hint_gate(N, L, R, READS, M, {"SK_DTW_HINT_MIN": "1"})    # L of 8 or 16, R <= 25, N >= 16
    tag = "L=%d R=%d N=%d M=%d" % (L, R, N, M)
    for key in SWITCHES:
        monkeypatch.delenv(key, raising=False)
    monkeypatch.setenv("SK_DTW_QL", str(L))
    runs = {}
    if L in (8, 16):
        monkeypatch.setenv("SK_DTW_HINT_MIN", "1")                         # (by default only large calls take the hint)
        runs["hint"] = Run(lib, api, sig, lens, motif, tag + " with the hint")
        monkeypatch.setenv("SK_DTW_NOHINT", "1")
    runs["plain"] = Run(lib, api, sig, lens, motif, tag + " without the hint")

    if N not in _WANT:
        _WANT[N] = rc.expect_screen(ora, dict(sig=sig, lens=lens, R=READS, motifs=[motif], scale="medmad", lo=0,
                                               hi=1200))["want"][0]
    want = _WANT[N]
    # the reference alone decides which reads are left out: MAD = 0, where it divides by zero -- the constant row and the
    # one-sample row at the most
    out = ~np.isfinite(want["dist"]) & (want["n"] > 0)
    assert out.sum() <= 2 and set(np.flatnonzero(out)) <= {h + 9, h + 13}, (tag, np.flatnonzero(out))
    ok = ~out
    # (the oracle has the true path widths: the rows too wide for the second tier's look-back, which nothing but the exact
    # retry can serve, are far fewer than the quarter of the reads that Run allows)
    wide = (want["end"] - want["start"] + 1 > 2 * N + N // 4 + 16) & ok
    assert wide.sum() <= rc.SCREEN_HOSTILE and 16 * rc.SCREEN_HOSTILE < 4 * READS, (tag, int(wide.sum()))
    for name, run in runs.items():
        assert np.all((run.hits["flags"][out] & 2) != 0) and np.all((run.hits["flags"][ok] & 2) == 0), (tag, name)
        _same(run.hits[ok], want[ok], "%s, %s" % (tag, name))
    if "hint" not in runs:
        return
    hint, plain = runs["hint"], runs["plain"]
    assert hint.hits.tobytes() == plain.hits.tobytes(), tag
    if not hinted_shape:  # more than 25 rows per lane, or a motif shorter than a granule: the gate keeps the plain kernels
        assert (hint.steps, hint.tier2, hint.retries) == (plain.steps, plain.tier2, plain.retries), tag
        return
    print("%s: window read-steps %d hinted, %d plain (%.3f); second tier %d / %d; retries %d / %d" % (
        tag, hint.steps, plain.steps, hint.steps / max(plain.steps, 1), hint.tier2, plain.tier2, hint.retries,
        plain.retries))
    assert 0 < hint.steps <= plain.steps, "%s: the hint lengthened the windows" % tag
    if N >= 128:          # (below, the hint's granule of 16 columns and margin of 8 can equal the plain look-back of N + 8)
        assert hint.steps < plain.steps, "%s: the hint did not shorten the windows" % tag
    # the plain synthetic rows alone, repeated up to 256 reads: a hint that is too short costs a read the second tier --
    # at most 5 % of the reads more than without it
    idx = np.arange(READS) % h
    part_plain = Run(lib, api, sig[idx], lens[idx], motif, tag + " plain rows without the hint")
    monkeypatch.delenv("SK_DTW_NOHINT")
    part_hint = Run(lib, api, sig[idx], lens[idx], motif, tag + " plain rows with the hint")
    print("%s: second tier on the plain rows %d hinted, %d plain" % (tag, part_hint.tier2, part_plain.tier2))
    assert part_hint.hits.tobytes() == hint.hits[idx].tobytes() and part_plain.hits.tobytes() == part_hint.hits.tobytes(), tag
    assert part_hint.tier2 <= part_plain.tier2 + 0.05 * READS, (tag, part_hint.tier2, part_plain.tier2)


@pytest.mark.parametrize("L,R", rc.SCREEN_GRID, ids=["L%d-R%d" % lr for lr in rc.SCREEN_GRID])
def test_screening_shape_equals_the_oracle(gpu, ora, monkeypatch, L, R):
    from squigglekit_amd import api
    lengths = rc.screen_grid_lengths(L, R)
    assert lengths[0] == L * R and (R == 1 or len(lengths) == 2)
    for N in lengths:
        _one_length(gpu.load(), api, ora, monkeypatch, L, R, N)
