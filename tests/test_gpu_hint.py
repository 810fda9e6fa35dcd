"""GPU: the start hint of the screening scheme (csrc/sk_sdtwq.hip: k_sdtw_qh / k_sdtw_ph).

The tagged sweep tells the pre-roll where each read's best path starts, so the exact window of a read looks back only
that far.  The hint changes which columns the window pass computes, never a record: with and without it
(SK_DTW_NOHINT=1) every read equals the oracle bit for bit -- distance, start, end -- on small batches that take every
layout the hint has (8 lanes with and without short lanes, 16 lanes), reads long enough for the tag to wrap three
times, and reads picked to mislead it."""
import ctypes as C

import numpy as np
import pytest

from conftest import oracle_motifseq_threaded

pytestmark = pytest.mark.gpu

HOSTILE = 16                                      # the last rows of a batch


def _same(got, want, label):
    bad = np.nonzero((got["start"] != want["start"]) | (got["end"] != want["end"]) | (got["n"] != want["n"])
                     | ~((got["dist"] == want["dist"]) | (np.isnan(got["dist"]) & np.isnan(want["dist"]))))[0]
    assert bad.size == 0, "%s: %d reads differ, first %s: got %s want %s" % (
        label, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


def _window_steps(L):
    ws = (C.c_uint64 * 2)()
    assert L.sk_last_dtw_window_steps(ws) == 0
    return int(ws[1])                             # read-steps the window pass was asked for, all tiers


def _batch(R, M, N):
    from squigglekit_amd import synth
    motif = synth.synthetic_motif(N, seed=11)
    sig = synth.squiggle_batch(R, M, 70000 + N, motif=motif)
    lens = np.full(R, M, dtype=np.int32)
    img = lambda v: np.clip(np.rint(v * 93.4 + 511.0), 1, 1199).astype(np.int16)      # noqa: E731
    copy = img(motif)
    h = R - HOSTILE
    # two copies further apart than one window takes (4 checkpoint intervals = 512 columns): a second window (sibling)
    for r, (a, b) in ((h, (60, M - N - 40)), (h + 1, (300, 300 + 520 + N))):
        sig[r, a:a + N] = copy
        sig[r, b:b + N] = copy
    # copies stretched 3x and 4x: paths wider than every look-back, and (but for 3 x 163) than the tag range of 512 columns
    for r, k in ((h + 2, 3), (h + 3, 4), (h + 4, 3)):
        s = img(np.repeat(motif, k))[:M - 200]
        off = 100 if r != h + 4 else M - s.size - 1
        sig[r, off:off + s.size] = s
    # copies that start in the read's first granule, and one that ends on its last sample
    for r, off in ((h + 5, 0), (h + 6, 5), (h + 7, 15), (h + 8, M - N)):
        sig[r, off:off + N] = copy
    sig[h + 9, :] = 500                                                    # constant: MAD = 0
    sig[h + 10, :] = 500 + (np.arange(M) % 2)                              # two levels: every cost ties with many others
    sig[h + 11, :] = np.tile(copy, M // N + 1)[:M]                         # the motif end to end: near-minima everywhere
    lens[h + 12], lens[h + 13], lens[h + 14], lens[h + 15] = N - 37, 1, 0, N + 1   # shorter than the motif, and just longer
    return sig, lens, motif


@pytest.mark.parametrize("R,M,N,lanes", [(512, 1600, 200, "8"),     # 8 lanes x 25 rows, no short lanes
                                         (512, 1600, 163, "8"),     # 8 x 21, five short lanes
                                         (384, 2100, 300, "16")])   # 16 x 19, four short lanes
def test_hinted_windows_equal_the_oracle_and_ask_for_fewer_steps(gpu, ora, monkeypatch, R, M, N, lanes):
    from squigglekit_amd import api
    L = gpu.load()
    monkeypatch.delenv("SK_DTW_NOHINT", raising=False)
    monkeypatch.setenv("SK_DTW_QL", lanes)
    monkeypatch.setenv("SK_DTW_HINT_MIN", "1")                             # (by default only large calls take the hint)
    sig, lens, motif = _batch(R, M, N)
    launches = C.c_int32()

    hinted = api.motifseq_batch(sig, lens, motif)
    L.sk_last_dtw_profile(None, C.byref(launches), None, None, None)
    assert launches.value >= 1, "the batch did not take the screening scheme"
    steps_hint, guard = _window_steps(L), api.last_dtw_guard()
    assert guard["premise_violations"] == 0 and guard["audit_mismatches"] == 0, guard
    assert guard["second_windows"] >= 1, "no read took a second window"

    monkeypatch.setenv("SK_DTW_NOHINT", "1")
    plain = api.motifseq_batch(sig, lens, motif)
    steps_plain, guard = _window_steps(L), api.last_dtw_guard()
    assert guard["premise_violations"] == 0 and guard["audit_mismatches"] == 0, guard
    monkeypatch.delenv("SK_DTW_NOHINT")

    want = oracle_motifseq_threaded(ora, sig, lens, motif)
    ok = (hinted["flags"] & 2) == 0                                        # (MAD = 0: the reference divides by zero)
    assert (~ok).sum() <= 2                                                # the constant read, the one-sample read
    _same(hinted[ok], want[ok], "with the hint")
    _same(plain[ok], want[ok], "SK_DTW_NOHINT=1")
    assert hinted.tobytes() == plain.tobytes()
    print("window read-steps: %d hinted, %d plain (%.2f)" % (steps_hint, steps_plain, steps_hint / steps_plain))
    assert 0 < steps_hint < steps_plain, "the hint did not shorten the windows"

    # the plain synthetic part alone: a hint that is too short costs a read the second tier -- at most 5 % of them
    h = R - HOSTILE
    part = api.motifseq_batch(sig[:h], lens[:h], motif)
    tier2 = int(L.sk_last_dtw_tier2())
    print("second tier: %d of %d reads" % (tier2, h))
    assert part.tobytes() == hinted[:h].tobytes()
    assert tier2 <= 0.05 * h, (tier2, h)


@pytest.mark.parametrize("N", [7, 12])
def test_a_motif_shorter_than_a_granule_keeps_the_plain_kernels(gpu, ora, monkeypatch, N):
    """The restart column of the hint lies up to 15 + 8 columns before the path's start, the plain look-back N + 8 columns
    before the first candidate: below 16 points the hint can only lengthen a window.  Found by
    tests/test_gpu_screen_grid.py: 256 reads over 8 lanes asked for 14 989 window read-steps with the hint against 14 121
    without it at 7 points, 19 451 against 17 148 at 12.  The gate (HINT_MIN_N) now leaves such motifs to k_sdtw_q /
    k_sdtw_p: forcing the hint on changes neither a record nor the work."""
    import randcases as rc
    from squigglekit_amd import api
    L = gpu.load()
    monkeypatch.delenv("SK_DTW_NOHINT", raising=False)
    monkeypatch.setenv("SK_DTW_QL", "8")
    monkeypatch.setenv("SK_DTW_HINT_MIN", "1")
    sig, lens, motif = rc.screen_batch(256, rc.screen_min_len(N), N, 70000 + N)
    launches = C.c_int32()
    asked = api.motifseq_batch(sig, lens, motif)
    L.sk_last_dtw_profile(None, C.byref(launches), None, None, None)
    assert launches.value >= 1, "the batch did not take the screening scheme"
    steps_asked = _window_steps(L)
    monkeypatch.setenv("SK_DTW_NOHINT", "1")
    plain = api.motifseq_batch(sig, lens, motif)
    steps_plain = _window_steps(L)
    want = oracle_motifseq_threaded(ora, sig, lens, motif)
    ok = (plain["flags"] & 2) == 0
    assert (~ok).sum() <= 2
    _same(plain[ok], want[ok], "SK_DTW_NOHINT=1")
    assert asked.tobytes() == plain.tobytes()
    assert 0 < steps_asked == steps_plain, (steps_asked, steps_plain)
