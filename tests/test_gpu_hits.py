"""MotifSeq hit lists on the GPU (sk_motifseq_hits_*, api.motifseq_hits*, MotifSeq --hits): bit for bit the numpy
statement of the contract in test_hits_host.py, hit 1 = the default path's record, the CLI's lines."""
import os

import numpy as np
import pytest

from conftest import GOLD
from test_cli import run_cli, scrappy_stub, tsv_files          # noqa: F401  (fixtures)
from test_hits_host import reference_hits

pytestmark = pytest.mark.gpu
MODEL = os.path.join(GOLD, "CATCTATCCAGGGTTAAATT.model")


def same(got, want, tag=""):
    """got = (hits[R, K], count[R]) against reference_hits' lists (None: count 0, flagged)."""
    hits, count = got
    for r, w in enumerate(want):
        if w is None:
            assert count[r] == 0 and hits[r, 0]["flags"] & 3, (tag, r)
            continue
        g = [(float(h["dist"]), int(h["start"]), int(h["end"])) for h in hits[r, :count[r]]]
        assert count[r] == len(w) and [x[1:] for x in g] == [x[1:] for x in w], (tag, r, g[:4], w[:4])
        assert all(np.float64(a[0]).tobytes() == np.float64(b[0]).tobytes() for a, b in zip(g, w)), (tag, r)
        rest = hits[r, count[r]:]
        assert np.all(np.isnan(rest["dist"])) and np.all(rest["start"] == -1) and np.all(rest["end"] == -1), (tag, r)


def mixed_reads(N, seed):
    """reads of every kind the contract names: empty after the filter, shorter than the motif, up to 4 000 samples,
    tie-heavy small integers"""
    from squigglekit_amd import synth
    motif = synth.synthetic_motif(N, seed=seed)
    base = synth.squiggle_batch(6, 4000, 1000 + seed, motif=motif)
    rng = np.random.default_rng(seed)
    reads = [np.full(40, 2000, dtype=np.int16),                                 # nothing survives scale_outliers
             base[0, :max(1, N // 2)], base[1, :300], base[2, :1500], base[3], base[4, :2500],
             (500 + rng.integers(0, 3, size=700)).astype(np.int16),            # ties everywhere
             (480 + 10 * rng.integers(0, 4, size=4000)).astype(np.int16)]
    return motif, reads


@pytest.mark.parametrize("N", [1, 15, 16, 17, 63, 64, 65, 200, 1024, 1025])
def test_int16_medmad_matches_the_reference(gpu, ora, N):
    from squigglekit_amd import api
    motif, reads = mixed_reads(N, N)
    for K in (1, 3, 64):
        want = reference_hits(ora, reads, motif, K)
        same(api.motifseq_hits(reads, [motif], K)[0], want, "N=%d K=%d" % (N, K))
    full = reference_hits(ora, reads, motif, 64)
    cut = float(np.median([h[1][0] for h in full if h and len(h) > 1]))
    same(api.motifseq_hits(reads, [motif], 8, max_dist=cut)[0], reference_hits(ora, reads, motif, 8, cut), "cut")


@pytest.mark.parametrize("N", [17, 200])
def test_batch_lane_layout_matches_the_reference(gpu, ora, monkeypatch, N):
    from squigglekit_amd import api
    monkeypatch.setenv("SK_DTW_SMALL_MAX", "0")                              # four reads per wavefront, as big batches
    motif, reads = mixed_reads(N, 3 * N)
    same(api.motifseq_hits(reads, [motif], 5)[0], reference_hits(ora, reads, motif, 5), "L16")


def test_zscale_and_float64_pa_match_the_reference(gpu, ora):
    from squigglekit_amd import api
    motif, reads = mixed_reads(200, 5)
    same(api.motifseq_hits(reads, [motif], 4, scale="zscale")[0], reference_hits(ora, reads, motif, 4, scale="zscale"))
    pa = [np.round((r.astype(np.int64) + 16.0) * (1493.94 / 8192.0), 2) for r in reads[1:]]
    for scale in ("medmad", "zscale"):
        same(api.motifseq_hits(pa, [motif], 6, scale=scale)[0], reference_hits(ora, pa, motif, 6, scale=scale), scale)
    flat, off = api.pack_f64(pa)
    centi = np.round(flat * 100).astype(np.int32)                              # centi-units, as the TSV tokenizer gives
    same(api.motifseq_hits_ragged_f64(centi, off, [motif], 6)[0], reference_hits(ora, pa, motif, 6), "centi")


def test_hit_one_is_the_default_record_on_a_large_batch(gpu):
    from squigglekit_amd import _lib, api, synth
    import ctypes as C
    motif = synth.synthetic_motif(200)
    sig = synth.squiggle_batch(20000, 4000, 2024, motif=motif)
    lens = np.full(20000, 4000, dtype=np.int32)
    want = api.motifseq_multi_batch(sig, lens, [motif])[0]
    launches = C.c_int32()
    _lib.load().sk_last_dtw_profile(None, C.byref(launches), None, None, None)
    assert launches.value >= 1, "the default call did not take the screening scheme"
    hits, count = api.motifseq_hits_batch(sig, lens, [motif], 8)[0]
    assert np.all(count >= 1)
    assert hits[:, 0].tobytes() == want.tobytes()
    d = hits["dist"]
    ok = np.arange(8)[None, :] < count[:, None]
    assert np.all(np.where(ok[:, 1:], d[:, 1:] >= d[:, :-1], True))
    for r in range(0, 20000, 997):                                             # disjoint intervals
        iv = sorted((int(h["start"]), int(h["end"])) for h in hits[r, :count[r]])
        assert all(a[1] < b[0] for a, b in zip(iv, iv[1:]))


def test_long_read_and_many_row_chunks(gpu, ora, monkeypatch):
    from squigglekit_amd import api, synth
    motif = synth.synthetic_motif(30, seed=2)
    long = synth.squiggle_batch(1, 200000, 55, motif=motif)[0]
    same(api.motifseq_hits([long], [motif], 8)[0], reference_hits(ora, [long], motif, 8), "200k")
    m2 = synth.synthetic_motif(90, seed=3)
    sig = synth.squiggle_batch(9, 4000, 66, motif=m2)
    lens = np.full(9, 4000, dtype=np.int32)
    lens[4] = 1234
    one = api.motifseq_hits_batch(sig, lens, [m2, motif], 5)
    monkeypatch.setenv("SK_HITS_ROW_BYTES", "100000")                          # two reads per chunk: five chunks
    many = api.motifseq_hits_batch(sig, lens, [m2, motif], 5)
    for (h1, c1), (h2, c2) in zip(one, many):
        assert h1.tobytes() == h2.tobytes() and np.array_equal(c1, c2)
    same(many[0], reference_hits(ora, [sig[r, :lens[r]] for r in range(9)], m2, 5), "chunks")


def test_sub_batched_call_matches_one_sub_batch(gpu, monkeypatch):
    """The host int16 route of the four families over three sub-batches: the only place where a sub-batch's first read,
    the whole call's read count and the per-motif block offsets all differ.  Same bytes as one sub-batch."""
    from squigglekit_amd import api, synth
    motifs = [synth.synthetic_motif(5, seed=1), synth.synthetic_motif(8, seed=2)]
    R, M = 9000, 128
    sig = synth.squiggle_batch(R, M, 424, motif=motifs[1])
    lens = np.full(R, M, dtype=np.int32)
    lens[::11] = 70
    fns = (api.motifseq_hits_batch, api.motifseq_background_batch, api.motifseq_paths_batch, api.motifseq_events_batch)

    def all_four():
        res = []
        for fn in fns:
            res.append(fn(sig, lens, motifs, 2))
            if fn in fns[2:]:
                assert api.last_path_mismatches() == 0, fn.__name__
        return res
    one = all_four()
    monkeypatch.setenv("SK_INGEST_MB", "1")                              # 4 096 reads a sub-batch at least: 3 sub-batches
    got = all_four()
    for fn, g, o in zip(fns, got, one):
        assert len(g) == len(o) == 2 and all(len(gk) == len(ok) == (2 if fn is fns[0] else 3) for gk, ok in zip(g, o))
        assert all(a.tobytes() == b.tobytes() and a.shape == b.shape for gk, ok in zip(g, o) for a, b in zip(gk, ok)), \
            fn.__name__
    for k in range(2):
        assert got[2][k][2].shape == (R, 2, motifs[k].size, 2) and got[3][k][2].shape == (R, 2, motifs[k].size)
        assert np.array_equal(api.spans_of_events(got[3][k][2]), got[2][k][2]), k
        for g in got[1:]:
            assert g[k][0].tobytes() == got[0][k][0].tobytes() and np.array_equal(g[k][1], got[0][k][1]), k
    assert np.any(got[0][0][1] >= 1) and np.any(got[2][1][2] >= 0)       # (the batch has hits and paths to compare)


def test_mad_zero_read_has_no_hits(gpu):
    from squigglekit_amd import _lib, api, synth
    motif = synth.synthetic_motif(40)
    sig = synth.squiggle_batch(3, 1000, 9, motif=motif)
    sig[1] = 500
    hits, count = api.motifseq_hits_batch(sig, np.full(3, 1000, dtype=np.int32), [motif], 4)[0]
    assert count[1] == 0 and hits[1, 0]["flags"] & _lib.SK_FLAG_DEGENERATE
    assert np.all(np.isnan(hits[1]["dist"])) and np.all(hits[1]["start"] == -1)
    assert count[0] >= 1 and count[2] >= 1


def test_two_ranks_on_one_device_equal_one(gpu, monkeypatch):
    from squigglekit_amd import api, multigpu, synth
    monkeypatch.setenv("SK_OVERSUBSCRIBE", "1")
    multigpu.close_groups()
    motif = synth.synthetic_motif(150, seed=4)
    sig = synth.squiggle_batch(301, 3000, 97531, motif=motif)
    lens = np.full(301, 3000, dtype=np.int32)
    lens[::5] = 2222
    plain = api.motifseq_hits_batch(sig, lens, [motif], 6)[0]
    got = api.motifseq_hits_batch(sig, lens, [motif], 6, devices=[0, 0])[0]
    assert got[0].tobytes() == plain[0].tobytes() and np.array_equal(got[1], plain[1])


def test_planted_copies_are_hits_one_to_four(gpu, ora):
    from squigglekit_amd import api, synth
    rng = np.random.default_rng(123)
    motif = synth.synthetic_motif(100, seed=9)
    y = np.cumsum(rng.normal(size=4000)) * 0.3
    y = (y - y.mean()) / (y.std() + 1e-9) * 2.0
    places = [300, 1200, 2100, 3300]
    for p in places:
        y[p:p + 100] = motif
    raw = np.round(500 + 60 * y).astype(np.int16)                              # the copies in ADC units
    hits, count = api.motifseq_hits([raw], [motif], 4)[0]
    assert count[0] == 4
    iv = sorted((int(h["start"]), int(h["end"])) for h in hits[0])
    # one hit inside each copy (the motif's flat stretches may be matched to fewer samples at either end)
    assert all(p - 5 <= s and e <= p + 104 and e - s >= 50 for (s, e), p in zip(iv, places)), iv
    same((hits, count), reference_hits(ora, [raw], motif, 4), "planted")


# ---- MotifSeq --hits ---------------------------------------------------------------------------------------------
def _cli_inputs(tsv_files, tmp_path):
    from squigglekit_amd import synth
    sig = synth.squiggle_batch(40, 3000, 4242, motif=synth.synthetic_motif(100))
    sig[3] = 500                                                               # MAD = 0
    np.save(tmp_path / "p.npy", sig)
    return [["-s", tsv_files["m_real_raw"]], ["-s", tsv_files["m_real_pA"]], ["-s", tsv_files["m_synthetic6"]],
            ["--blow5", os.path.join(GOLD, "example_0.blow5")], ["--i16", str(tmp_path / "p.npy")]]


def test_cli_hits_one_is_the_default_output(gpu, scrappy_stub, tsv_files, tmp_path):  # noqa: F811
    from squigglekit_amd.motifseq_cli import main
    for inp in _cli_inputs(tsv_files, tmp_path):
        for extra in ([], ["-x"], ["--strict-compat"]):
            argv = inp + ["-m", MODEL] + extra
            want = run_cli(main, argv)
            got = run_cli(main, argv + ["--hits", "1"])
            assert got == want, argv


def test_cli_min_hit_p_filters_the_hit_lines(gpu, scrappy_stub, tsv_files, tmp_path):  # noqa: F811
    from squigglekit_amd.motifseq_cli import main
    for inp in _cli_inputs(tsv_files, tmp_path):
        for extra in ([], ["-x"]):
            argv = inp + ["-m", MODEL, "--hits", "5"] + extra
            out, _, code = run_cli(main, argv)
            assert code == 0
            lines = out.split("\n")[1:-1]
            if "-s" in inp and "m_synthetic6" in inp[1] or "--i16" in inp:
                assert len(lines) > len(set(ln.split("\t")[1] for ln in lines))        # several hits per read
            hp = [float(ln.split("\t")[11]) for ln in lines]
            P = float(np.median(hp)) if hp else 50.0
            got, _, code = run_cli(main, argv + ["--min_hit_p", repr(P)])
            assert code == 0
            keep = [ln for ln, h in zip(lines, hp) if not h < P]
            assert got.split("\n")[1:-1] == keep, argv


def test_wide_outlier_limits(gpu, ora, scrappy_stub, tsv_files, tmp_path):  # noqa: F811
    """Limits wider than the int16 histogram: integer reads take the float64 kernels, same contract; --hits 1 prints
    what the plain command prints."""
    from squigglekit_amd import api
    from squigglekit_amd.motifseq_cli import main
    motif, reads = mixed_reads(200, 8)
    reads = reads[1:]
    lo, hi = -10000, 30000
    same(api.motifseq_hits(reads, [motif], 5, scale_low=lo, scale_hi=hi)[0],
         reference_hits(ora, reads, motif, 5, lo=lo, hi=hi), "wide")
    for inp in _cli_inputs(tsv_files, tmp_path):
        argv = inp + ["-m", MODEL, "--scale_low", str(lo), "--scale_hi", str(hi)]
        want = run_cli(main, argv)
        assert want[2] == 0, (argv, want[1][-300:])
        assert run_cli(main, argv + ["--hits", "1"]) == want, argv
