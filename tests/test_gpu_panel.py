"""MotifSeq panel inside a search region on the GPU (sk_motifseq_panel_*, api.motifseq_panel*, MotifSeq --region /
--panel), bit for bit against the reference composition of test_panel_host.py: Python slices of the raw reads, the
oracle on each slice, numpy's (dist - mean) / sd, ranked.  Never against the code under test."""
import ctypes as C

import numpy as np
import pytest

from test_cli import run_cli
from test_panel_host import model_terms, panel_motifs, panel_reads, rank_scores, reference_panel

pytestmark = pytest.mark.gpu
INT32_MAX = 2 ** 31 - 1


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, ref, tag):
    """got = (panel, from, records per motif) of the library, ref = reference_panel(...).  Every read is compared: a read
    whose MAD is 0 by its flag, n and its unranked panel record (the reference divides by zero there: no distance to
    compare), every other read in every bit of dist and of the scores."""
    from squigglekit_amd import api
    panel, frm, allrec = got
    recs, flags, rfrm, best, second, sb, ss = ref
    assert np.array_equal(frm, rfrm), tag
    cmp = flags != 2
    for k, g in enumerate(allrec):
        assert np.array_equal(g["n"], recs[k]["n"]), (tag, k)
        assert np.array_equal(g["flags"] & 3, flags), (tag, k)
        assert np.array_equal(bits(g["dist"][cmp]), bits(recs[k]["dist"][cmp])), (tag, k)
        assert np.array_equal(g["start"][cmp], recs[k]["start"][cmp]) and np.array_equal(g["end"][cmp], recs[k]["end"][cmp]), (tag, k)
    assert np.array_equal(panel["best"], best) and np.array_equal(panel["second"], second), tag
    assert np.array_equal(bits(panel["score_best"]), bits(sb)), tag
    assert np.array_equal(bits(panel["score_second"]), bits(ss)), tag
    for r in range(len(frm)):
        h = panel["hit"][r]
        if best[r] >= 0:
            assert h.tobytes() == allrec[best[r]][r].tobytes(), (tag, r)
        else:
            assert np.isnan(h["dist"]) and h["start"] == -1 and h["end"] == -1, (tag, r)
            assert h["n"] == recs[0]["n"][r] and h["flags"] & 3 == flags[r], (tag, r)
    g = api.last_dtw_guard()                                            # the screening scheme's guard: no alarm, ever
    assert (g["premise_violations"], g["audit_mismatches"], g["alarm"], g["exact_fallback"]) == (0, 0, 0, 0), (tag, g)


@pytest.fixture(scope="module")
def case(example_model):
    motifs = panel_motifs(example_model)
    sig, planted = panel_reads(motifs)
    return motifs, sig, planted


@pytest.mark.parametrize("region", [(0, 2000), (-3000, None), (500, 500)])
def test_int16_medmad_regions(gpu, ora, case, region):
    from squigglekit_amd import api
    motifs, sig, _ = case
    mean, sd = model_terms(motifs)
    lens = np.full(sig.shape[0], sig.shape[1], dtype=np.int32)
    got = api.motifseq_panel_batch(sig, lens, motifs, mean, sd, region=region, records=True)
    same(got, reference_panel(ora, list(sig), motifs, region), region)
    if region == (500, 500):
        assert np.all(got[0]["hit"]["flags"] & gpu.SK_FLAG_EMPTY) and np.all(got[0]["best"] == -1)


def test_ragged_lengths_and_one_motif(gpu, ora, case):
    from squigglekit_amd import api
    motifs, sig, _ = case
    rng = np.random.default_rng(3)
    reads = [sig[r, :int(n)] for r, n in enumerate(rng.integers(0, sig.shape[1], size=sig.shape[0]))]
    reads[0], reads[1] = sig[0, :0], sig[1, :1]
    mean, sd = model_terms(motifs)
    for region in ((0, 2000), (-3000, None), (-100, 50), (1000, -1000)):
        got = api.motifseq_panel(reads, motifs[:1], mean[:1], sd[:1], region=region, records=True)
        same(got, reference_panel(ora, reads, motifs[:1], region), region)
        assert np.all(got[0]["second"] == -1) and np.all(np.isnan(got[0]["score_second"]))


def test_int16_zscale(gpu, ora, case):
    from squigglekit_amd import api
    motifs, sig, _ = case
    mean, sd = model_terms(motifs)
    got = api.motifseq_panel(list(sig), motifs, mean, sd, region=(0, 2000), scale="zscale", records=True)
    same(got, reference_panel(ora, list(sig), motifs, (0, 2000), scale="zscale"), "zscale")


@pytest.mark.parametrize("scale", ["medmad", "zscale"])
def test_float64_route(gpu, ora, case, scale):
    from squigglekit_amd import api
    motifs, sig, _ = case
    pick = [motifs[0], motifs[3], motifs[9], motifs[11]]
    mean, sd = model_terms(pick)
    pa = [np.round((sig[r].astype(np.int64) + 16.0) * (1493.94 / 8192.0), 2) for r in list(range(20)) + [61, 62, 63]]
    pa[5] = pa[5][:900]
    for region in ((0, 2000), (-3000, None), (500, 500)):
        got = api.motifseq_panel(pa, pick, mean, sd, region=region, scale=scale, records=True)
        same(got, reference_panel(ora, pa, pick, region, scale=scale), (scale, region))


def test_win_from_stall_cuts_equals_after_stall(gpu, ora, example_model):
    from squigglekit_amd import api, synth
    sig = synth.squiggle_batch(40, 4000, 31337, motif=example_model)
    reads = [sig[r, :4000 - 37 * (r % 5)] for r in range(40)]
    cuts = api.stall_cuts(reads)
    assert np.count_nonzero(cuts) >= 20
    win = np.stack([cuts, np.full(len(reads), INT32_MAX)], axis=1)
    mean, sd = model_terms([example_model])
    got = api.motifseq_panel(reads, [example_model], mean, sd, win=win, records=True)
    same(got, reference_panel(ora, reads, [example_model], win=win), "win")
    want, wcuts = api.motifseq_after_stall(reads, example_model)
    assert got[2][0].tobytes() == want.tobytes() and np.array_equal(got[1], wcuts)


def test_sub_batched_call(gpu, ora, monkeypatch):
    from squigglekit_amd import api, synth
    motifs = [synth.synthetic_motif(40, seed=1), synth.synthetic_motif(70, seed=2), synth.synthetic_motif(40, seed=3)]
    R, M = 9000, 1000
    sig = synth.squiggle_batch(R, M, 99173, motif=motifs[1])
    lens = np.full(R, M, dtype=np.int32)
    lens[::11] = 250
    mean, sd = model_terms(motifs)
    one = api.motifseq_panel_batch(sig, lens, motifs, mean, sd, region=(100, 400), records=True)
    monkeypatch.setenv("SK_INGEST_MB", "1")                              # 4 096 reads a sub-batch at least: 3 sub-batches
    got = api.motifseq_panel_batch(sig, lens, motifs, mean, sd, region=(100, 400), records=True)
    assert got[0].tobytes() == one[0].tobytes() and np.array_equal(got[1], one[1])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[2], one[2]))
    same(got, reference_panel(ora, [sig[r, :lens[r]] for r in range(R)], motifs, (100, 400)), "sub-batches")


def test_long_windows_over_many_reads_take_the_default_path(gpu, ora, example_model, monkeypatch):
    """300 reads x 2 000-sample windows: the panel hands each motif to the default DTW path (screening + certified
    window), whose records are the exact ones; SK_PANEL_EXACT=1 keeps the one-grid exact kernel.  Same bits both ways."""
    from squigglekit_amd import api, synth
    motifs = [example_model, example_model[::-1].copy(), example_model[:100].copy()]
    sig = synth.squiggle_batch(300, 4000, 60606, motif=example_model)
    lens = np.full(300, 4000, dtype=np.int32)
    mean, sd = model_terms(motifs)
    got = api.motifseq_panel_batch(sig, lens, motifs, mean, sd, region=(1000, 3000), records=True)
    launches = C.c_int32()
    gpu.load().sk_last_dtw_profile(None, C.byref(launches), None, None, None)
    assert launches.value >= 1, "the long windows did not take the screening scheme"
    same(got, reference_panel(ora, list(sig), motifs, (1000, 3000)), "delegated")
    monkeypatch.setenv("SK_PANEL_EXACT", "1")
    exact = api.motifseq_panel_batch(sig, lens, motifs, mean, sd, region=(1000, 3000), records=True)
    assert exact[0].tobytes() == got[0].tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(exact[2], got[2]))


def test_device_resident_form_and_two_ranks(gpu, case, monkeypatch):
    from squigglekit_amd import api, multigpu
    motifs, sig, _ = case
    L = gpu.load()
    R, M = sig.shape
    mean, sd = model_terms(motifs)
    lens = np.full(R, M, dtype=np.int32)
    want = api.motifseq_panel_batch(sig, lens, motifs, mean, sd, region=(0, 2000), records=True)
    flat = np.ascontiguousarray(np.concatenate(motifs))
    moff = np.concatenate([[0], np.cumsum([m.size for m in motifs])]).astype(np.int32)
    K = len(motifs)
    sizes = [sig.nbytes, lens.nbytes, R * 48, R * 4, K * R * 24]
    d_sig, d_len, d_out, d_from, d_all = (L.sk_dev_alloc(n) for n in sizes)
    try:
        gpu.check(L.sk_dev_upload(d_sig, gpu.ptr(sig), sig.nbytes))
        gpu.check(L.sk_dev_upload(d_len, gpu.ptr(lens), lens.nbytes))
        for with_all in (True, False):
            gpu.check(L.sk_motifseq_panel_dev_i16(d_sig, M, d_len, R, 0, 2000, None, gpu.ptr(flat), gpu.ptr(moff), K, gpu.ptr(mean),
                                                  gpu.ptr(sd), 0, 0, 1200, d_out, d_from, d_all if with_all else None))
            gpu.check(L.sk_sync())
            out = np.zeros(R, dtype=gpu.PANEL_DTYPE)
            frm = np.zeros(R, dtype=np.int32)
            allrec = np.zeros((K, R), dtype=gpu.HIT_DTYPE)
            gpu.check(L.sk_dev_download(gpu.ptr(out), d_out, out.nbytes))
            gpu.check(L.sk_dev_download(gpu.ptr(frm), d_from, frm.nbytes))
            gpu.check(L.sk_dev_download(gpu.ptr(allrec), d_all, allrec.nbytes))
            assert out.tobytes() == want[0].tobytes() and np.array_equal(frm, want[1])
            assert all(allrec[k].tobytes() == want[2][k].tobytes() for k in range(K))
    finally:
        for p in (d_sig, d_len, d_out, d_from, d_all):
            L.sk_dev_free(p)
    monkeypatch.setenv("SK_OVERSUBSCRIBE", "1")
    multigpu.close_groups()
    two = api.motifseq_panel_batch(sig, lens, motifs, mean, sd, region=(0, 2000), records=True, devices=[0, 0])
    assert two[0].tobytes() == want[0].tobytes() and np.array_equal(two[1], want[1])


def test_invalid_arguments(gpu, case):
    from squigglekit_amd import api
    motifs, sig, _ = case
    L = gpu.load()
    sig = np.ascontiguousarray(sig[:4])
    lens = np.full(4, sig.shape[1], dtype=np.int32)
    mean, sd = model_terms(motifs[:2])
    flat = np.ascontiguousarray(np.concatenate(motifs[:2]))
    moff = np.array([0, 163, 326], dtype=np.int32)
    out = np.zeros(4, dtype=gpu.PANEL_DTYPE)

    def call(nm=2, moff=moff, mean=mean, sd=sd, win=None, out=out):
        return L.sk_motifseq_panel_i16(gpu.ptr(sig), sig.shape[1], gpu.ptr(lens), 4, 0, 2000, None if win is None else gpu.ptr(win),
                                       gpu.ptr(flat), gpu.ptr(moff), nm, None if mean is None else gpu.ptr(mean),
                                       None if sd is None else gpu.ptr(sd), 0, 0, 1200, None if out is None else gpu.ptr(out),
                                       None, None)
    assert call() == 0
    assert call(nm=0) == gpu.SK_ERR_INVALID and call(nm=257) == gpu.SK_ERR_INVALID
    assert call(moff=np.array([0, 163, 163], dtype=np.int32)) == gpu.SK_ERR_INVALID            # an empty motif
    assert call(sd=np.array([1.0, 0.0])) == gpu.SK_ERR_INVALID
    assert call(sd=np.array([1.0, np.inf])) == gpu.SK_ERR_INVALID and call(mean=np.array([np.nan, 1.0])) == gpu.SK_ERR_INVALID
    assert call(mean=None) == gpu.SK_ERR_INVALID and call(out=None) == gpu.SK_ERR_INVALID
    bad = np.array([[0, 100], [500, 300], [0, 100], [0, 100]], dtype=np.int32)
    assert call(win=bad) == gpu.SK_ERR_INVALID and b"win[1]" in L.sk_last_error()
    fine = np.array([[0, 100], [10 ** 6, -10 ** 6], [300, 300], [-50, INT32_MAX]], dtype=np.int32)   # row 1: both cut to the read
    assert call(win=fine) == 0
    assert out["hit"]["n"].tolist()[1:3] == [0, 0] and out["best"][1] == -1
    with pytest.raises(ValueError):
        api.motifseq_panel(list(sig), [], [], [])


# ---- MotifSeq --region / --panel -------------------------------------------------------------------------------------
def _cli_files(tmp_path, motifs, sig):
    bait = tmp_path / "panel.tsv"
    names = ["bc%02d" % k for k in range(4)]
    pick = [motifs[0], motifs[1], motifs[9], motifs[4]]
    bait.write_text("".join("%s\t20\t.\t%s\n" % (n, "\t".join(repr(float(v)) for v in m)) for n, m in zip(names, pick)))
    rows = np.ascontiguousarray(sig[:24])
    rows[5] = 500                                                       # MAD = 0
    npy = tmp_path / "p.npy"
    np.save(npy, rows)
    tsv = tmp_path / "p.tsv"
    tsv.write_text("".join("\t".join(["p.npy", str(r)] + ["c%d" % i for i in range(6)] + [str(int(v)) for v in rows[r]]) + "\n"
                           for r in range(rows.shape[0])))
    return str(bait), str(npy), str(tsv), rows, pick, names


def test_cli_panel_over_packed_and_tsv_input(gpu, case, tmp_path):
    from squigglekit_amd import api, fastio
    from squigglekit_amd.motifseq_cli import main, PANEL_HEADER
    motifs, sig, _ = case
    bait, npy, tsv, rows, pick, names = _cli_files(tmp_path, motifs, sig)
    a = run_cli(main, ["--i16", npy, "-m", bait, "--panel", "--region", "0:2000"])
    b = run_cli(main, ["-s", tsv, "-m", bait, "--panel", "--region", "0:2000"])
    assert a[2] == 0 and b[2] == 0 and a[0] == b[0]
    lines = a[0].split("\n")[:-1]
    assert lines[0].split("\t") == PANEL_HEADER and len(lines) == 1 + 23 and "the MAD of 5 is 0" in a[1]
    mean = np.array([(2.90 * 20) + -9.6] * 4)
    panel, frm = api.motifseq_panel(list(rows), pick, mean, mean * 0.08468, region=(0, 2000))
    keep = [r for r in range(24) if r != 5]
    for ln, r in zip(lines[1:], keep):
        f = ln.split("\t")
        p = panel[r]
        z = float(p["score_best"])
        pv = float(fastio.ndtr(z))
        assert f[:6] == ["p.npy", str(r), names[p["best"]], str(p["hit"]["start"]), str(p["hit"]["end"]),
                         str(p["hit"]["end"] - p["hit"]["start"])]
        assert f[6:] == [repr(float(p["hit"]["dist"])), repr(z), repr(pv), repr((1 - pv) * 100), names[p["second"]],
                         repr(float(p["score_second"])), repr(float(p["score_second"]) - z), str(frm[r])]
    whole = run_cli(main, ["--i16", npy, "-m", bait, "--panel"])         # --panel implies nothing about the region
    assert whole[2] == 0 and whole[0] == run_cli(main, ["--i16", npy, "-m", bait, "--panel", "--region", ":"])[0]


def test_cli_region_with_hits_and_paths_equals_presliced_input(gpu, case, tmp_path):
    from squigglekit_amd.motifseq_cli import main
    motifs, sig, _ = case
    bait, npy, tsv, rows, pick, names = _cli_files(tmp_path, motifs, sig)
    for region, cut, lo in (("0:2000", slice(0, 2000), 0), ("-3000:", slice(-3000, None), rows.shape[1] - 3000)):
        pre = tmp_path / "pre.npy"
        np.save(pre, np.ascontiguousarray(rows[:, cut]))
        pa, pb = str(tmp_path / "a.paths"), str(tmp_path / "b.paths")
        got = run_cli(main, ["--i16", npy, "-m", bait, "--region=" + region, "--hits", "3", "--paths", pa])
        want = run_cli(main, ["--i16", str(pre), "-m", bait, "--hits", "3", "--paths", pb])
        assert got[2] == 0 and want[2] == 0
        gl, wl = got[0].split("\n")[:-1], want[0].split("\n")[:-1]
        assert len(gl) == len(wl) > 24 and gl[0] == wl[0] + "\tsearch_from"
        assert gl[1:] == [w.replace("pre.npy", "p.npy", 1) + "\t%d" % lo for w in wl[1:]]
        assert open(pa).read() == open(pb).read().replace("pre.npy", "p.npy")
        plain = run_cli(main, ["--i16", npy, "-m", bait, "--region=" + region])
        pre_plain = run_cli(main, ["--i16", str(pre), "-m", bait])
        assert plain[0].split("\n")[1:-1] == [w.replace("pre.npy", "p.npy", 1) + "\t%d" % lo for w in pre_plain[0].split("\n")[1:-1]]


# ---- every seam of the pieces the panel shares with the first-match path, in one call --------------------------------
SEAM_POINTS = (1, 15, 16, 17, 31, 32, 255, 256, 257, 1024, 1025)
SEAM_REGION = (0, 300)


@pytest.fixture(scope="module")
def seams(ora):
    """Eleven motifs around every lane and row boundary (1, 15 and 16 points share (L = 16, R = 1) with 15, 1 and 0 short
    lanes: one grid with blockIdx.y > 0, a table entry of its own per motif, and a lane 0 that owns no row; 1 025 points
    take the chained launcher) and seven reads -- not a multiple of four, so the last wavefront has dead lane groups --
    of 0, 300 (every sample outside the limits), 1 and 64 .. 300 samples, as int16 rows and as float64 pA values; the
    reference composition of both, computed once."""
    from squigglekit_amd import synth
    motifs = [synth.synthetic_motif(n, seed=40 + i) for i, n in enumerate(SEAM_POINTS)]
    sig = synth.squiggle_batch(7, 1000, 4242, motif=motifs[4])[:, 700:]         # (behind the recipe's stall plateau)
    ints = [sig[0, :0], np.full(300, 2000, dtype=np.int16), sig[2, :1], sig[3, :64], sig[4, :137], sig[5, :211], sig[6, :300]]
    flts = [np.round((x.astype(np.int64) + 16.0) * (1493.94 / 8192.0), 2) for x in ints]
    flts[1] = np.full(300, 2000.25)
    assert [x.size for x in ints] == [0, 300, 1, 64, 137, 211, 300]
    return motifs, {"int16": ints, "float64": flts}, {k: reference_panel(ora, v, motifs, SEAM_REGION)
                                                      for k, v in (("int16", ints), ("float64", flts))}


@pytest.mark.parametrize("route", ["int16", "float64"])
@pytest.mark.parametrize("no_small", [False, True])
def test_every_seam_of_the_shared_sweep(gpu, seams, monkeypatch, no_small, route):
    """77 (read, motif) pairs, far below the 256 reads at which a group is delegated to the screening path: the one-grid
    kernel, under both lane layouts (SK_DTW_NO_SMALL: motifs of up to 256 points stay at 16 lanes, R up to 16; unset:
    32 points and more spread over 64 lanes).  Every record equals (a) the reference composition and (b), field for
    field, what the first-match entry point returns for the same windows -- the same kernel in another mode (int16:
    motifseq_multi_batch on region_rows; float64: motifseq_multi_ragged_f64 on the sliced reads)."""
    from squigglekit_amd import api
    if no_small:
        monkeypatch.setenv("SK_DTW_NO_SMALL", "1")
    motifs, reads, refs = seams
    mean, sd = model_terms(motifs)
    if route == "int16":
        sig, lens = api.pack_i16(reads[route])
        got = api.motifseq_panel_batch(sig, lens, motifs, mean, sd, region=SEAM_REGION, records=True)
        rows, wlen, frm = api.region_rows(sig, lens, SEAM_REGION)
        first = api.motifseq_multi_batch(rows, wlen, motifs)
        assert np.array_equal(frm, got[1])
    else:
        got = api.motifseq_panel_ragged_f64(*api.pack_f64(reads[route]), motifs, mean, sd, region=SEAM_REGION, records=True)
        first = api.motifseq_multi_ragged_f64(*api.pack_f64([x[slice(*SEAM_REGION)] for x in reads[route]]), motifs)
    same(got, refs[route], (route, no_small))
    assert len(got[2]) == len(first) == len(SEAM_POINTS)
    for k, (g, f) in enumerate(zip(got[2], first)):
        tag = (route, no_small, SEAM_POINTS[k])
        nan = np.isnan(g["dist"])
        assert np.array_equal(nan, np.isnan(f["dist"])) and np.array_equal(bits(g["dist"][~nan]), bits(f["dist"][~nan])), tag
        for field in ("start", "end", "n", "flags"):
            assert np.array_equal(g[field], f[field]), (tag, field)
