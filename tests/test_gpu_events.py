"""MotifSeq events and pooled models on the GPU (sk_motifseq_events_*, sk_events_pool*, api.motifseq_events*,
api.pool_events, api.refine_motif, MotifSeq --pool): every record equals the numpy statement of the contract in
test_events_host.py byte for byte (tobytes(): no tolerance anywhere), the hit records are the hit-list call's, the
spans the paths call's, and the kernel's self-check counts nothing."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLD
from test_cli import run_cli, scrappy_stub, tsv_files          # noqa: F401  (fixtures)
from test_events_host import (cached_batch, dba_input, reference_pool, reference_round, synthetic_events)

pytestmark = pytest.mark.gpu
MODEL = os.path.join(GOLD, "CATCTATCCAGGGTTAAATT.model")
# motif size -> seed of event_reads: chosen so that the reference meets check_input_conditions (the stalled point of
# the plateau read is part of a hit)
SEEDS = {1: 1, 25: 15, 64: 11, 65: 4, 200: 3, 500: 500, 1100: 1100}


def same(got, paths, events, tag=""):
    """got = (hits[R, K], count[R], events[R, K, N]) against the reference's paths and events."""
    from squigglekit_amd import api
    assert api.last_path_mismatches() == 0, tag
    hits, count, ev = got
    assert ev.dtype == api.EVENT_DTYPE and ev.shape == events.shape, tag
    for r, w in enumerate(paths):
        if w is None:                                                            # flagged: NaN, -1, 0
            assert count[r] == 0 and hits[r, 0]["flags"] & 3, (tag, r)
        else:
            assert count[r] == len(w), (tag, r)
            for k, ((dist, start, end), _) in enumerate(w):
                assert (int(hits[r, k]["start"]), int(hits[r, k]["end"])) == (start, end), (tag, r, k)
                assert np.float64(hits[r, k]["dist"]).tobytes() == np.float64(dist).tobytes(), (tag, r, k)
        for k in range(ev.shape[1]):
            if ev[r, k].tobytes() != events[r, k].tobytes():
                bad = [i for i in range(ev.shape[2]) if ev[r, k, i].tobytes() != events[r, k, i].tobytes()]
                raise AssertionError((tag, r, k, bad[:5], ev[r, k, bad[0]], events[r, k, bad[0]]))
    assert ev.tobytes() == events.tobytes(), tag


# ---- events against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", ["medmad", "zscale"])
@pytest.mark.parametrize("K", [1, 3])
def test_int16_route_matches_the_reference(gpu, K, scale):
    from squigglekit_amd import api
    motif, reads, paths, events = cached_batch(200, SEEDS[200], K, scale, "i16")
    got = api.motifseq_events(reads, [motif], K, scale=scale)
    same(got[0], paths, events, "int16 %s K=%d" % (scale, K))
    plain = api.motifseq_hits(reads, [motif], K, scale=scale)[0]                 # hits and counts: the hit-list call's
    assert got[0][0].tobytes() == plain[0].tobytes() and got[0][1].tobytes() == plain[1].tobytes()
    sp = api.motifseq_paths(reads, [motif], K, scale=scale)[0][2]                # spans: the paths call's
    assert np.array_equal(api.spans_of_events(got[0][2]), sp)


@pytest.mark.parametrize("scale", ["medmad", "zscale"])
@pytest.mark.parametrize("K", [1, 3])
def test_float64_pa_and_centi_routes_match_the_reference(gpu, K, scale):
    from squigglekit_amd import api
    motif, reads, paths, events = cached_batch(200, SEEDS[200], K, scale, "pa")
    got = api.motifseq_events(reads, [motif], K, scale=scale)
    same(got[0], paths, events, "pA %s K=%d" % (scale, K))
    flat, off = api.pack_f64(reads)
    centi = np.round(flat * 100).astype(np.int32)                                # centi-units, as the TSV tokenizer gives
    got = api.motifseq_events_ragged_f64(centi, off, [motif], K, scale=scale)
    same(got[0], paths, events, "centi %s K=%d" % (scale, K))
    plain = api.motifseq_hits_ragged_f64(centi, off, [motif], K, scale=scale)[0]
    assert got[0][0].tobytes() == plain[0].tobytes() and got[0][1].tobytes() == plain[1].tobytes()


@pytest.mark.parametrize("N", [1, 25, 64, 65, 200, 500, 1100])
def test_motif_sizes_across_stripe_edges_and_the_chained_pass(gpu, N):
    from squigglekit_amd import api
    motif, reads, paths, events = cached_batch(N, SEEDS[N], 3, "medmad", "i16")
    got = api.motifseq_events(reads, [motif], 3)
    same(got[0], paths, events, "N=%d" % N)
    assert np.array_equal(api.spans_of_events(got[0][2]), api.motifseq_paths(reads, [motif], 3)[0][2])


def test_both_path_tiers_and_two_motifs_in_one_call(gpu, monkeypatch):
    from squigglekit_amd import api
    m1, reads, paths, events = cached_batch(200, SEEDS[200], 3, "medmad", "i16")
    widths = [h[2] - h[1] + 1 for w in paths if w for h, _ in w]
    assert min(widths) <= 400 and max(widths) > 512                              # one hit fits the LDS tier, one does not
    m2, _, paths2, events2 = cached_batch(64, SEEDS[64], 3, "medmad", "i16")
    from test_events_host import reference_batch
    from oracle import oracle as ora
    paths2, events2 = reference_batch(ora, reads, m2, 3)                         # the 64-point motif on THESE reads
    got = api.motifseq_events(reads, [m1, m2], 3)
    same(got[0], paths, events, "first motif")
    same(got[1], paths2, events2, "second motif")
    monkeypatch.setenv("SK_PATH_LDS_BYTES", "0")                                 # every hit through the scratch tier
    scr = api.motifseq_events(reads, [m1], 3)
    same(scr[0], paths, events, "scratch tier")


def test_a_window_wider_than_the_lds_columns(gpu, ora):
    from squigglekit_amd import api
    from test_events_host import reference_batch
    from test_gpu_paths import plateau_read
    from test_hits_host import normalised
    raw = plateau_read(1500)                                                     # PATH_LDS_COLS is 1 024
    y = normalised(ora, raw, "medmad", 0, 32768)
    motif = np.array([y[0], y[1], y[-1]])
    paths, events = reference_batch(ora, [raw], motif, 1, lo=0, hi=32768)
    assert events[0, 0, 1]["dwell"] > 1024
    got = api.motifseq_events([raw], [motif], 1, scale_low=0, scale_hi=32768)
    same(got[0], paths, events, "wide window")


def test_device_resident_entry(gpu):
    from squigglekit_amd import api
    from squigglekit_amd._lib import ptr
    L = gpu.load()
    motif, reads, paths, events = cached_batch(200, SEEDS[200], 3, "medmad", "i16")
    buf, lens = api.pack_i16(reads)
    R, K, N = len(reads), 3, motif.size
    moff = np.array([0, N], dtype=np.int32)
    sizes = [buf.nbytes, lens.nbytes, R * K * 24, R * 4, R * K * N * 32]
    d = [L.sk_dev_alloc(s) for s in sizes]
    try:
        assert all(d)
        assert L.sk_dev_upload(d[0], ptr(buf), buf.nbytes) == 0 and L.sk_dev_upload(d[1], ptr(lens), lens.nbytes) == 0
        rc = L.sk_motifseq_events_dev_i16(d[0], buf.shape[1], d[1], R, ptr(motif), ptr(moff), 1, 0, 0, 1200, K,
                                          float("inf"), d[2], d[3], d[4])
        assert rc == 0, L.sk_last_error()
        ev = np.zeros((R, K, N), dtype=api.EVENT_DTYPE)
        assert L.sk_dev_download(ptr(ev), d[4], ev.nbytes) == 0
        assert L.sk_last_path_mismatches() == 0
        assert ev.tobytes() == events.tobytes()
        # the events stay on the device: pooled there, the same as pooled from the host
        d_pool = L.sk_dev_alloc(N * 56)
        try:
            assert L.sk_events_pool_dev(d[4], None, R * K, N, d_pool) == 0, L.sk_last_error()
            pool = np.zeros(N, dtype=api.POOL_DTYPE)
            assert L.sk_dev_download(ptr(pool), d_pool, pool.nbytes) == 0
            # ... and with a mask that lies on the device too: every third hit
            third = (np.arange(R * K) % 3 == 0).astype(np.uint8)
            d_use = L.sk_dev_alloc(third.nbytes)
            try:
                assert d_use and L.sk_dev_upload(d_use, ptr(third), third.nbytes) == 0
                assert L.sk_events_pool_dev(d[4], d_use, R * K, N, d_pool) == 0, L.sk_last_error()
                masked = np.zeros(N, dtype=api.POOL_DTYPE)
                assert L.sk_dev_download(ptr(masked), d_pool, masked.nbytes) == 0
            finally:
                L.sk_dev_free(d_use)
        finally:
            L.sk_dev_free(d_pool)
        assert pool.tobytes() == api.pool_events(ev).tobytes() == pool_bytes(reference_pool(events))
        assert 0 < masked["hits"][0] < pool["hits"][0]
        assert masked.tobytes() == api.pool_events(ev, third).tobytes() == pool_bytes(reference_pool(events, third))
    finally:
        for p in d:
            L.sk_dev_free(p)


# ---- pool against the reference -----------------------------------------------------------------------------------------------
def pool_bytes(ref):
    """reference_pool's records as the bytes of POOL_DTYPE (pad 0)."""
    from squigglekit_amd import api
    out = np.zeros(ref.size, dtype=api.POOL_DTYPE)
    for f in api.POOL_DTYPE.names:
        out[f] = ref[f]
    return out.tobytes()


@pytest.mark.parametrize("H", [1, 7, 8, 9, 127, 128, 129, 8191, 8192, 8193, 20000])
def test_pool_matches_the_reference(gpu, H):
    from squigglekit_amd import api
    for N in (1, 63, 64, 65, 200):
        ev = synthetic_events(H, N, 1000 * N + H)
        third = np.arange(H) % 3 == 0
        for tag, use in (("all", None), ("none", np.zeros(H, bool)), ("third", third)):
            got = api.pool_events(ev, use)
            assert got.dtype == api.POOL_DTYPE and got.shape == (N,)
            assert got.tobytes() == pool_bytes(reference_pool(ev, use)), (H, N, tag)
    alive = synthetic_events(H, 3, H, dead_every=0)                               # no hit without a path
    assert api.pool_events(alive).tobytes() == pool_bytes(reference_pool(alive))
    assert np.all(api.pool_events(alive)["hits"] == H)


def test_pool_does_not_depend_on_the_split_of_the_events_call(gpu):
    from squigglekit_amd import api
    motif, reads, paths, events = cached_batch(200, SEEDS[200], 3, "medmad", "i16")
    whole = api.motifseq_events(reads, [motif], 3)[0][2]
    buf, lens = api.pack_i16(reads)
    parts = [api.motifseq_events_batch(buf[lo:hi], lens[lo:hi], [motif], 3)[0][2] for lo, hi in ((0, 5), (5, 6), (6, 24))]
    split = np.concatenate(parts)
    assert split.tobytes() == whole.tobytes()
    # `devices=`: two GPUs where the machine has them; on a single GPU this is one shard and the three-part split above
    # alone carries the check
    ndev = gpu.load().sk_device_count()
    shard = api.motifseq_events(reads, [motif], 3, devices=list(range(min(ndev, 2))))[0][2]
    assert shard.tobytes() == whole.tobytes()
    want = pool_bytes(reference_pool(events))
    assert api.pool_events(whole).tobytes() == api.pool_events(split).tobytes() == api.pool_events(shard).tobytes() == want


# ---- refinement ------------------------------------------------------------------------------------------------------------------
def test_refine_motif_is_the_explicit_loop_and_its_first_round_the_reference_round(gpu, ora):
    from squigglekit_amd import api
    truth, search, reads = dba_input()
    cut = 60.0
    rounds = api.refine_motif(reads, search, rounds=2, max_hits=2, max_dist=cut)
    x = search.copy()
    for t in range(2):
        hits, _, ev = api.motifseq_events(reads, [x], 2)[0]
        pool = api.pool_events(ev, hits["dist"] <= cut)
        x = np.where(pool["hits"] > 0, pool["level"], x)
        assert rounds[t][0].tobytes() == x.tobytes() and rounds[t][1].tobytes() == pool.tobytes(), t
    first = api.refine_motif(reads, search)                                      # rounds=1, max_hits=1, no limit
    x1, pool1 = reference_round(ora, reads, search)
    assert len(first) == 1 and first[0][0].tobytes() == x1.tobytes() and first[0][1].tobytes() == pool_bytes(pool1)
    assert np.mean(np.abs(first[0][0] - truth)) < np.mean(np.abs(search - truth))


# ---- MotifSeq --pool ---------------------------------------------------------------------------------------------------------------
def predicted_pool_table(stdout, reads_of, model_path, K):
    """The --pool table for the hit lines of `stdout`: pool_events over the events of exactly those hits, in line order."""
    from squigglekit_amd import api, tsvio
    models, order, _, bases = tsvio.read_scrappie_model_bases(model_path)
    lines = ["model\tpoint\tpos\tbase\tmodel_current\thits\tlevel\tlevel_sd\tsd_mean\tdwell_mean\tdwell_sd\tcost_mean"]
    printed = {name: [] for name in order}
    cache = {}
    for ln in stdout.split("\n")[1:-1]:
        f = ln.split("\t")
        rid, name, start, end = f[1], f[2], int(f[3]), int(f[4])
        if (rid, name) not in cache:
            cache[rid, name] = api.motifseq_events([reads_of[rid]], [np.array(models[name])], K)[0]
        hits, count, ev = cache[rid, name]
        k = [q for q in range(count[0]) if (hits[0, q]["start"], hits[0, q]["end"]) == (start, end)]
        assert len(k) == 1
        printed[name].append(ev[0, k[0]])
    for name in order:
        pool = api.pool_events(np.stack(printed[name]))
        where = {i: (pos, base) for pos, base, _, first, cnt in bases[name] for i in range(first, first + cnt)}
        for i, rec in enumerate(pool):
            row = (name, i) + where[i] + (float(models[name][i]), int(rec["hits"])) + tuple(
                float(rec[f]) for f in ("level", "level_sd", "sd_mean", "dwell_mean", "dwell_sd", "cost_mean"))
            lines.append("\t".join("{}".format(v) for v in row))
    return "\n".join(lines) + "\n", {name: len(v) for name, v in printed.items()}


@pytest.mark.parametrize("extra", [[], ["--hits", "3", "--min_hit_p"]])
def test_cli_pool_table_and_unchanged_stdout(gpu, scrappy_stub, tsv_files, tmp_path, extra):  # noqa: F811
    from squigglekit_amd.motifseq_cli import main
    for kind in ("m_real_raw", "m_synthetic6"):
        argv = ["-s", tsv_files[kind], "-m", MODEL] + extra
        if extra:                                                                # P: the median hit_Probability of --hits 3
            hp = [float(ln.split("\t")[11]) for ln in run_cli(main, argv[:-1])[0].split("\n")[1:-1]]
            argv.append(repr(float(np.median(hp))))
            assert min(hp) < float(np.median(hp)) or len(hp) == 1                # (some line is left out)
        want = run_cli(main, argv)
        assert want[2] == 0
        table = tmp_path / ("pool_%s_%d.tsv" % (kind, len(extra)))
        got = run_cli(main, argv + ["--pool", str(table)])
        assert got[0] == want[0] and got[2] == 0, argv                          # stdout byte for byte
        reads_of = {}
        for ln in open(tsv_files[kind]):
            f = ln.rstrip("\n").split("\t")
            reads_of[f[1]] = np.array([int(v) for v in f[8:]])
        nlines = len(want[0].split("\n")) - 2
        assert nlines >= 1, argv
        text, npooled = predicted_pool_table(want[0], reads_of, MODEL, 3 if extra else 1)
        assert sum(npooled.values()) == nlines                                   # only the printed lines are pooled
        assert open(table).read() == text, argv
        # --paths beside --pool: its file is the one --paths writes alone
        alone, both = tmp_path / "alone.tsv", tmp_path / "both.tsv"
        assert run_cli(main, argv + ["--paths", str(alone)])[0] == want[0]
        assert run_cli(main, argv + ["--paths", str(both), "--pool", str(table)])[0] == want[0]
        assert open(both).read() == open(alone).read() and open(table).read() == text


@pytest.mark.parametrize("bad", [["--panel"], ["--after_stall"]])
def test_cli_refusals_exit_with_status_2(gpu, tsv_files, tmp_path, bad):  # noqa: F811
    from squigglekit_amd.motifseq_cli import main
    out = run_cli(main, ["-s", tsv_files["m_real_raw"], "-m", MODEL, "--pool", str(tmp_path / "p.tsv")] + bad)
    assert out[2] == 2 and not (tmp_path / "p.tsv").exists()
