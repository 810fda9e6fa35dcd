"""MotifSeq alignment paths on the GPU (sk_motifseq_paths_*, api.motifseq_paths*, dtw_subsequence(full_path=True),
MotifSeq --paths): the spans equal the numpy statement of the contract in test_paths_host.py as integers, the records
are the hit-list call's byte for byte, and the kernel's self-check counts nothing."""
import os

import numpy as np
import pytest

from conftest import GOLD
from test_cli import run_cli, scrappy_stub, tsv_files          # noqa: F401  (fixtures)
from test_gpu_hits import mixed_reads
from test_paths_host import check_spans_shape, full_cost, reference_paths, spans_of, trace

pytestmark = pytest.mark.gpu
MODEL = os.path.join(GOLD, "CATCTATCCAGGGTTAAATT.model")


def same(got, want, tag=""):
    """got = (hits[R, K], count[R], spans[R, K, N, 2]) against reference_paths' lists.  Every hit of every read is
    compared; a read without a path (None: empty after the filter, or MAD = 0) must be flagged and carry spans -1."""
    from squigglekit_amd import api
    assert api.last_path_mismatches() == 0, tag
    hits, count, spans = got
    nopath = 0
    for r, w in enumerate(want):
        if w is None:
            nopath += 1
            assert count[r] == 0 and hits[r, 0]["flags"] & 3 and np.all(spans[r] == -1), (tag, r)
            continue
        assert count[r] == len(w), (tag, r, count[r], len(w))
        for k, ((dist, start, end), sp) in enumerate(w):
            h = hits[r, k]
            assert (int(h["start"]), int(h["end"])) == (start, end), (tag, r, k)
            assert np.float64(h["dist"]).tobytes() == np.float64(dist).tobytes(), (tag, r, k)
            assert spans[r, k].dtype == np.int32 and np.array_equal(spans[r, k], sp), (tag, r, k, spans[r, k][:6], sp[:6])
        assert np.all(spans[r, count[r]:] == -1), (tag, r)
    assert nopath <= 2, tag


def same_as_hit_lists(got, plain):
    for (h, c, _), (h0, c0) in zip(got, plain):
        assert h.tobytes() == h0.tobytes() and c.tobytes() == c0.tobytes()


@pytest.mark.parametrize("N", [1, 16, 17, 64, 65, 200, 1024, 1025])
def test_int16_medmad_matches_the_contract(gpu, ora, N):
    from squigglekit_amd import api
    motif, reads = mixed_reads(N, N)
    for K in (1, 3, 8):
        got = api.motifseq_paths(reads, [motif], K)
        same(got[0], reference_paths(ora, reads, motif, K), "N=%d K=%d" % (N, K))
        same_as_hit_lists(got, api.motifseq_hits(reads, [motif], K))


@pytest.mark.parametrize("N", [17, 200])
def test_batch_lane_layout_matches_the_contract(gpu, ora, monkeypatch, N):
    from squigglekit_amd import api
    monkeypatch.setenv("SK_DTW_SMALL_MAX", "0")                              # four reads per wavefront, as big batches
    motif, reads = mixed_reads(N, 3 * N)
    got = api.motifseq_paths(reads, [motif], 3)
    same(got[0], reference_paths(ora, reads, motif, 3), "L16")
    same_as_hit_lists(got, api.motifseq_hits(reads, [motif], 3))


def test_zscale_float64_pa_and_centi_match_the_contract(gpu, ora):
    from squigglekit_amd import api
    motif, reads = mixed_reads(200, 5)
    for K in (1, 3):
        same(api.motifseq_paths(reads, [motif], K, scale="zscale")[0],
             reference_paths(ora, reads, motif, K, scale="zscale"), "zscale")
    pa = [np.round((r.astype(np.int64) + 16.0) * (1493.94 / 8192.0), 2) for r in reads[1:]]
    for scale in ("medmad", "zscale"):
        got = api.motifseq_paths(pa, [motif], 3, scale=scale)
        same(got[0], reference_paths(ora, pa, motif, 3, scale=scale), "pA " + scale)
        same_as_hit_lists(got, api.motifseq_hits(pa, [motif], 3, scale=scale))
    flat, off = api.pack_f64(pa)
    centi = np.round(flat * 100).astype(np.int32)                              # centi-units, as the TSV tokenizer gives
    got = api.motifseq_paths_ragged_f64(centi, off, [motif], 8)
    same(got[0], reference_paths(ora, pa, motif, 8), "centi")
    same_as_hit_lists(got, api.motifseq_hits_ragged_f64(centi, off, [motif], 8))


def test_two_motifs_share_one_call(gpu, ora):
    from squigglekit_amd import api, synth
    m1, reads = mixed_reads(65, 21)
    m2 = synth.synthetic_motif(30, seed=2)
    got = api.motifseq_paths(reads, [m1, m2], 3)
    same(got[0], reference_paths(ora, reads, m1, 3), "first motif")
    same(got[1], reference_paths(ora, reads, m2, 3), "second motif")
    same_as_hit_lists(got, api.motifseq_hits(reads, [m1, m2], 3))


# ---- both tiers ------------------------------------------------------------------------------------------------------
def test_lds_tier_and_forced_scratch_tier_agree_with_the_contract(gpu, ora, monkeypatch):
    from squigglekit_amd import api
    motif, reads = mixed_reads(200, 77)
    want = reference_paths(ora, reads, motif, 3)
    widths = [h[2] - h[1] + 1 for w in want if w for h, _ in w]
    assert max(widths) <= 512, widths                                         # every window fits the LDS tier's default
    lds = api.motifseq_paths(reads, [motif], 3)
    same(lds[0], want, "LDS tier")
    monkeypatch.setenv("SK_PATH_LDS_BYTES", "0")                              # nothing fits: every hit takes the scratch tier
    scr = api.motifseq_paths(reads, [motif], 3)
    same(scr[0], want, "scratch tier")
    monkeypatch.setenv("SK_PATH_SCRATCH_BYTES", "1000")                       # ... with a single wavefront's slab
    one = api.motifseq_paths(reads, [motif], 3)
    same(one[0], want, "scratch tier, one wavefront")
    assert scr[0][2].tobytes() == lds[0][2].tobytes() == one[0][2].tobytes()


def plateau_read(n_plateau=5200):
    """One isolated high sample, a two-value plateau, one distinct last sample (int16; the limits 0 .. 32768 keep all)."""
    mid = np.where(np.arange(n_plateau) % 2 == 0, 600, 601)
    return np.concatenate([[32767], mid, [12000]]).astype(np.int16)


def test_a_window_wider_than_4096_columns(gpu, ora):
    from squigglekit_amd import api
    from test_hits_host import normalised
    raw = plateau_read()
    y = normalised(ora, raw, "medmad", 0, 32768)
    assert y.size == raw.size and np.all(np.isfinite(y))
    motif = np.array([y[0], y[1], y[-1]])                                     # first sample, plateau, last sample
    opx, opy = ora.dtw_subsequence_path(motif, y)
    assert opy[-1] - opy[0] + 1 > 4096, (opy[0], opy[-1])                     # the reference path is that wide
    want = reference_paths(ora, [raw], motif, 1, lo=0, hi=32768)
    assert np.array_equal(want[0][0][1], spans_of(opx, opy, 3))
    got = api.motifseq_paths([raw], [motif], 1, scale_low=0, scale_hi=32768)
    same(got[0], want, "wide window")
    sp = got[0][2][0, 0]
    assert sp[1, 1] - sp[1, 0] + 1 > 4096                                     # row 1 runs along the whole plateau
    # the same pair through the mlpy boundary
    dist, _, (px, py) = api.dtw_subsequence(motif, y, full_path=True)
    assert api.last_path_mismatches() == 0
    assert np.array_equal(px, opx) and np.array_equal(py, opy)


# ---- the mlpy boundary ---------------------------------------------------------------------------------------------------
def test_single_pair_full_path_on_the_shipped_read(gpu, ora, example_read, example_model):
    from squigglekit_amd import api
    y = api.normalise(example_read["signal"])
    assert y.size == 36977 and example_model.size == 163
    dist, cost, (px, py) = api.dtw_subsequence(example_model, y, full_path=True)
    assert api.last_path_mismatches() == 0
    opx, opy = ora.dtw_subsequence_path(example_model, y)
    assert np.array_equal(px, opx) and np.array_equal(py, opy)
    od = ora.dtw_subsequence(example_model, y)
    assert np.float64(dist).tobytes() == np.float64(od[0]).tobytes() and (py[0], py[-1]) == (od[1], od[2])
    d0, c0, p0 = api.dtw_subsequence(example_model, y)                        # without the keyword: as before
    assert d0 == dist and c0 is None
    assert p0[0].tolist() == [0, 162] and p0[1].tolist() == [od[1], od[2]]


# ---- scale -----------------------------------------------------------------------------------------------------------------
def test_spans_agree_with_the_records_on_a_large_batch(gpu, ora):
    from concurrent.futures import ThreadPoolExecutor
    from squigglekit_amd import api, synth
    from test_hits_host import normalised
    motif = synth.synthetic_motif(200)
    R = 20000
    sig = synth.squiggle_batch(R, 4000, 2024, motif=motif)
    lens = np.full(R, 4000, dtype=np.int32)
    hits, count, spans = api.motifseq_paths_batch(sig, lens, [motif], 1)[0]
    assert api.last_path_mismatches() == 0
    h0, c0 = api.motifseq_hits_batch(sig, lens, [motif], 1)[0]
    assert hits.tobytes() == h0.tobytes() and count.tobytes() == c0.tobytes()
    assert np.all(count == 1)
    sp = spans[:, 0]
    assert np.array_equal(sp[:, 0, 0], hits[:, 0]["start"]) and np.array_equal(sp[:, 0, 1], hits[:, 0]["start"])
    assert np.array_equal(sp[:, -1, 1], hits[:, 0]["end"])
    assert np.all(sp[:, :, 0] <= sp[:, :, 1])
    step = sp[:, 1:, 0] - sp[:, :-1, 1]
    assert np.all((step == 0) | (step == 1))
    rows = list(range(0, R, 37))                                              # 541 reads against the oracle's path
    assert len(rows) >= 500

    def oracle_spans(r):
        px, py = ora.dtw_subsequence_path(motif, normalised(ora, sig[r]))
        return spans_of(px, py, motif.size)
    with ThreadPoolExecutor(16) as ex:
        want = list(ex.map(oracle_spans, rows))
    for r, w in zip(rows, want):
        assert np.array_equal(sp[r], w), r


# ---- MotifSeq --paths --------------------------------------------------------------------------------------------------------
def predicted_table(ora, stdout, sigs, model_path):
    """The --paths table the numpy contract predicts for the hit lines of `stdout` (read id -> normalised signal)."""
    from squigglekit_amd import tsvio
    models, order, _, bases = tsvio.read_scrappie_model_bases(model_path)
    lines = ["fast5\treadID\tmodel\thit\tpos\tbase\tmodel_current\tstart\tend\tlength\tmean_signal"]
    costs = {}
    seen = {}
    for ln in stdout.split("\n")[1:-1]:
        f = ln.split("\t")
        fast5, rid, name, start, end = f[0], f[1], f[2], int(f[3]), int(f[4])
        y = sigs[rid]
        if (rid, name) not in costs:
            costs[rid, name] = full_cost(ora, models[name], y)
        rank = seen[rid, name] = seen.get((rid, name), 0) + 1
        px, py = trace(costs[rid, name], end)
        assert py[0] == start
        sp = spans_of(px, py, len(models[name]))
        for pos, base, current, first, cnt in bases[name]:
            if cnt == 0:
                a, b, length, mean = -1, -1, 0, float("nan")
            else:
                a, b = int(sp[first, 0]), int(sp[first + cnt - 1, 1])
                length, mean = b - a + 1, np.mean(y[a:b + 1])
            lines.append("\t".join(str(v) for v in (fast5, rid, name, rank, pos, base, current, a, b, length))
                         + "\t{}".format(mean))
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("extra", [[], ["--hits", "3"]])
def test_cli_paths_table_and_unchanged_stdout(gpu, ora, scrappy_stub, tsv_files, tmp_path, extra):  # noqa: F811
    from squigglekit_amd import api, blow5, tsvio
    from squigglekit_amd.motifseq_cli import main
    inputs = {"tsv": ["-s", tsv_files["m_real_raw"]], "syn": ["-s", tsv_files["m_synthetic6"]],
              "blow5": ["--blow5", os.path.join(GOLD, "example_0.blow5")]}
    for kind, inp in inputs.items():
        argv = inp + ["-m", MODEL] + extra
        want = run_cli(main, argv)
        assert want[2] == 0
        table = tmp_path / ("paths_%s_%d.tsv" % (kind, len(extra)))
        got = run_cli(main, argv + ["--paths", str(table)])
        assert got[0] == want[0] and got[2] == 0, argv                          # stdout byte for byte
        if kind == "blow5":
            sigs = {rec["read_id"]: api.normalise(rec["signal"]) for rec in blow5.read_blow5(inp[1])}
        else:
            sigs = {}
            for ln in open(inp[1]):
                f = ln.rstrip("\n").split("\t")
                sigs[f[1]] = api.normalise(np.array([int(v) for v in f[8:]]))
        assert len(got[0].split("\n")) > 2, argv                                # some hit was printed
        assert open(table).read() == predicted_table(ora, want[0], sigs, MODEL), argv
