"""MotifSeq read background on the GPU (sk_motifseq_background_*, api.motifseq_background*, MotifSeq --background):
every record bit for bit numpy on the oracle's last row (test_background_host.reference_background), the hit lists
those of the hit-list twin, the CLI's file.

Conditions on the inputs: a comparison skips only reads the reference itself flags, and in every batch at least 90 % of
the reads are unflagged with reference std > 0 and mad > 0 -- asserted from the reference alone (check_inputs) before
any GPU output is looked at.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import GOLD
from test_cli import run_cli, scrappy_stub, tsv_files          # noqa: F401  (fixtures)
from test_background_host import reference_background, usable
from test_hits_host import normalised

pytestmark = pytest.mark.gpu
MODEL = os.path.join(GOLD, "CATCTATCCAGGGTTAAATT.model")


def reference_records(ora, reads, motif, scale="medmad"):
    """reference_background per raw read (None: flagged by the reference), reads spread over host threads."""
    def one(raw):
        y = normalised(ora, raw, scale)
        return reference_background(motif, y) if y.size and np.all(np.isfinite(y)) else None
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(one, reads))


def check_inputs(want):
    assert usable(want) >= 0.9, "fewer than 90 %% of the reads are usable: %.3f" % usable(want)


def same(bg, want, flags=None, tag=""):
    """bg [R] BG_DTYPE against the reference's records, bit for bit; flagged reads: NaN fields, below -1."""
    assert len(bg) == len(want)
    for r, w in enumerate(want):
        g = bg[r]
        if w is None:
            assert all(np.isnan(g[f]) for f in ("mean", "std", "median", "mad")) and g["below"] == -1, (tag, r)
            if flags is not None:
                assert flags[r] & 3, (tag, r)
            continue
        for i, f in enumerate(("mean", "std", "median", "mad")):
            assert np.float64(g[f]).tobytes() == np.float64(w[i]).tobytes(), (tag, r, f, float(g[f]), w[i])
        assert (int(g["below"]), int(g["n"])) == (w[4], w[5]), (tag, r, int(g["below"]), int(g["n"]), w[4:])


def mixed_batch(R, seed, motif, M=4000):
    """R int16 reads of about M samples (a seeded mix: most carry the motif, lengths vary, a few are tie-heavy or
    flagged: nothing survives the filter, MAD 0)."""
    from squigglekit_amd import synth
    rng = np.random.default_rng(seed)
    base = synth.squiggle_batch(R, M, 7000 + seed, motif=motif)
    reads = []
    for r in range(R):
        n = M if r % 3 else int(rng.integers(M // 2, M + 1))
        reads.append(base[r, :n])
    for r in range(0, R, 41):
        reads[r] = (480 + 10 * rng.integers(0, 4, size=M)).astype(np.int16)     # ties everywhere
    for r in range(17, R, 97):
        reads[r] = np.full(40, 2000, dtype=np.int16)                            # nothing survives scale_outliers
    for r in range(29, R, 113):
        reads[r] = np.full(900, 500, dtype=np.int16)                            # MAD 0
    return reads


def to_pa(reads):
    return [np.round((r.astype(np.int64) + 16.0) * (1493.94 / 8192.0), 2) for r in reads]


@pytest.mark.parametrize("R", [300, 2400])
def test_int16_routes_match_numpy_on_the_last_row(gpu, ora, example_model, R):
    from squigglekit_amd import api
    reads = mixed_batch(R, R, example_model)
    for scale in ("medmad", "zscale"):
        want = reference_records(ora, reads, example_model, scale)
        check_inputs(want)
        hits, count, bg = api.motifseq_background(reads, [example_model], 1, scale=scale)[0]
        same(bg, want, hits[:, 0]["flags"], "%s R=%d" % (scale, R))


def test_float64_pa_and_centi_routes_match(gpu, ora, example_model):
    from squigglekit_amd import api
    reads = [r for r in mixed_batch(300, 5, example_model) if len(r) > 40]
    pa = to_pa(reads)
    for scale in ("medmad", "zscale"):
        want = reference_records(ora, pa, example_model, scale)
        check_inputs(want)
        same(api.motifseq_background(pa, [example_model], 2, scale=scale)[0][2], want, None, "pA " + scale)
    flat, off = api.pack_f64(pa)
    centi = np.round(flat * 100).astype(np.int32)
    want = reference_records(ora, pa, example_model)
    check_inputs(want)
    same(api.motifseq_background_ragged_f64(centi, off, [example_model], 2)[0][2], want, None, "centi")


def test_motifs_of_several_lengths(gpu, ora):
    from squigglekit_amd import api, synth
    motifs = [synth.synthetic_motif(N, seed=N) for N in (25, 200, 500, 1100)]           # 1 100: the chained pass
    reads = mixed_batch(48, 9, motifs[1])
    res = api.motifseq_background(reads, motifs, 3)
    for m, (_, _, bg) in zip(motifs, res):
        want = reference_records(ora, reads, m)
        check_inputs(want)
        same(bg, want, None, "N=%d" % m.size)


def test_row_lengths_in_lds_and_in_global_memory(gpu, ora, example_read):
    from squigglekit_amd import api, synth
    motif = synth.synthetic_motif(40, seed=8)
    lengths = [1, 2, 7, 8, 9, 63, 64, 65, 128, 129, 4096, 4097, 8147, 8192, 8193, 20000]   # (8 147: a tree of seven levels)
    base = np.clip(synth.squiggle_batch(len(lengths), 20000, 4321, motif=motif), 1, 1199)   # (the filter keeps every sample)
    reads = [base[i, :n] for i, n in enumerate(lengths)]
    real = np.asarray(example_read["signal"])
    for scale in ("medmad", "zscale"):               # (medmad flags the one-sample read; zscale gives it std = mad = 0)
        for batch, tag in ((reads, "rows in LDS"), (reads + [real], "rows in global memory")):
            want = reference_records(ora, batch, motif, scale)
            check_inputs(want)
            assert [w[5] for w in want[:len(lengths)] if w is not None] == [n for n, w in zip(lengths, want) if w is not None]
            assert len(batch) == len(lengths) or want[-1][5] == 36977       # the real read's columns after the filter
            same(api.motifseq_background(batch, [motif], 1, scale=scale)[0][2], want, None, tag + " " + scale)


@pytest.mark.parametrize("K", [1, 8])
def test_hit_list_twin(gpu, K):
    from squigglekit_amd import api, synth
    motif = synth.synthetic_motif(120, seed=3)
    sig = synth.squiggle_batch(257, 3000, 99, motif=motif)
    lens = np.full(257, 3000, dtype=np.int32)
    lens[::7] = 1777
    m2 = synth.synthetic_motif(60, seed=4)
    twin = api.motifseq_hits_batch(sig, lens, [motif, m2], K)
    got = api.motifseq_background_batch(sig, lens, [motif, m2], K)
    for (h, c), (h2, c2, bg) in zip(twin, got):
        assert h.tobytes() == h2.tobytes() and np.array_equal(c, c2)
        assert np.array_equal(bg["n"], h[:, 0]["n"]) and np.all(bg["n"] > lens - 50) and np.all(bg["std"] > 0)
    pa = to_pa([sig[r, :lens[r]] for r in range(40)])
    for (h, c), (h2, c2, _) in zip(api.motifseq_hits(pa, [motif], K), api.motifseq_background(pa, [motif], K)):
        assert h.tobytes() == h2.tobytes() and np.array_equal(c, c2)


def test_many_row_chunks_give_the_same_records(gpu, ora, monkeypatch):
    from squigglekit_amd import api, synth
    m2, motif = synth.synthetic_motif(90, seed=3), synth.synthetic_motif(30, seed=2)
    sig = synth.squiggle_batch(9, 4000, 66, motif=m2)
    lens = np.full(9, 4000, dtype=np.int32)
    lens[4] = 1234
    want = reference_records(ora, [sig[r, :lens[r]] for r in range(9)], m2)
    check_inputs(want)
    one = api.motifseq_background_batch(sig, lens, [m2, motif], 5)
    monkeypatch.setenv("SK_HITS_ROW_BYTES", "100000")                          # two reads per chunk: five chunks
    many = api.motifseq_background_batch(sig, lens, [m2, motif], 5)
    for a, b in zip(one, many):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    same(many[0][2], want, None, "chunks")


def test_flagged_reads_have_nan_records(gpu):
    from squigglekit_amd import _lib, api, synth
    motif = synth.synthetic_motif(40)
    sig = synth.squiggle_batch(4, 1000, 9, motif=motif)
    sig[1] = 500                                                               # MAD 0
    sig[2] = 3000                                                              # all outliers
    hits, count, bg = api.motifseq_background_batch(sig, np.full(4, 1000, dtype=np.int32), [motif], 4)[0]
    assert hits[1, 0]["flags"] & _lib.SK_FLAG_DEGENERATE and hits[2, 0]["flags"] & _lib.SK_FLAG_EMPTY
    for r in (1, 2):
        assert count[r] == 0 and bg[r]["below"] == -1 and bg[r]["n"] == hits[r, 0]["n"]
        assert all(np.isnan(bg[r][f]) for f in ("mean", "std", "median", "mad"))
    for r in (0, 3):
        assert bg[r]["below"] >= 0 and 900 < bg[r]["n"] == hits[r, 0]["n"] and np.isfinite(bg[r]["mad"])


def test_two_ranks_on_one_device_equal_one(gpu, monkeypatch):
    from squigglekit_amd import api, multigpu, synth
    monkeypatch.setenv("SK_OVERSUBSCRIBE", "1")
    multigpu.close_groups()
    motif = synth.synthetic_motif(150, seed=4)
    sig = synth.squiggle_batch(301, 3000, 97531, motif=motif)
    lens = np.full(301, 3000, dtype=np.int32)
    lens[::5] = 2222
    plain = api.motifseq_background_batch(sig, lens, [motif], 6)[0]
    got = api.motifseq_background_batch(sig, lens, [motif], 6, devices=[0, 0])[0]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, got))
    assert np.all(plain[2]["std"] > 0)


def test_null_bg_is_invalid(gpu):
    from squigglekit_amd import _lib
    L = _lib.load()
    sig = np.full((1, 64), 500, dtype=np.int16)
    lens = np.array([64], dtype=np.int32)
    motif, moff = np.zeros(4), np.array([0, 4], dtype=np.int32)
    hits, cnt = np.zeros(1, dtype=_lib.HIT_DTYPE), np.zeros(1, dtype=np.int32)
    rc = L.sk_motifseq_background_i16(_lib.ptr(sig), 64, _lib.ptr(lens), 1, _lib.ptr(motif), _lib.ptr(moff), 1, 0, 0, 1200, 1,
                                      float("inf"), _lib.ptr(hits), _lib.ptr(cnt), None)
    assert rc == _lib.SK_ERR_INVALID


# ---- the command line ----------------------------------------------------------------------------------------------
def predicted_file(ora, stdout, raws, model_path, max_z=None):
    """(the --background file, the stdout lines that stay) from the printed hits and reference_background."""
    from squigglekit_amd import tsvio
    from squigglekit_amd.motifseq_cli import BACKGROUND_HEADER
    models, order, _ = tsvio.read_model_auto(model_path)
    lines = stdout.split("\n")
    out, kept, rank, memo = ["\t".join(BACKGROUND_HEADER)], [lines[0]], {}, {}
    for ln in lines[1:]:
        if not ln:
            continue
        f = ln.split("\t")
        key = (f[1], f[2])
        rank[key] = rank.get(key, 0) + 1
        if key not in memo:
            memo[key] = reference_background(np.asarray(models[f[2]], dtype=np.float64), normalised(ora, raws[f[1]]))
        mean, std, med, mad, below, n = memo[key]
        dist = np.float64(float(f[6]))
        with np.errstate(all="ignore"):
            lz = float((dist - np.float64(mean)) / np.float64(std))
            rz = float((dist - np.float64(med)) / (np.float64(mad) * 1.4826))
        if max_z is not None and lz > max_z:
            continue
        kept.append(ln)
        out.append("\t".join("{}".format(v) for v in (f[0], f[1], f[2], rank[key], float(dist), mean, std, lz, med, mad, rz,
                                                        below, n)))
    return "\n".join(out) + "\n", kept


@pytest.mark.parametrize("extra", [[], ["--hits", "4"], ["--hits", "6", "--min_hit_p", "20"]])
def test_cli_background_file_and_unchanged_stdout(gpu, ora, scrappy_stub, tsv_files, tmp_path, extra):  # noqa: F811
    from squigglekit_amd import blow5
    from squigglekit_amd.motifseq_cli import main
    inputs = {"tsv": ["-s", tsv_files["m_real_raw"]], "syn": ["-s", tsv_files["m_synthetic6"]],
              "blow5": ["--blow5", os.path.join(GOLD, "example_0.blow5")]}
    for kind, inp in inputs.items():
        argv = inp + ["-m", MODEL] + extra
        want = run_cli(main, argv)
        assert want[2] == 0
        table = tmp_path / ("bg_%s_%d.tsv" % (kind, len(extra)))
        got = run_cli(main, argv + ["--background", str(table)])
        assert got[0] == want[0] and got[2] == 0, argv                          # stdout byte for byte
        if kind == "blow5":
            raws = {rec["read_id"]: rec["signal"] for rec in blow5.read_blow5(inp[1])}
        else:
            raws = {}
            for ln in open(inp[1]):
                f = ln.rstrip("\n").split("\t")
                raws[f[1]] = np.array([int(v) for v in f[8:]])
        assert len(got[0].split("\n")) > 2, argv                                # some hit was printed
        text, _ = predicted_file(ora, want[0], raws, MODEL)
        assert open(table).read() == text, argv
        if kind == "syn" and extra:
            # --max_local_Z: a threshold between the printed scores, so that some lines go and some stay
            zs = sorted(float(ln.split("\t")[7]) for ln in text.split("\n")[1:] if ln)
            cut = (zs[len(zs) // 2 - 1] + zs[len(zs) // 2]) / 2
            text2, kept = predicted_file(ora, want[0], raws, MODEL, cut)
            assert 1 < len(kept) < len(want[0].split("\n")) - 1
            got2 = run_cli(main, argv + ["--background", str(table), "--max_local_Z=" + repr(cut)])
            assert got2[2] == 0 and got2[0] == "\n".join(kept) + "\n" and open(table).read() == text2, argv


# ---- seeded random cases -------------------------------------------------------------------------------------------
def random_case(seed):
    """A seeded case of its own: motif length, read count and lengths, scale, K and route all drawn from the seed."""
    from squigglekit_amd import synth
    rng = np.random.default_rng(seed)
    N = int(rng.choice([5, 31, 64, 163, 300, 1030]))
    motif = synth.synthetic_motif(N, seed=seed)
    R = int(rng.integers(20, 60))
    M = int(rng.choice([600, 2500, 4096, 9000]))
    base = synth.squiggle_batch(R, M, 31000 + seed, motif=motif)
    reads = [base[r, :int(rng.integers(max(2, M // 3), M + 1))] for r in range(R)]
    if rng.random() < 0.5:
        reads[int(rng.integers(R))] = np.full(50, 2000, dtype=np.int16)
    return dict(motif=motif, reads=reads, scale=str(rng.choice(["medmad", "zscale"])), K=int(rng.choice([1, 2, 8])),
                route=str(rng.choice(["int16", "pA", "centi"])))


@pytest.mark.parametrize("seed", [11, 12, 13, 14, 15, 16, 17, 18])
def test_seeded_random_cases(gpu, ora, seed):
    from squigglekit_amd import api
    c = random_case(seed)
    reads = c["reads"] if c["route"] == "int16" else to_pa(c["reads"])
    want = reference_records(ora, reads, c["motif"], c["scale"])
    check_inputs(want)
    if c["route"] == "centi":
        flat, off = api.pack_f64(reads)
        got = api.motifseq_background_ragged_f64(np.round(flat * 100).astype(np.int32), off, [c["motif"]], c["K"],
                                                 scale=c["scale"])[0]
        twin = api.motifseq_hits_ragged_f64(np.round(flat * 100).astype(np.int32), off, [c["motif"]], c["K"],
                                            scale=c["scale"])[0]
    else:
        got = api.motifseq_background(reads, [c["motif"]], c["K"], scale=c["scale"])[0]
        twin = api.motifseq_hits(reads, [c["motif"]], c["K"], scale=c["scale"])[0]
    same(got[2], want, None, "seed %d %s" % (seed, c["route"]))
    assert got[0].tobytes() == twin[0].tobytes() and np.array_equal(got[1], twin[1])
