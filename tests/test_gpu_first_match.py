"""GPU: what must not move when the host code of the first-match family (sk_motifseq_dev_i16 .. sk_motifseq_dev_f64)
is rearranged: the single-motif entry points against the multi-motif ones with one motif, several motifs over several
sub-batches against the unsplit call and the oracle, api.motifseq_multi on mixed reads against motifseq_any per motif,
and the return code of every entry point for the usual argument mistakes."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
MODES = {"medmad": 0, "zscale": 1}


def _oracle_equal(got, want, label):
    """The comparison of test_fused_zscale_prologue_numpy_order: n everywhere, the record where a sample survived.
    Under medmad a read whose MAD is 0 (one sample, a constant read) is left out as in
    test_motifseq_ragged_and_edge_reads: the reference divides by zero there and the oracle's distance is not finite."""
    ok = (got["n"] > 0) & (np.isfinite(want["dist"]) if "medmad" in label else True)
    assert np.array_equal(got["n"], want["n"]), label
    for f in ("dist", "start", "end"):
        assert np.array_equal(got[f][ok], want[f][ok]), (label, f)


@pytest.fixture(scope="module")
def one_motif(ora):
    """600 reads x stride 1 000, a 40-point motif; lengths from 200 to the stride with the corner lengths planted.
    The oracle's records per scale mode, computed once."""
    from squigglekit_amd import synth
    R, stride = 600, 1000
    motif = synth.synthetic_motif(40, seed=8)
    sig = synth.squiggle_batch(R, stride, 171717, motif=motif)
    lens = np.random.default_rng(17).integers(200, stride + 1, R).astype(np.int32)
    corner = [0, 1, 7, 39, 40, 41, stride]
    lens[:len(corner)] = corner
    want = {s: ora.motifseq_batch_i16(sig, lens, motif, scale_mode=m) for s, m in MODES.items()}
    return sig, lens, motif, want


@pytest.mark.parametrize("scale", list(MODES))
def test_single_equals_multi_of_one_i16_host(gpu, one_motif, scale):
    from squigglekit_amd._lib import HIT_DTYPE, check, ptr
    L = gpu.load()
    sig, lens, motif, want = one_motif
    R, stride = sig.shape
    moff = np.array([0, motif.size], dtype=np.int32)
    single, multi = np.zeros(R, dtype=HIT_DTYPE), np.zeros(R, dtype=HIT_DTYPE)
    check(L.sk_motifseq_batch_i16(ptr(sig), stride, ptr(lens), R, ptr(motif), motif.size, MODES[scale], 0, 1200, ptr(single)))
    check(L.sk_motifseq_multi_batch_i16(ptr(sig), stride, ptr(lens), R, ptr(motif), ptr(moff), 1, MODES[scale], 0, 1200,
                                        ptr(multi)))
    assert single.tobytes() == multi.tobytes()
    _oracle_equal(single, want[scale], "host int16 " + scale)


@pytest.mark.parametrize("scale", list(MODES))
def test_single_equals_multi_of_one_i16_dev(gpu, one_motif, scale):
    from squigglekit_amd._lib import HIT_DTYPE, check, ptr
    L = gpu.load()
    sig, lens, motif, want = one_motif
    R, stride = sig.shape
    moff = np.array([0, motif.size], dtype=np.int32)
    bufs = []

    def alloc(nbytes):
        q = L.sk_dev_alloc(nbytes)
        assert q
        bufs.append(q)
        return q
    try:
        d_sig, d_len, d_a, d_b = alloc(sig.nbytes), alloc(lens.nbytes), alloc(R * 24), alloc(R * 24)
        check(L.sk_dev_upload(d_sig, ptr(sig), sig.nbytes))
        check(L.sk_dev_upload(d_len, ptr(lens), lens.nbytes))
        check(L.sk_motifseq_dev_i16(d_sig, stride, d_len, R, ptr(motif), motif.size, MODES[scale], 0, 1200, d_a))
        check(L.sk_motifseq_multi_dev_i16(d_sig, stride, d_len, R, ptr(motif), ptr(moff), 1, MODES[scale], 0, 1200, d_b))
        single, multi = np.zeros(R, dtype=HIT_DTYPE), np.zeros(R, dtype=HIT_DTYPE)
        check(L.sk_dev_download(ptr(single), d_a, single.nbytes))
        check(L.sk_dev_download(ptr(multi), d_b, multi.nbytes))
    finally:
        for q in bufs:
            L.sk_dev_free(q)
    assert single.tobytes() == multi.tobytes()
    _oracle_equal(single, want[scale], "device int16 " + scale)


@pytest.mark.parametrize("scale", list(MODES))
def test_single_equals_multi_of_one_ragged(gpu, one_motif, scale):
    """the same integer samples as float64 and as centi-units (value x 100)"""
    from squigglekit_amd._lib import HIT_DTYPE, check, ptr
    L = gpu.load()
    sig, lens, motif, _ = one_motif
    R = sig.shape[0]
    off = np.zeros(R + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    flat = np.ascontiguousarray(np.concatenate([sig[r, :lens[r]] for r in range(R)]), dtype=np.float64)
    centi = np.ascontiguousarray(np.concatenate([sig[r, :lens[r]] for r in range(R)]).astype(np.int32) * 100)
    moff = np.array([0, motif.size], dtype=np.int32)
    single, multi, cent = (np.zeros(R, dtype=HIT_DTYPE) for _ in range(3))
    check(L.sk_motifseq_batch_f64(ptr(flat), ptr(off), R, ptr(motif), motif.size, MODES[scale], 0, 1200, ptr(single)))
    check(L.sk_motifseq_multi_batch_f64(ptr(flat), ptr(off), R, ptr(motif), ptr(moff), 1, MODES[scale], 0, 1200, ptr(multi)))
    check(L.sk_motifseq_multi_batch_centi(ptr(centi), ptr(off), R, ptr(motif), ptr(moff), 1, MODES[scale], 0, 1200, ptr(cent)))
    assert single.tobytes() == multi.tobytes()
    assert single.tobytes() == cent.tobytes()
    assert np.all(single["n"] <= lens) and np.any(single["n"] > 0)


@pytest.mark.parametrize("scale", list(MODES))
def test_multi_motif_over_sub_batches(gpu, ora, monkeypatch, scale):
    """9 000 reads x stride 512, motifs of 24, 40 and 64 points.  SK_INGEST_MB=1: three sub-batches of 3 000 reads
    (sub_batches: at least 4 096 reads each, then an even split), so the fused prologue runs with the first motif of
    each only and the retry total accumulates across motifs and sub-batches.  Equal to the unsplit call byte for byte;
    equal to the oracle around reads 4 096 and 8 192 (a split at the floor itself) and around the seams 3 000 / 6 000."""
    from squigglekit_amd import api, synth
    R, stride = 9000, 512
    motifs = [synth.synthetic_motif(n, seed=20 + n) for n in (24, 40, 64)]
    sig = synth.squiggle_batch(R, stride, 272727, motif=motifs[1])
    lens = np.random.default_rng(27).integers(100, stride + 1, R).astype(np.int32)
    whole = api.motifseq_multi_batch(sig, lens, motifs, scale=scale)
    monkeypatch.setenv("SK_INGEST_MB", "1")
    split = api.motifseq_multi_batch(sig, lens, motifs, scale=scale)
    monkeypatch.delenv("SK_INGEST_MB")
    assert len(whole) == len(split) == 3
    for k in range(3):
        assert split[k].tobytes() == whole[k].tobytes(), k
    rows = np.concatenate([np.arange(4090, 4103), np.arange(8186, 8199), np.arange(2994, 3007), np.arange(5994, 6007)])
    for k, m in enumerate(motifs):
        _oracle_equal(split[k][rows], ora.motifseq_batch_i16(sig[rows], lens[rows], m, scale_mode=MODES[scale]),
                      "motif %d %s" % (k, scale))


def test_multi_on_mixed_reads_equals_any_per_motif(gpu):
    """40 reads, every other one integer valued, 3 motifs: motifseq_multi (int16 rows once, the float reads staged
    once for all motifs) gives motifseq_any's records motif by motif."""
    from squigglekit_amd import api, synth
    motifs = [synth.synthetic_motif(n, seed=30 + n) for n in (24, 40, 64)]
    rng = np.random.default_rng(37)
    sig = synth.squiggle_batch(40, 900, 373737, motif=motifs[0])
    reads = []
    for r in range(40):
        x = sig[r, :int(rng.integers(300, 901))]
        reads.append(x if r % 2 == 0 else np.round((x.astype(np.float64) + 16.0) * (1493.94 / 8192.0) * 5.0, 2))
    for scale in MODES:
        got = api.motifseq_multi(reads, motifs, scale=scale)
        want = [api.motifseq_any(reads, m, scale=scale) for m in motifs]
        assert len(got) == 3
        for k in range(3):
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (scale, k)
            assert np.all(got[k]["n"] > 0)


# ---------------------------------------------------------------------------------------------------------------
# Argument table.  Every case returns from the checks: no kernel is launched.  The codes are those of the code before
# the first-match family got one request and one check (read off its checks, then run).
INVALID = -1
ENTRIES = ["dev_i16", "batch_i16", "multi_dev_i16", "multi_batch_i16", "batch_f64", "multi_batch_f64",
           "multi_batch_centi", "dev_f64"]
# case -> code per entry point; "empty": nreads == 0 and every pointer NULL, motif included -- only
# sk_motifseq_batch_i16 answers an empty batch before it looks at the motif
CASES = {
    "null_motif": INVALID, "no_motif": INVALID, "empty_motif": INVALID, "scale_mode_7": INVALID,
    "nreads_minus_1": INVALID, "null_out": INVALID,
    "empty": {"batch_i16": 0},
    "empty_with_motif": 0,
}


def _expected(case, entry):
    want = CASES[case]
    return want.get(entry, INVALID) if isinstance(want, dict) else want


@pytest.fixture(scope="module")
def arg_bufs(gpu):
    """one valid read of 64 samples in every form an entry point takes"""
    from squigglekit_amd._lib import HIT_DTYPE, ptr
    L = gpu.load()
    b = {"sig": (np.arange(64, dtype=np.int16) * 7 % 300 + 400).reshape(1, 64), "len": np.array([64], dtype=np.int32),
         "off": np.array([0, 64], dtype=np.int64), "out": np.zeros(4, dtype=HIT_DTYPE)}
    b["f64"] = np.ascontiguousarray(b["sig"][0], dtype=np.float64)
    b["centi"] = np.ascontiguousarray(b["sig"][0].astype(np.int32) * 100)
    dev = {k: L.sk_dev_alloc(b[k].nbytes) for k in ("sig", "len", "off", "f64", "out")}
    assert all(dev.values())
    for k in ("sig", "len", "off", "f64"):
        assert L.sk_dev_upload(dev[k], ptr(b[k]), b[k].nbytes) == 0
    yield b, dev
    for q in dev.values():
        L.sk_dev_free(q)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_table(gpu, arg_bufs, entry, case):
    from squigglekit_amd._lib import ptr
    L = gpu.load()
    b, dev = arg_bufs
    motif = np.linspace(-1.0, 1.0, 16)
    multi = entry.startswith("multi")
    on_dev = "_dev_" in entry or entry.startswith("dev_")
    a = {"nreads": 1, "motif": ptr(motif), "nmotif": 16, "moff": np.array([0, 16], dtype=np.int32), "nmotifs": 1,
         "mode": 0, "out": dev["out"] if on_dev else ptr(b["out"]), "input": True}
    if case == "null_motif":
        a["motif"] = None
    elif case == "no_motif":
        a["nmotif"], a["nmotifs"] = 0, 0
    elif case == "empty_motif":
        a["nmotif"], a["moff"] = 0, np.array([0, 0], dtype=np.int32)
    elif case == "scale_mode_7":
        a["mode"] = 7
    elif case == "nreads_minus_1":
        a["nreads"] = -1
    elif case == "null_out":
        a["out"] = None
    elif case == "empty":
        a.update(nreads=0, motif=None, nmotif=0, moff=None, nmotifs=0, out=None, input=False)
    elif case == "empty_with_motif":
        a.update(nreads=0, out=None, input=False)
    moff = None if a["moff"] is None else ptr(a["moff"])
    mot = (a["motif"], moff, a["nmotifs"]) if multi else (a["motif"], a["nmotif"])
    tail = mot + (a["mode"], 0, 1200, a["out"])
    given = a["input"]
    if entry.endswith("_i16"):
        rows = (dev["sig"], 64, dev["len"]) if on_dev else (ptr(b["sig"]), 64, ptr(b["len"]))
        args = (rows if given else (None, 64, None)) + (a["nreads"],) + tail
    elif entry == "dev_f64":
        args = ((dev["f64"], dev["off"]) if given else (None, None)) + (a["nreads"], 64 if given else 0, 64 if given else 0) + tail
    else:
        src = b["centi"] if entry.endswith("centi") else b["f64"]
        args = ((ptr(src), ptr(b["off"])) if given else (None, None)) + (a["nreads"],) + tail
    rc = getattr(L, "sk_motifseq_" + entry)(*args)
    assert rc == _expected(case, entry), (entry, case, rc, L.sk_last_error())
