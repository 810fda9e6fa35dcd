"""GPU: the signal HMM's state paths (sk_hmm.hip: the forward pass that keeps the back pointers, the backward sweep, the
statistics fill) against the numpy statement of their definition (tests/hmm_path_ref.py).

Every field is compared exactly and arrays by tobytes(): there is no tolerance anywhere.  The pool, the models and the
seams are those of tests/test_gpu_hmm.py: 64 reads share a wavefront, tiles of 128 (int16) and 32 (float64) samples; the
back pointers of a group are padded to the longest read the call allows, and a large batch is worked through in slices of
whole groups (SK_HMM_SCRATCH_MB).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import hmm_path_ref
import hmm_ref
from test_gpu_hmm import MODEL_NAMES, models, planted, pool, rows  # noqa: F401  (pool and models are fixtures)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_same(got, want, what):
    """(rec, off, seg) of a call against (off, seg) of the statement; rec is compared by the caller"""
    g_off, g_seg = got[1], got[2]
    w_off, w_seg = want[1], want[2]
    assert g_off.dtype == np.int64 and g_off.tolist() == w_off.tolist(), what
    assert g_seg.dtype == w_seg.dtype and g_seg.shape == w_seg.shape, what
    for f in ("state", "start", "length", "n1", "sum", "sumsq"):
        a, b = g_seg[f], w_seg[f]
        if a.dtype.kind == "f":
            a, b = a.view(np.uint64), b.view(np.uint64)
        bad = np.flatnonzero((a != b).reshape(len(g_seg), -1).any(axis=1))
        assert bad.size == 0, "%s: %s differs at segment %d: got %r, want %r" % (what, f, bad[0], g_seg[bad[0]], w_seg[bad[0]])
    assert g_seg.tobytes() == w_seg.tobytes(), what


@pytest.fixture(scope="module")
def want(pool, models):
    """the statement's (rec, off, seg) of the pool under every model, computed once (rec: n_used and final_state only --
    the records are compared with the Viterbi call's)"""
    buf, lens = rows(pool)
    x = buf.astype(np.float64)
    return {name: hmm_path_ref.segments_rows(m, x, lens, raw=buf, records=False) for name, m in models.items()}


def take(want, R):
    """the statement's result cut to the first R reads"""
    rec, off, seg = want
    return rec[:R], off[:R + 1], seg[:off[R]]


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_models_on_the_pool(gpu, pool, models, want, name):
    from squigglekit_amd import api
    buf, lens = rows(pool)
    got = api.hmm_segments_batch(buf, lens, models[name])
    assert got[0].tobytes() == api.hmm_viterbi_batch(buf, lens, models[name]).tobytes(), name
    assert_same(got, want[name], name)
    hmm_path_ref.invariants(models[name], *got)
    per = np.diff(got[1])
    if name == "stays in 0":
        assert (per == (lens > 0)).all()                                  # one segment per read with samples
    if name == "all tied":
        assert (per == (lens > 0)).all() and (got[2]["state"] == 0).all()
    if name == "synth_raw":
        assert per.max() >= 3


def test_read_counts_and_unaligned_rows(gpu, pool, models, want):
    from squigglekit_amd import api
    for name in ("synth_raw", "random S=5"):
        for R in (1, 63, 64, 65, 130):
            buf, lens = rows(pool[:R], stride=4000)
            got = api.hmm_segments_batch(buf, lens, models[name])
            assert_same(got, take(want[name], R), "%d reads %s" % (R, name))
            assert got[0].tobytes() == api.hmm_viterbi_batch(buf, lens, models[name]).tobytes()
        buf, lens = rows(pool, stride=4003)                               # rows that are not 16-byte aligned
        assert_same(api.hmm_segments_batch(buf, lens, models[name]), want[name], "stride 4003 " + name)


def test_padding_and_empty_groups(gpu, models):
    """a group whose reads have 0 .. 3 samples but one of 4 000 (its back pointers are padded to 4 000 rows and written for
    one lane only), then a group of only empty reads, then a short one"""
    from squigglekit_amd import api
    rng = np.random.default_rng(77)
    reads = [planted(rng, i % 4) for i in range(64)]
    reads[37] = planted(rng, 4000)
    reads += [np.zeros(0, dtype=np.int16)] * 64 + [planted(rng, n) for n in (200, 0, 131)]
    buf, lens = rows(reads)
    for name in ("synth_raw", "integer S=6"):
        got = api.hmm_segments_batch(buf, lens, models[name])
        assert_same(got, hmm_path_ref.segments_batch(models[name], buf, lens), name)
        assert got[0].tobytes() == api.hmm_viterbi_batch(buf, lens, models[name]).tobytes()
        assert (np.diff(got[1])[64:128] == 0).all()
        hmm_path_ref.invariants(models[name], *got)


def test_limit(gpu, pool, models):
    from squigglekit_amd import api
    m = models["random S=6"]
    buf, lens = rows(pool)
    for limit in (1, 64, 129, 5000):                                      # below, equal to and above the lengths
        got = api.hmm_segments_batch(buf, lens, m, limit=limit)
        assert_same(got, hmm_path_ref.segments_batch(m, buf, lens, limit=limit), "limit %d" % limit)
        assert got[0].tobytes() == api.hmm_viterbi_batch(buf, lens, m, limit=limit).tobytes()
        assert (got[0]["n_used"] == np.minimum(lens, limit)).all()


def test_calibration(gpu, pool, models, want):
    """the component decisions follow the calibrated values, the sums stay raw"""
    from squigglekit_amd import api
    rng = np.random.default_rng(5)
    buf, lens = rows(pool)
    R = len(pool)
    m = api.hmm_model([0.5, 0.5, 0.0], [[0.99, 0.01, 0.0], [0.0, 0.999, 0.001], [0.0, 0.0, 1.0]],
                      [[(1.0, 90.9, 5.3)], [(0.9, 118.2, 1.7), (0.1, None, 400.0)], [(0.5, 112.0, 4.0), (0.5, 111.0, 18.0)]])
    cal = np.stack([rng.uniform(-20, 20, R), rng.uniform(0.15, 0.25, R)], axis=1)
    got = api.hmm_segments_batch(buf, lens, m, cal2=cal)
    assert_same(got, hmm_path_ref.segments_batch(m, buf, lens, cal2=cal), "calibrated")
    assert got[0].tobytes() == api.hmm_viterbi_batch(buf, lens, m, cal2=cal).tobytes()
    assert 0 < got[2]["n1"].sum() < got[2]["length"].sum()                # both components win somewhere
    for r in (5, 70, 129):                                                # raw sums: those of the read's samples
        g = got[2][got[1][r]:got[1][r + 1]]
        assert g["sum"].sum() == pool[r].astype(np.int64).sum() and g["sumsq"].sum() == (pool[r].astype(np.int64) ** 2).sum()
    ident = np.tile([0.0, 1.0], (R, 1))
    assert_same(api.hmm_segments_batch(buf, lens, models["synth_raw"], cal2=ident), want["synth_raw"], "identity pair")
    assert api.hmm_segments_batch(buf, lens, m)[2].tobytes() != got[2].tobytes()


def device_call(gpu, buf, lens, model, cal=None, shift=0, cap=None, limit=0):
    """sk_hmm_segments_dev_i16 on uploaded rows (shift: bytes past the 16-byte aligned base): rec, off and d_seg with 8
    records of room behind cap, every byte 0x5A before the call"""
    L = gpu.load()
    R = len(lens)
    cap = 64 * R if cap is None else cap
    sizes = (buf.nbytes + 16, lens.nbytes, 16 * R, R * 40, (R + 1) * 8, (cap + 8) * 48)
    d = [L.sk_dev_alloc(n) for n in sizes]
    try:
        assert all(d) and d[0] % 16 == 0
        gpu.check(L.sk_dev_upload(d[0] + shift, gpu.ptr(buf), buf.nbytes))
        gpu.check(L.sk_dev_upload(d[1], gpu.ptr(lens), lens.nbytes))
        if cal is not None:
            gpu.check(L.sk_dev_upload(d[2], gpu.ptr(cal), cal.nbytes))
        mark = np.full((cap + 8) * 48, 0x5A, dtype=np.uint8)
        gpu.check(L.sk_dev_upload(d[5], gpu.ptr(mark), mark.nbytes))
        rec, off = np.zeros(R, dtype=gpu.HMM_DTYPE), np.zeros(R + 1, dtype=np.int64)
        seg = np.zeros(cap + 8, dtype=gpu.HMM_SEG_DTYPE)
        gpu.check(L.sk_hmm_segments_dev_i16(d[0] + shift, buf.shape[1], d[1], R, d[2] if cal is not None else None,
                                            C.byref(model), limit, d[3], d[4], d[5] if cap else None, cap))
        gpu.check(L.sk_sync())
        for dst, src in ((rec, d[3]), (off, d[4]), (seg, d[5])):
            gpu.check(L.sk_dev_download(gpu.ptr(dst), src, dst.nbytes))
        return rec, off, seg
    finally:
        for p in d:
            if p:
                L.sk_dev_free(p)


def test_device_form(gpu, pool, models, want):
    from squigglekit_amd import api
    buf, lens = rows(pool)
    R = len(pool)
    cal = np.tile([0.0, 1.0], (R, 1))
    for name, c2, shift in (("synth_raw", None, 0), ("random S=5", cal, 0), ("random S=6", None, 2)):
        assert buf.shape[1] % 8 == 0                                      # shift 2: the base alone breaks the 16-byte alignment
        w = want[name]
        rec, off, seg = device_call(gpu, buf, lens, models[name], c2, shift, cap=int(w[1][-1]) + 7)
        assert rec.tobytes() == api.hmm_viterbi_batch(buf, lens, models[name]).tobytes(), name
        assert_same((rec, off, seg[:off[-1]]), w, "device form " + name)
        assert (seg[off[-1]:].view(np.uint8) == 0x5A).all()                # nothing past the segments
    # above cap: SK_OK, d_off complete, nothing written past d_seg[cap - 1]
    w = want["random S=5"]
    for cap in (int(w[1][-1]) - 1, int(w[1][-1]) // 2, 0):
        rec, off, seg = device_call(gpu, buf, lens, models["random S=5"], cap=cap)
        assert off.tolist() == w[1].tolist() and (seg[cap:].view(np.uint8) == 0x5A).all(), cap
        assert rec.tobytes() == api.hmm_viterbi_batch(buf, lens, models["random S=5"]).tobytes()


def test_float64_feed(gpu, pool, models, want):
    from squigglekit_amd import api
    for name in ("synth_raw", "integer S=6", "random S=2"):
        values, off = api.pack_f64([r.astype(np.float64) for r in pool])
        rec, soff, seg = api.hmm_segments_ragged_f64(values, off, models[name])
        w = want[name]
        assert seg.dtype == api.HMM_SEGF_DTYPE and soff.tolist() == w[1].tolist(), name
        assert rec.tobytes() == api.hmm_viterbi_ragged_f64(values, off, models[name]).tobytes()
        for f in ("state", "start", "length", "n1"):
            assert (seg[f] == w[2][f]).all(), (name, f)
        assert (seg["sum"] == w[2]["sum"]).all() and (seg["sumsq"] == w[2]["sumsq"]).all()      # equal as numbers
        got = api.hmm_segments_ragged_f64(values, off, models[name], limit=33)                  # one past the tile of 32
        assert_same(got, hmm_path_ref.segments_reads(models[name], pool, limit=33), "float64, limit 33 " + name)
    # values that are not integers: bit for bit the statement's, the sums in rising order
    rng = np.random.default_rng(9)
    reads = [r.astype(np.float64) * 0.21 + rng.normal(0, 0.01, r.size) for r in pool[:70]]
    m = api.hmm_model([0.5, 0.5, 0.0], [[0.99, 0.01, 0.0], [0.0, 0.999, 0.001], [0.0, 0.0, 1.0]],
                      [[(1.0, 90.9, 5.3)], [(0.9, 118.2, 1.7), (0.1, None, 400.0)], [(0.5, 112.0, 4.0), (0.5, 111.0, 18.0)]])
    for mm in (m, models["random S=5"]):
        got = api.hmm_segments_ragged_f64(*api.pack_f64(reads), mm)
        ref = hmm_path_ref.segments_reads(mm, reads)
        assert_same(got, ref, "float64 reads")
        assert got[0].tobytes() == ref[0].tobytes()
        hmm_path_ref.invariants(mm, *got)
    # the mixed list form: input order kept, each read through its own feed
    mixed = [r if i % 2 else reads[i] for i, r in enumerate(pool[:40])]
    rec, segs = api.hmm_segments(mixed, m)
    assert rec.tobytes() == api.hmm_viterbi(mixed, m).tobytes()
    for i, r in enumerate(mixed):
        one = hmm_path_ref.segments_reads(m, [r], raw=bool(i % 2) or len(r) == 0)    # (an empty read counts as integer-valued)
        assert segs[i].dtype == one[2].dtype and segs[i].tobytes() == one[2].tobytes(), i
        assert api.hmm_state_path(segs[i], len(r)).size == len(r)


def test_overflow_contract(gpu, pool, models, want):
    L = gpu.load()
    buf, lens = rows(pool)
    R = len(pool)
    m = models["random S=5"]
    w = want["random S=5"]
    total = int(w[1][-1])
    values, voff = np.concatenate([r.astype(np.float64) for r in pool]), np.zeros(R + 1, dtype=np.int64)
    np.cumsum(lens, out=voff[1:])

    def run(cap, f64):
        rec, off = np.zeros(R, dtype=gpu.HMM_DTYPE), np.full(R + 1, -7, dtype=np.int64)
        seg = np.full(max(cap, 1) * 48, 0x5A, dtype=np.uint8)
        sp = gpu.ptr(seg) if cap else None
        if f64:
            rc = L.sk_hmm_segments_f64_len(gpu.ptr(values), gpu.ptr(voff), R, C.byref(m), 0, gpu.ptr(rec), gpu.ptr(off), sp, cap)
        else:
            rc = L.sk_hmm_segments_i16(gpu.ptr(buf), buf.shape[1], gpu.ptr(lens), R, None, C.byref(m), 0, gpu.ptr(rec),
                                       gpu.ptr(off), sp, cap)
        return rc, rec, off, seg
    for f64 in (False, True):
        rc, rec, off, seg = run(0, f64)                                   # the counting call
        assert rc == gpu.SK_ERR_OVERFLOW and off.tolist() == w[1].tolist()
        assert rec["final_state"].tolist() == w[0]["final_state"].tolist()
        rc, rec, off, seg = run(total - 1, f64)                           # one short
        assert rc == gpu.SK_ERR_OVERFLOW and off.tolist() == w[1].tolist() and (seg == 0x5A).all()
        rc, rec, off, seg = run(total, f64)                               # exact
        assert rc == 0 and off.tolist() == w[1].tolist()
        got = seg.view(gpu.HMM_SEGF_DTYPE if f64 else gpu.HMM_SEG_DTYPE)
        assert (got["state"] == w[2]["state"]).all() and (got["sum"] == w[2]["sum"]).all()
    # no segment at all: the counting call returns SK_OK
    none = np.zeros(3, dtype=np.int32)
    rec, off = np.zeros(3, dtype=gpu.HMM_DTYPE), np.full(4, -7, dtype=np.int64)
    assert L.sk_hmm_segments_i16(gpu.ptr(buf), buf.shape[1], gpu.ptr(none), 3, None, C.byref(m), 0, gpu.ptr(rec), gpu.ptr(off),
                                 None, 0) == 0
    assert off.tolist() == [0, 0, 0, 0] and (rec["final_state"] == -1).all()


def test_sub_batches_equal_one_call(gpu, models, monkeypatch):
    """9 000 reads x stride 128 with SK_INGEST_MB=1: three sub-batches of 3 000 reads, each with its calibration pairs and
    its own groups; the offsets run on across them"""
    from squigglekit_amd import api
    rng = np.random.default_rng(5)
    base = np.stack([planted(rng, 128) for _ in range(90)])
    sig = np.tile(base, (100, 1))
    lens = (np.arange(9000) * 37 % 129).astype(np.int32)
    cal = np.stack([(np.arange(9000) % 7).astype(np.float64), np.full(9000, 1.0)], axis=1)
    m = models["synth_raw"]
    one = api.hmm_segments_batch(sig, lens, m, cal2=cal)
    monkeypatch.setenv("SK_INGEST_MB", "1")
    three = api.hmm_segments_batch(sig, lens, m, cal2=cal)
    monkeypatch.delenv("SK_INGEST_MB")
    assert [a.tobytes() for a in three] == [a.tobytes() for a in one]
    assert one[0].tobytes() == api.hmm_viterbi_batch(sig, lens, m, cal2=cal).tobytes()
    pick = [0, 1, 2999, 3000, 3001, 5999, 6000, 8999]                     # ... and both are the definition's
    ref = hmm_path_ref.segments_batch(m, sig[pick], lens[pick], cal2=cal[pick])
    for k, r in enumerate(pick):
        assert one[2][one[1][r]:one[1][r + 1]].tobytes() == ref[2][ref[1][k]:ref[1][k + 1]].tobytes(), r


def test_slices_equal_one_call(gpu, pool, models, want, monkeypatch):
    """SK_HMM_SCRATCH_MB=1: 1 MB holds the back pointers of one group of 4 000-sample rows, so the 130 reads take three
    slices -- host form, device form and float64 feed"""
    from squigglekit_amd import api
    buf, lens = rows(pool)
    assert buf.shape[1] * 256 <= (1 << 20) < 2 * buf.shape[1] * 256
    monkeypatch.setenv("SK_HMM_SCRATCH_MB", "1")
    try:
        for name in ("synth_raw", "random S=5"):
            assert_same(api.hmm_segments_batch(buf, lens, models[name]), want[name], "slices " + name)
            rec, off, seg = device_call(gpu, buf, lens, models[name], cap=int(want[name][1][-1]))
            assert_same((rec, off, seg[:off[-1]]), want[name], "slices, device form " + name)
            assert rec.tobytes() == api.hmm_viterbi_batch(buf, lens, models[name]).tobytes()
        values, off = api.pack_f64([r.astype(np.float64) for r in pool])
        got = api.hmm_segments_ragged_f64(values, off, models["synth_raw"])
        assert got[1].tolist() == want["synth_raw"][1].tolist() and (got[2]["sum"] == want["synth_raw"][2]["sum"]).all()
    finally:
        monkeypatch.delenv("SK_HMM_SCRATCH_MB")


def test_pool_and_one_refit_round(gpu, pool, models, want):
    """hmm_pool over the GPU's segments: the statement's pooled integers exactly; one hmm_refit round from each: the same
    description"""
    from squigglekit_amd import api
    buf, lens = rows(pool)
    spec = api.polya_spec("synth_raw")
    rec, off, seg = api.hmm_segments_batch(buf, lens, models["synth_raw"])
    got = api.hmm_pool(rec, off, seg, 6)
    plain = hmm_path_ref.pool(*want["synth_raw"], 6)
    for f in ("n", "sum", "sumsq", "trans", "init"):
        assert got[f].dtype == np.int64 and got[f].tolist() == plain[f], f
    theirs = {k: np.array(v) for k, v in plain.items()}
    states = (api.ADAPTER, api.POLYA, api.TRANSCRIPT)
    for update in (("mean", "sigma"), ("mean", "sigma", "weight", "trans")):
        a = api.hmm_refit(spec, got, states, update=update)
        assert a == api.hmm_refit(spec, theirs, states, update=update) and a != (spec[0], spec[1], spec[2])
    # hmm_fit on the GPU: one round over the pool is that refit
    fitted, history = api.hmm_fit(pool, spec, states, 1)
    assert fitted == api.hmm_refit(spec, got, states) and history[0]["segments"] == int(off[-1])


def test_cli_segments_and_polya_net(gpu, pool, models, tmp_path):
    """dRNA_polya.py --i16 --segments FILE --polya_net: stdout and the segments file against lines formed from the numpy
    statement; without the new flags the output is what it was"""
    from squigglekit_amd import api, polya_cli
    reads = [r for r in pool if len(r) >= 255][:24]
    n = min(len(r) for r in reads)
    a = np.stack([r[:n] for r in reads])
    path = tmp_path / "reads.npy"
    np.save(path, a)
    names = [str(i) for i in range(len(a))]
    m = models["synth_raw"]
    rec, off, seg = hmm_path_ref.segments_batch(m, a, np.full(len(a), n))
    base = [sys.executable, os.path.join(ROOT, "dRNA_polya.py"), "--i16", str(path), "--preset", "synth_raw", "--batch", "10"]
    p = subprocess.run(base + ["--segments", "segs.tsv", "--polya_net"], capture_output=True, text=True, timeout=120,
                       cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr
    assert p.stdout == "".join(polya_cli.polya_lines(names, rec, net=polya_cli.polya_net(rec, off, seg)))
    assert (tmp_path / "segs.tsv").read_text() == "".join(polya_cli.segment_lines(names, off, seg, api.POLYA_STATES))
    first = (tmp_path / "segs.tsv").read_text().splitlines()[0].split("\t")
    assert len(first) == 8 and first[:2] == ["0", "0"] and first[2] in api.POLYA_STATES and first[3] == "0"
    old = subprocess.run(base, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert old.returncode == 0, old.stderr
    assert old.stdout == "".join(polya_cli.polya_lines(names, hmm_ref.viterbi_batch(m, a, np.full(len(a), n))))
    assert [ln.rsplit("\t", 1)[0] for ln in p.stdout.splitlines()] == old.stdout.splitlines()
