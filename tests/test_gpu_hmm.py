"""GPU: the signal HMM's Viterbi pass (sk_hmm.hip) against the numpy statement of its definition (tests/hmm_ref.py).

Every field of every record is compared exactly, the score by its bit pattern: there is no tolerance anywhere.  The
kernel's seams: 64 reads share a wavefront (one lane each), the int16 feed loads tiles of 128 samples per read with
16-byte loads (2-byte loads for rows that are not 16-byte aligned), the float64 feed tiles of 32 values.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import hmm_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = -np.inf
# the seams of both feeds' tiles (128 and 32), +-1
LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4000)


def assert_same(got, want, what):
    assert got.shape == want.shape, what
    for f in ("final_state", "n_used", "enter"):
        bad = np.flatnonzero((got[f] != want[f]).reshape(len(got), -1).any(axis=1))
        assert bad.size == 0, "%s: %s differs at read %d: got %r, want %r" % (what, f, bad[0], got[bad[0]], want[bad[0]])
    bad = np.flatnonzero(got["score"].view(np.uint64) != want["score"].view(np.uint64))
    assert bad.size == 0, "%s: score differs at read %d: got %r, want %r" % (what, bad[0], got[bad[0]], want[bad[0]])
    assert got.tobytes() == want.tobytes(), what


def rows(reads, stride=None):
    lens = np.array([len(r) for r in reads], dtype=np.int32)
    stride = stride or max(8, (int(lens.max()) + 7) // 8 * 8)
    buf = np.full((len(reads), stride), -12345, dtype=np.int16)          # (nothing past a read's end may matter)
    for i, r in enumerate(reads):
        buf[i, :len(r)] = r
    return buf, lens


def planted(rng, n):
    """a short direct-RNA-like read of n samples: adapter N(430, 25), poly(A) N(560, 8), a body of levels N(530, 80)"""
    la, lp = int(n * rng.uniform(0.2, 0.5)), int(n * rng.uniform(0.1, 0.3))
    body = np.repeat(rng.normal(530, 80, n // 8 + 2), 8)[:max(0, n - la - lp)] + rng.normal(0, 8, max(0, n - la - lp))
    return np.rint(np.concatenate([rng.normal(430, 25, la), rng.normal(560, 8, lp), body])[:n]).astype(np.int16)


def random_model(rng, S, integer=False):
    """S states, -inf in linit, ltrans and the second components; integer: small integer scores and levels (ties)"""
    from squigglekit_amd._lib import HmmModel
    if integer:
        linit = rng.integers(-3, 1, S).astype(np.float64)
        ltrans = rng.integers(-2, 1, (S, S)).astype(np.float64)
        c = rng.integers(-2, 1, (S, 2)).astype(np.float64)
        mu = rng.integers(498, 503, (S, 2)).astype(np.float64)
        h = rng.integers(0, 2, (S, 2)).astype(np.float64)
    else:
        linit = np.log(rng.uniform(0.05, 1.0, S))
        ltrans = np.log(rng.uniform(0.001, 1.0, (S, S)))
        c = np.log(rng.uniform(0.05, 1.0, (S, 2))) - np.log(rng.uniform(5, 60, (S, 2)))
        mu = rng.uniform(380, 620, (S, 2))
        h = 1.0 / (2.0 * rng.uniform(5, 60, (S, 2)) ** 2)
        h[rng.random((S, 2)) < 0.2] = 0.0
    linit[rng.random(S) < 0.3] = NINF
    if not np.isfinite(linit).any():
        linit[0] = 0.0
    ltrans[rng.random((S, S)) < 0.35] = NINF
    c[rng.random(S) < 0.5, 1] = NINF
    return HmmModel.from_arrays(S, linit, ltrans, c, mu, h)


@pytest.fixture(scope="module")
def pool():
    """130 planted reads: every length of LENGTHS inside the first group of 64, mixed lengths after it"""
    rng = np.random.default_rng(20261018)
    lengths = list(LENGTHS) + [int(v) for v in rng.choice([0, 3, 40, 100, 130, 260, 300, 520, 700, 900], size=130 - len(LENGTHS))]
    order = rng.permutation(64)
    lengths[:64] = [lengths[i] for i in order]
    return [planted(rng, n) for n in lengths]


@pytest.fixture(scope="module")
def models():
    from squigglekit_amd import api
    rng = np.random.default_rng(11)
    out = {"synth_raw": api.polya_model("synth_raw")}
    for S in (1, 2, 5, 6):
        out["random S=%d" % S] = random_model(rng, S)
        out["integer S=%d" % S] = random_model(rng, S, integer=True)
    # the best path never leaves state 0: state 1 fits nothing and is hard to reach
    out["stays in 0"] = api.hmm_model([0.5, 0.5], [[0.999, 0.001], [0.5, 0.5]], [[(1.0, 500.0, 200.0)], [(1.0, 5000.0, 1.0)]])
    # tied predecessors: every transition 0, every state the same flat emission -- every candidate ties at every step
    out["all tied"] = api.HmmModel.from_arrays(4, [0.0] * 4, np.zeros((4, 4)), np.tile([-1.0, NINF], (4, 1)), np.zeros((4, 2)),
                                               np.zeros((4, 2)))
    return out


@pytest.fixture(scope="module")
def want(pool, models):
    """the numpy statement's records of the pool under every model, computed once"""
    buf, lens = rows(pool)
    return {name: hmm_ref.viterbi_batch(m, buf, lens) for name, m in models.items()}


MODEL_NAMES = ["synth_raw", "stays in 0", "all tied"] + ["%s S=%d" % (k, S) for k in ("random", "integer") for S in (1, 2, 5, 6)]


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_models_on_the_pool(gpu, pool, models, want, name):
    from squigglekit_amd import api
    buf, lens = rows(pool)
    got = api.hmm_viterbi_batch(buf, lens, models[name])
    assert_same(got, want[name], name)
    if name == "stays in 0":
        assert (got["final_state"][lens > 0] == 0).all() and (got["enter"][lens > 0][:, 1] == -1).all()
    if name == "all tied":
        assert (got["final_state"][lens > 0] == 0).all() and (got["enter"][lens > 0] == [0, -1, -1, -1, -1, -1]).all()
    if name == "synth_raw":
        assert api.polya_segments(got)["found"].any()


def test_read_counts_and_unaligned_rows(gpu, pool, models, want):
    from squigglekit_amd import api
    for name in ("synth_raw", "random S=5"):
        for R in (1, 63, 64, 65, 130):
            buf, lens = rows(pool[:R], stride=4000)
            assert_same(api.hmm_viterbi_batch(buf, lens, models[name]), want[name][:R], "%d reads %s" % (R, name))
        buf, lens = rows(pool, stride=4003)                               # rows that are not 16-byte aligned
        assert_same(api.hmm_viterbi_batch(buf, lens, models[name]), want[name], "stride 4003 " + name)


def test_limit(gpu, pool, models):
    from squigglekit_amd import api
    m = models["random S=6"]
    buf, lens = rows(pool)
    for limit in (1, 64, 129, 300, 4000, 5000):                           # below, equal to and above the lengths
        got = api.hmm_viterbi_batch(buf, lens, m, limit=limit)
        assert_same(got, hmm_ref.viterbi_batch(m, buf, lens, limit=limit), "limit %d" % limit)
        assert (got["n_used"] == np.minimum(lens, limit)).all()


def test_calibration(gpu, pool, models, want):
    from squigglekit_amd import api
    rng = np.random.default_rng(5)
    buf, lens = rows(pool)
    R = len(pool)
    # a pA model: the raw levels of the planted reads under (raw + 3) * 0.21
    m = api.hmm_model([0.5, 0.5, 0.0], [[0.99, 0.01, 0.0], [0.0, 0.999, 0.001], [0.0, 0.0, 1.0]],
                      [[(1.0, 90.9, 5.3)], [(0.9, 118.2, 1.7), (0.1, None, 400.0)], [(0.5, 112.0, 4.0), (0.5, 111.0, 18.0)]])
    cal = np.stack([rng.uniform(-20, 20, R), rng.uniform(0.15, 0.25, R)], axis=1)
    got = api.hmm_viterbi_batch(buf, lens, m, cal2=cal)
    assert_same(got, hmm_ref.viterbi_batch(m, buf, lens, cal2=cal), "calibrated")
    assert len(set(got["final_state"].tolist())) > 1
    # NULL against the identity pair, and against a calibration that matters
    ident = np.tile([0.0, 1.0], (R, 1))
    assert_same(api.hmm_viterbi_batch(buf, lens, models["synth_raw"], cal2=ident), want["synth_raw"], "identity pair")
    assert api.hmm_viterbi_batch(buf, lens, m).tobytes() != got.tobytes()


def test_device_form_equals_host_form(gpu, pool, models, want):
    L = gpu.load()
    buf, lens = rows(pool)
    R = len(pool)
    cal = np.tile([0.0, 1.0], (R, 1))
    sizes = (buf.nbytes, lens.nbytes, cal.nbytes, R * 40)
    d = [L.sk_dev_alloc(n) for n in sizes]
    try:
        assert all(d)
        for dst, a in zip(d, (buf, lens, cal)):
            gpu.check(L.sk_dev_upload(dst, gpu.ptr(a), a.nbytes))
        for name, d_cal in (("synth_raw", None), ("random S=5", d[2])):
            rec = np.zeros(R, dtype=gpu.HMM_DTYPE)
            gpu.check(L.sk_hmm_viterbi_dev_i16(d[0], buf.shape[1], d[1], R, d_cal, C.byref(models[name]), 0, d[3]))
            gpu.check(L.sk_sync())
            gpu.check(L.sk_dev_download(gpu.ptr(rec), d[3], rec.nbytes))
            assert_same(rec, want[name], "device form " + name)
    finally:
        for p in d:
            if p:
                L.sk_dev_free(p)


def test_device_form_with_a_misaligned_base(gpu, pool, models, want):
    """rows of a stride that is a multiple of 8 from a base 2 bytes past a 16-byte boundary: the launcher has to see the
    base, not only the stride, and take the 2-byte loads"""
    L = gpu.load()
    buf, lens = rows(pool)
    R = len(pool)
    assert buf.shape[1] % 8 == 0
    d_sig, d_len, d_rec = L.sk_dev_alloc(buf.nbytes + 16), L.sk_dev_alloc(lens.nbytes), L.sk_dev_alloc(R * 40)
    try:
        assert d_sig and d_len and d_rec and d_sig % 16 == 0
        gpu.check(L.sk_dev_upload(d_sig + 2, gpu.ptr(buf), buf.nbytes))
        gpu.check(L.sk_dev_upload(d_len, gpu.ptr(lens), lens.nbytes))
        rec = np.zeros(R, dtype=gpu.HMM_DTYPE)
        gpu.check(L.sk_hmm_viterbi_dev_i16(d_sig + 2, buf.shape[1], d_len, R, None, C.byref(models["random S=6"]), 0, d_rec))
        gpu.check(L.sk_sync())
        gpu.check(L.sk_dev_download(gpu.ptr(rec), d_rec, rec.nbytes))
        assert_same(rec, want["random S=6"], "device form, base + 2 bytes")
    finally:
        for p in (d_sig, d_len, d_rec):
            if p:
                L.sk_dev_free(p)


def test_float64_feed_equals_int16_feed(gpu, pool, models, want):
    from squigglekit_amd import api
    for name in ("synth_raw", "integer S=6", "random S=2"):
        values, off = api.pack_f64([r.astype(np.float64) for r in pool])
        assert_same(api.hmm_viterbi_ragged_f64(values, off, models[name]), want[name], "float64 " + name)
        got = api.hmm_viterbi_ragged_f64(values, off, models[name], limit=33)
        assert_same(got, hmm_ref.viterbi_reads(models[name], pool, limit=33), "float64, limit 33 " + name)
    # values that are not integers, and the mixed list form
    rng = np.random.default_rng(9)
    reads = [r.astype(np.float64) * 0.21 + rng.normal(0, 0.01, r.size) if i % 2 else r for i, r in enumerate(pool[:40])]
    m = models["random S=5"]
    assert_same(api.hmm_viterbi(reads, m), hmm_ref.viterbi_reads(m, reads), "mixed list")


def test_sub_batches_equal_one_call(gpu, pool, models, monkeypatch):
    """9 000 reads x stride 128 with SK_INGEST_MB=1: three sub-batches of 3 000 reads, each with its calibration pairs"""
    from squigglekit_amd import api
    rng = np.random.default_rng(5)
    base = np.stack([planted(rng, 128) for _ in range(90)])
    sig = np.tile(base, (100, 1))
    lens = (np.arange(9000) * 37 % 129).astype(np.int32)
    cal = np.stack([(np.arange(9000) % 7).astype(np.float64), np.full(9000, 1.0)], axis=1)
    m = models["synth_raw"]
    one = api.hmm_viterbi_batch(sig, lens, m, cal2=cal)
    monkeypatch.setenv("SK_INGEST_MB", "1")
    three = api.hmm_viterbi_batch(sig, lens, m, cal2=cal)
    monkeypatch.delenv("SK_INGEST_MB")
    assert_same(three, one, "sub-batches")
    pick = [0, 1, 2999, 3000, 3001, 5999, 6000, 8999]                     # ... and both are the definition's
    assert_same(one[pick], hmm_ref.viterbi_batch(m, sig[pick], lens[pick], cal2=cal[pick]), "picked reads")


def test_cli_i16_stdout(gpu, pool, models, want, tmp_path):
    """dRNA_polya.py --i16: its stdout against lines formed from the numpy statement's records"""
    from squigglekit_amd import polya_cli
    reads = [r for r in pool if len(r) >= 255][:24]
    n = min(len(r) for r in reads)
    a = np.stack([r[:n] for r in reads])
    path = tmp_path / "reads.npy"
    np.save(path, a)
    rec = hmm_ref.viterbi_batch(models["synth_raw"], a, np.full(len(a), n))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "dRNA_polya.py"), "--i16", str(path), "--preset", "synth_raw",
                        "--batch", "10"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr
    assert p.stdout == "".join(polya_cli.polya_lines([str(i) for i in range(len(a))], rec))
    assert len(p.stdout.splitlines()) == len(a)


def test_cli_tsv_with_a_read_without_samples(gpu, pool, models, tmp_path):
    """dRNA_polya.py -s: one line per read, the read without samples included, in input order"""
    from squigglekit_amd import polya_cli
    reads = [pool[i] for i in np.argsort([-len(r) for r in pool])[:3]]
    reads.insert(1, np.zeros(0, dtype=np.int16))
    path = tmp_path / "raw.tsv"
    path.write_text("".join("f.fast5\tid%d\tx\ty%s\n" % (i, "".join("\t%d" % v for v in r)) for i, r in enumerate(reads)))
    rec = hmm_ref.viterbi_reads(models["synth_raw"], reads)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "dRNA_polya.py"), "-s", str(path), "--preset", "synth_raw"],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr
    assert p.stdout == "".join(polya_cli.polya_lines(["id%d" % i for i in range(4)], rec))
    assert p.stdout.splitlines()[1] == "id1\t.\t.\t.\t.\t0\t."
