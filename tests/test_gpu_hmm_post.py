"""GPU: the signal HMM's posteriors (sk_hmm_post.hip) against the numpy statement of their definition
(tests/hmm_post_ref.py).

Every field of every record, every soft count and every dense posterior is compared by its bit pattern: there is no
tolerance anywhere.  The kernels' seams: 64 reads share a wavefront (one lane each), alpha is checkpointed every B = 128
samples (SK_HMM_POST_BLOCK) and recomputed block by block, the int16 feed loads tiles of 128 samples per read, the float64
feed tiles of 32 values, a call is worked through in slices of whole 64-read groups (SK_HMM_SCRATCH_MB) and the host form
in sub-batches (SK_INGEST_MB).
"""
import ctypes as C

import numpy as np
import pytest

import hmm_post_ref as ref

pytestmark = pytest.mark.gpu

NINF = -np.inf
B = 128
# 0, 1, 2; the float64 tile's seams; B - 1, B, B + 1 (the int16 tile's seams too); 2 B + 1; the same for B = 256
LENGTHS = (0, 1, 2, 31, 32, 33, 127, 128, 129, 255, 256, 257, 513)
FIELDS = (("post", ("loglik", "final_post", "occ")), ("counts", ("n", "sx", "sxx", "xi", "init")))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same(got, want, what, rows=None):
    """got, want: (post, counts or None, goff or None, gamma or None); rows: the reads of `want` that `got` holds"""
    gp, gc, goff, gg = got
    wp, wc, woff, wg = want
    if rows is None:
        rows = np.arange(len(wp))
    rows = np.asarray(rows, dtype=np.int64)
    assert len(gp) == len(rows), what
    assert (gp["n_used"] == wp["n_used"][rows]).all() and (gp["flags"] == wp["flags"][rows]).all(), what
    for rec, names in FIELDS:
        g, w = (gp, wp) if rec == "post" else (gc, wc)
        if g is None:
            continue
        for f in names:
            bad = np.flatnonzero((bits(g[f]) != bits(w[f][rows])).reshape(len(rows), -1).any(axis=1))
            assert bad.size == 0, "%s: %s.%s differs at read %d: got %r, want %r" % (what, rec, f, bad[0], g[f][bad[0]],
                                                                                   w[f][rows[bad[0]]])
    if gg is not None:
        assert goff.tolist() == np.concatenate([[0], np.cumsum(wp["n_used"][rows])]).tolist(), what
        for k, r in enumerate(rows):
            a, b = gg[goff[k]:goff[k + 1]], wg[woff[r]:woff[r + 1]]
            assert (bits(a) == bits(b)).all(), "%s: gamma differs at read %d (sample %d)" % (
                what, r, np.flatnonzero((bits(a) != bits(b)).any(axis=1))[0])
        assert not np.isnan(gg).any()


def rows_of(reads, stride=None):
    lens = np.array([len(r) for r in reads], dtype=np.int32)
    stride = stride or max(8, (int(lens.max()) + 7) // 8 * 8)
    buf = np.full((len(reads), stride), -12345, dtype=np.int16)          # (nothing past a read's end may matter)
    for i, r in enumerate(reads):
        buf[i, :len(r)] = r
    return buf, lens


def planted(rng, n):
    """a short direct-RNA-like read of n samples: adapter N(430, 25), poly(A) N(560, 8), a body of levels N(530, 80); and
    two samples far from every state (-300 and 3 000), so that sk_exp's cut-off and the -inf branches run"""
    la, lp = int(n * rng.uniform(0.2, 0.5)), int(n * rng.uniform(0.1, 0.3))
    body = np.repeat(rng.normal(530, 80, n // 8 + 2), 8)[:max(0, n - la - lp)] + rng.normal(0, 8, max(0, n - la - lp))
    x = np.rint(np.concatenate([rng.normal(430, 25, la), rng.normal(560, 8, lp), body])[:n]).astype(np.int16)
    if n >= 20:
        x[rng.integers(0, n)], x[rng.integers(0, n)] = -300, 3000
    return x


@pytest.fixture(scope="module")
def pool():
    """130 planted reads: every length of LENGTHS inside the first group of 64, mixed lengths after it"""
    rng = np.random.default_rng(20261021)
    lengths = list(LENGTHS) + [int(v) for v in rng.choice([0, 3, 40, 100, 130, 200, 260, 300, 400], size=130 - len(LENGTHS))]
    order = rng.permutation(64)
    lengths[:64] = [lengths[i] for i in order]
    return [planted(rng, n) for n in lengths]


@pytest.fixture(scope="module")
def models():
    from squigglekit_amd import api
    out = {"S=1": api.hmm_model([1.0], [[1.0]], [[(0.7, 500.0, 90.0), (0.3, None, 4000.0)]]),
           # a loop 0 -> 1 -> 2 -> 0; a read starts in 0 or 2, never in 1
           "S=3 loop": api.hmm_model([0.6, 0.0, 0.4], [[0.95, 0.05, 0.0], [0.0, 0.9, 0.1], [0.02, 0.0, 0.98]],
                                     [[(1.0, 430.0, 30.0)], [(0.9, 560.0, 10.0), (0.1, None, 4000.0)], [(1.0, 530.0, 90.0)]]),
           "synth_raw": api.polya_model("synth_raw"),
           "rna_pa": api.polya_model("rna_pa"),
           # a dead end: 0 -> 1 and nothing leaves 1, so a read of three samples or more has probability 0
           "dead end": api.HmmModel.from_arrays(2, [0.0, NINF], [[NINF, 0.0], [NINF, NINF]], [[-5.0, NINF], [-5.0, -6.0]],
                                                [[500.0, 0.0], [500.0, 400.0]], [[1e-4, 0.0], [1e-4, 1e-5]])}
    return out


MODEL_NAMES = ["S=1", "S=3 loop", "synth_raw", "rna_pa", "dead end"]


def cal_of(name, R):
    """the calibration pairs a model is run under: rna_pa sees pA (500 raw -> about 95 pA), the rest raw values"""
    if name != "rna_pa":
        return None
    return np.stack([np.arange(R) % 5 + 8.0, np.full(R, 0.1875) + (np.arange(R) % 3) * 0.001], axis=1)


@pytest.fixture(scope="module")
def want(pool, models):
    """the numpy statement's records, counts and dense posteriors of the pool under every model, computed once"""
    buf, lens = rows_of(pool)
    return {name: ref.posterior_batch(m, buf, lens, cal2=cal_of(name, len(pool))) for name, m in models.items()}


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_models_on_the_pool(gpu, pool, models, want, name):
    from squigglekit_amd import api
    buf, lens = rows_of(pool)
    got = api.hmm_posterior_batch(buf, lens, models[name], cal2=cal_of(name, len(pool)), counts=True, dense=True)
    assert got[0].dtype == ref.POST_DTYPE and got[1].dtype == ref.COUNTS_DTYPE
    assert_same(got, want[name], name)
    post = got[0]
    if name == "dead end":
        dead = lens >= 3
        assert (post["flags"][dead] == gpu.SK_HMM_POST_IMPOSSIBLE).all() and (post["loglik"][dead] == NINF).all()
        assert (post["flags"][~dead] == 0).all() and np.isfinite(post["loglik"][~dead]).all()
        assert not post["occ"][dead].any() and not got[1]["xi"][dead].any()
        goff, gamma = got[2], got[3]
        assert not any(gamma[goff[r]:goff[r + 1]].any() for r in np.flatnonzero(dead))
    else:
        assert (post["flags"] == 0).all() and np.isfinite(post["loglik"]).all()
        assert np.abs(post["occ"].sum(axis=1) - lens).max() < 1e-6


def test_empty_and_tiny_reads(gpu, pool, models, want):
    post = want["synth_raw"][0]
    lens = np.array([len(r) for r in pool])
    for n in (0, 1, 2):
        assert (lens == n).any()
    z = post[lens == 0]
    assert (z["loglik"] == 0.0).all() and (z["flags"] == 0).all() and not z["occ"].any() and not z["final_post"].any()


@pytest.mark.parametrize("R", [1, 63, 64, 65, 130])
def test_read_counts(gpu, pool, models, want, R):
    """the lane and group seams: R reads from the end of the pool (so a group starts with other reads than in the pool)"""
    from squigglekit_amd import api
    rows = np.arange(len(pool) - R, len(pool))
    buf, lens = rows_of(pool)
    got = api.hmm_posterior_batch(buf[rows], lens[rows], models["synth_raw"], counts=True, dense=True)
    assert_same(got, want["synth_raw"], "%d reads" % R, rows)


def test_without_counts_and_dense_rows(gpu, pool, models, want):
    """counts = NULL and gamma = NULL: the same records; either alone: the same"""
    from squigglekit_amd import api
    buf, lens = rows_of(pool)
    for counts, dense in ((False, False), (True, False), (False, True)):
        got = api.hmm_posterior_batch(buf, lens, models["synth_raw"], counts=counts, dense=dense)
        assert (got[1] is None) == (not counts) and (got[3] is None) == (not dense)
        assert got[0].tobytes() == want["synth_raw"][0].tobytes(), (counts, dense)
        assert_same(got, want["synth_raw"], "counts %r, dense %r" % (counts, dense))


def test_rows_that_are_not_16_byte_aligned(gpu, pool, models, want):
    """a stride that is no multiple of 8 samples: the 2-byte loads"""
    from squigglekit_amd import api
    buf, lens = rows_of(pool, stride=515)
    got = api.hmm_posterior_batch(buf, lens, models["synth_raw"], counts=True, dense=True)
    assert_same(got, want["synth_raw"], "stride 515")


@pytest.mark.parametrize("limit", [100, 129, 1000])
def test_limit(gpu, pool, models, want, limit):
    """limit below, at and above lengths of the pool"""
    from squigglekit_amd import api
    buf, lens = rows_of(pool)
    rows = np.arange(70)
    theirs = want["synth_raw"] if limit >= lens.max() else ref.posterior_batch(models["synth_raw"], buf[rows], lens[rows],
                                                                               limit=limit)
    got = api.hmm_posterior_batch(buf[rows], lens[rows], models["synth_raw"], limit=limit, counts=True, dense=True)
    assert (got[0]["n_used"] == np.minimum(lens[rows], limit)).all()
    assert_same(got, theirs, "limit %d" % limit, rows if limit >= lens.max() else None)


def test_ragged_float64_gives_the_int16_bytes(gpu, pool, models, want):
    """the float64 feed on the same integer values (tiles of 32: 31 / 32 / 33 are in the pool), and the mixed list"""
    from squigglekit_amd import api
    values, off = api.pack_f64([r.astype(np.float64) for r in pool])
    for name in ("synth_raw", "S=3 loop"):
        got = api.hmm_posterior_ragged_f64(values, off, models[name], counts=True, dense=True)
        assert_same(got, want[name], "float64 feed, " + name)
    mixed = [r.astype(np.float64) + (0.25 if i % 3 == 0 and len(r) else 0.0) for i, r in enumerate(pool[:40])]
    post, cnt, gammas = api.hmm_posterior(mixed, models["synth_raw"], counts=True, dense=True)
    theirs = ref.posterior_reads(models["synth_raw"], mixed)
    assert_same((post, cnt, theirs[2], np.concatenate(gammas)), theirs, "mixed list")
    lim = ref.posterior_reads(models["synth_raw"], mixed, limit=33)
    got = api.hmm_posterior_ragged_f64(*api.pack_f64(mixed), models["synth_raw"], limit=33, counts=True, dense=True)
    assert_same(got, lim, "float64 feed, limit 33")


def device_call(gpu, buf, lens, model, cal=None, limit=0, counts=True, dense=True):
    """sk_hmm_posterior_dev_i16 on uploaded rows; d_gamma has 8 rows of room behind it, every byte 0x5A before the call"""
    L = gpu.load()
    R = len(lens)
    n = np.minimum(np.clip(lens, 0, buf.shape[1]), limit) if limit else np.clip(lens, 0, buf.shape[1])
    goff = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    total = int(goff[R])
    sizes = (buf.nbytes, lens.nbytes, 16 * R, R * 112, R * 624, goff.nbytes, (total + 8) * 48)
    d = [L.sk_dev_alloc(s) for s in sizes]
    try:
        assert all(d)
        gpu.check(L.sk_dev_upload(d[0], gpu.ptr(buf), buf.nbytes))
        gpu.check(L.sk_dev_upload(d[1], gpu.ptr(lens), lens.nbytes))
        if cal is not None:
            gpu.check(L.sk_dev_upload(d[2], gpu.ptr(cal), cal.nbytes))
        gpu.check(L.sk_dev_upload(d[5], gpu.ptr(goff), goff.nbytes))
        mark = np.full((total + 8) * 48, 0x5A, dtype=np.uint8)
        gpu.check(L.sk_dev_upload(d[6], gpu.ptr(mark), mark.nbytes))
        gpu.check(L.sk_hmm_posterior_dev_i16(d[0], buf.shape[1], d[1], R, d[2] if cal is not None else None, C.byref(model),
                                             limit, d[3], d[4] if counts else None, d[5] if dense else None,
                                             d[6] if dense else None))
        gpu.check(L.sk_sync())
        post, cnt = np.zeros(R, dtype=gpu.HMM_POST_DTYPE), np.zeros(R, dtype=gpu.HMM_COUNTS_DTYPE)
        gamma = np.zeros((total + 8, 6))
        for dst, src in ((post, d[3]), (cnt, d[4]), (gamma, d[6])):
            gpu.check(L.sk_dev_download(gpu.ptr(dst), src, dst.nbytes))
        assert (gamma[total:].view(np.uint8) == 0x5A).all(), "the dense rows were written past their end"
        return post, cnt if counts else None, goff if dense else None, gamma[:total] if dense else None
    finally:
        for p in d:
            if p:
                L.sk_dev_free(p)


def test_device_form_equals_the_host_form(gpu, pool, models, want):
    buf, lens = rows_of(pool)
    for name in ("synth_raw", "rna_pa", "dead end"):
        got = device_call(gpu, buf, lens, models[name], cal=cal_of(name, len(pool)))
        assert_same(got, want[name], "device form, " + name)
    post = device_call(gpu, buf, lens, models["synth_raw"], counts=False, dense=False)[0]
    assert post.tobytes() == want["synth_raw"][0].tobytes()


def test_block_sizes_and_slices_give_the_same_bytes(gpu, pool, models, want, monkeypatch):
    """SK_HMM_POST_BLOCK=256: other checkpoints, the same bytes.  SK_HMM_SCRATCH_MB=1: a group's slab alone is 384 KiB
    (768 KiB at B = 256), so the 130 reads take two slices (three at B = 256) -- host form, device form, float64 feed"""
    from squigglekit_amd import api
    buf, lens = rows_of(pool)
    values, off = api.pack_f64([r.astype(np.float64) for r in pool])
    for env in ({"SK_HMM_POST_BLOCK": "256"}, {"SK_HMM_SCRATCH_MB": "1"}, {"SK_HMM_POST_BLOCK": "256", "SK_HMM_SCRATCH_MB": "1"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        try:
            for name in ("synth_raw", "S=3 loop"):
                got = api.hmm_posterior_batch(buf, lens, models[name], counts=True, dense=True)
                assert_same(got, want[name], "%r, %s" % (env, name))
            assert_same(device_call(gpu, buf, lens, models["synth_raw"]), want["synth_raw"], "%r, device form" % env)
            got = api.hmm_posterior_ragged_f64(values, off, models["synth_raw"], counts=True, dense=True)
            assert_same(got, want["synth_raw"], "%r, float64 feed" % env)
        finally:
            for k in env:
                monkeypatch.delenv(k)


def test_sub_batches_equal_one_call(gpu, models, monkeypatch):
    """9 000 reads x stride 128 with SK_INGEST_MB=1: three sub-batches of 3 000 reads, each with its calibration pairs, its
    counts and its dense rows"""
    from squigglekit_amd import api
    rng = np.random.default_rng(5)
    base = np.stack([planted(rng, 128) for _ in range(90)])
    sig = np.tile(base, (100, 1))
    lens = (np.arange(9000) * 37 % 129).astype(np.int32)
    cal = np.stack([(np.arange(9000) % 7).astype(np.float64), np.full(9000, 1.0)], axis=1)
    m = models["synth_raw"]
    one = api.hmm_posterior_batch(sig, lens, m, cal2=cal, counts=True, dense=True)
    monkeypatch.setenv("SK_INGEST_MB", "1")
    three = api.hmm_posterior_batch(sig, lens, m, cal2=cal, counts=True, dense=True)
    monkeypatch.delenv("SK_INGEST_MB")
    assert [a.tobytes() for a in three] == [a.tobytes() for a in one]
    pick = np.array([0, 1, 2999, 3000, 3001, 5999, 6000, 8999])          # ... and both are the definition's
    theirs = ref.posterior_batch(m, sig[pick], lens[pick], cal2=cal[pick])
    goff = one[2]
    got = (one[0][pick], one[1][pick], theirs[2], np.concatenate([one[3][goff[r]:goff[r + 1]] for r in pick]))
    assert_same(got, theirs, "sub-batches")


def test_soft_pool_refit_and_interval(gpu, pool, models, want):
    """hmm_soft_pool over the GPU's counts equals the pool of the statement's; one hmm_fit_em round from the GPU equals
    one with the statement as `decode`; hmm_boundary_interval on the GPU's dense rows"""
    from squigglekit_amd import api
    spec = api.polya_spec("synth_raw")
    reads = [r for r in pool if len(r) >= 100]
    mine, h1 = api.hmm_fit_em(reads, spec, (api.ADAPTER, api.POLYA), 1, min_count=4)
    theirs, h2 = api.hmm_fit_em(reads, spec, (api.ADAPTER, api.POLYA), 1, min_count=4,
                                decode=lambda batch, model, limit: [ref.posterior_reads(model, batch, limit)[:2]])
    assert mine == theirs and h1[0]["loglik"] == h2[0]["loglik"] and h1[0]["reads"] == len(reads)
    for f in ("n", "sum", "sumsq", "trans", "init"):
        assert h1[0]["pooled"][f].tobytes() == h2[0]["pooled"][f].tobytes(), f
    post, _cnt, gammas = api.hmm_posterior(reads[:8], models["synth_raw"], dense=True)
    for g, p in zip(gammas, post):
        lo, hi = api.hmm_boundary_interval(g, (api.POLYA, api.CLIFF, api.TRANSCRIPT))
        assert -1 <= lo and (hi == -1 or lo <= hi < p["n_used"])


def test_the_cut_off_of_sk_exp_is_inclusive(gpu):
    """sk_exp(d) is 0.0 unless d >= -700.0.  Two states that never reach each other, the first with a constant emission
    of 0.0, the second of c: on a read of one sample L = 0.0 (the second term of the sum is absorbed) and the second
    state's posterior is sk_exp(c - 0.0).  c = -700.0 gives 2^-1010 times a polynomial, about 9.86e-305, not 0.0; the
    next double below -700.0 gives 0.0, and so does a second sample (-1 400.0).  No drawn case gets an argument of
    exactly -700.0 outside a sum that absorbs it (tests/RANDOM_CASES_HMMPOST.md), so this model is made by hand.  The
    one-shot call on both feeds and a filtered session, against the statement, by bits."""
    from squigglekit_amd import api
    below = np.nextafter(-700.0, -np.inf)
    edge = float(ref.sk_exp(np.array([-700.0]))[0])
    assert 9.8e-305 < edge < 9.9e-305 and ref.sk_exp(np.array([below]))[0] == 0.0
    reads = [np.array([500], dtype=np.int16), np.array([500, 501], dtype=np.int16), np.zeros(0, dtype=np.int16)]
    buf, lens = rows_of(reads)
    for c, first in ((-700.0, edge), (below, 0.0)):
        arrays = dict(nstates=2, linit=np.zeros(2), ltrans=np.array([[0.0, NINF], [NINF, 0.0]]),
                      c=np.array([[0.0, NINF], [c, NINF]]), mu=np.zeros((2, 2)), h=np.zeros((2, 2)))
        theirs = ref.posterior_batch(arrays, buf, lens)
        assert theirs[0]["loglik"].tolist() == [0.0, 0.0, 0.0] and theirs[3][:, 1].tolist() == [first, 0.0, 0.0]
        assert theirs[0]["occ"][:2, 1].tolist() == [first, 0.0] and theirs[1]["init"][:2, 1].tolist() == [first, 0.0]
        model = api.HmmModel.from_arrays(2, arrays["linit"], arrays["ltrans"], arrays["c"], arrays["mu"], arrays["h"])
        assert_same(api.hmm_posterior_batch(buf, lens, model, counts=True, dense=True), theirs, "c = %r, int16 feed" % c)
        got = api.hmm_posterior_ragged_f64(*api.pack_f64([r.astype(np.float64) for r in reads]), model, counts=True, dense=True)
        assert_same(got, theirs, "c = %r, float64 feed" % c)
        with api.HmmStream(model, 3, filter=True) as hs:
            hs.push([0, 1], reads[:2])
            filt = hs.filter([0, 1, 2])
        assert bits(filt["post"]).tolist() == bits(theirs[0]["final_post"]).tolist() and filt["loglik"].tolist() == [0.0] * 3


def test_three_em_rounds_equal_the_statement(gpu):
    """three rounds of hmm_fit_em on 40 drawn reads of 100 .. 400 samples, from the GPU and with the statement as
    `decode`: the same model, loglik and pooled bytes in every round -- rounds 2 and 3 run under the models the rounds
    before them fitted, which no other test has seen"""
    from squigglekit_amd import api
    rng = np.random.default_rng(20261022)
    reads = [planted(rng, int(n)) for n in rng.integers(100, 401, 40)]
    spec = api.polya_spec("synth_raw")
    mine, h1 = api.hmm_fit_em(reads, spec, (api.ADAPTER, api.POLYA), 3, min_count=4)
    theirs, h2 = api.hmm_fit_em(reads, spec, (api.ADAPTER, api.POLYA), 3, min_count=4,
                                decode=lambda batch, model, limit: [ref.posterior_reads(model, batch, limit)[:2]])
    assert mine == theirs and len(h1) == len(h2) == 3
    for a, b in zip(h1, h2):
        assert a["spec"] == b["spec"] and a["reads"] == b["reads"] == len(reads), a["round"]
        assert np.float64(a["loglik"]).tobytes() == np.float64(b["loglik"]).tobytes(), a["round"]
        for f in ("n", "sum", "sumsq", "trans", "init"):
            assert a["pooled"][f].tobytes() == b["pooled"][f].tobytes(), (a["round"], f)
    assert h1[0]["spec"] != spec and h1[1]["spec"] != h1[0]["spec"] and h1[2]["spec"] != h1[1]["spec"]   # the model moved
    assert h1[0]["loglik"] < h1[1]["loglik"] < h1[2]["loglik"]


def test_cli_posterior_and_interval_columns(gpu, pool, models, tmp_path, capsys):
    """dRNA_polya.py -s --posterior --interval 0.1 on the GPU: the first seven columns are the tool's usual ones, the other
    seven those of the statement's posteriors; a read without samples has `.` throughout"""
    from squigglekit_amd import api, polya_cli
    reads = [pool[i] for i in np.flatnonzero([len(r) >= 200 for r in pool])[:3]]
    reads.insert(1, np.zeros(0, dtype=np.int16))
    path = tmp_path / "raw.tsv"
    path.write_text("".join("f.fast5\tid%d\tx\ty%s\n" % (i, "".join("\t%d" % v for v in r)) for i, r in enumerate(reads)))
    polya_cli.main(["-s", str(path), "--preset", "synth_raw"])
    plain = capsys.readouterr()[0].splitlines()
    polya_cli.main(["-s", str(path), "--preset", "synth_raw", "--posterior", "--interval", "0.1"])
    got = [ln.split("\t") for ln in capsys.readouterr()[0].splitlines()]
    assert ["\t".join(c[:7]) for c in got] == plain and [len(c) for c in got] == [14] * 4
    post, _c, goff, gamma = ref.posterior_reads(models["synth_raw"], reads, counts=False)
    want = polya_cli.posterior_columns(post, [gamma[goff[r]:goff[r + 1]] for r in range(4)], True, 0.1)
    assert [c[7:] for c in got] == want and want[1] == ["."] * 7
