"""No GPU: the numpy statement of the signal HMM's posteriors (tests/hmm_post_ref.py) against numpy's exp / log and a plain
scipy.special.logsumexp forward-backward, the ABI's argument checks, the soft-count pooling and Baum-Welch refit with the
statement as `decode`, and the new columns of dRNA_polya.py.  The GPU is compared with the statement bit for bit in
tests/test_gpu_hmm_post.py.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hmm_post_ref as ref
import hmm_ref
from test_hmm_host import bad_models, good_model, planted
from test_hmm_path_host import start_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = -np.inf


def ulps(got, want):
    """|got - want| in units of the spacing of want"""
    return float(np.max(np.abs(got - want) / np.spacing(np.abs(want))))


def test_sk_exp_and_sk_log_against_numpy():
    """Seeded grids: 3 000 000 points of [-700, 0] and 2 000 000 of [1, 6] (default_rng(1)), ends included.

    Measured with numpy 2 on x86-64 (glibc's exp and log, both below 1 ulp): sk_exp is within 1 ulp of np.exp, sk_log
    within 3 ulp of np.log -- its last step adds k * LN2 to a rounded (z + z) * p, three roundings near a result below
    2.  The bounds are those figures plus 1 ulp of slack for other libm builds."""
    rng = np.random.default_rng(1)
    d = -700.0 * rng.random(3_000_000)
    d[:3] = [0.0, -700.0, -1e-300]
    e = ulps(ref.sk_exp(d), np.exp(d))
    s = 1.0 + 5.0 * rng.random(2_000_000)
    s[:3] = [1.0, 6.0, np.nextafter(1.0, 2.0)]
    with np.errstate(invalid="ignore", divide="ignore"):
        lg = np.log(s)
        got = ref.sk_log(s)
        g = float(np.max(np.where(lg > 0, np.abs(got - lg) / np.spacing(np.where(lg > 0, lg, 1.0)), 0.0)))
    print("largest error: sk_exp %.3g ulp, sk_log %.3g ulp" % (e, g))
    assert e <= 1 + 1 and g <= 3 + 1
    assert ref.sk_exp(np.array([0.0]))[0] == 1.0 and ref.sk_log(np.array([1.0]))[0] == 0.0
    assert ref.sk_exp(np.array([NINF, -700.0000001, -1e308]))[0:3].tolist() == [0.0, 0.0, 0.0]
    assert np.signbit(ref.sk_exp(np.array([NINF]))[0]) == False                                   # noqa: E712
    small = ref.sk_exp(np.array([-700.0]))[0]
    assert small > 2.0 ** -1022 and abs(small / np.exp(-700.0) - 1.0) < 1e-15                      # never subnormal
    assert ref.sk_exp(np.array([1e-17]))[0] == 1.0                                                 # a rounding error above 0
    for K in range(1, 7):                                                                          # lse of K equal candidates
        assert abs(ref.lse(np.full((1, K), -3.0), axis=1)[0] - (-3.0 + np.log(K))) < 1e-15
    assert ref.lse(np.array([[NINF, NINF]]), axis=1)[0] == NINF
    assert ref.lse(np.array([[NINF, 2.5, NINF]]), axis=1)[0] == 2.5                                # a -inf candidate adds 0.0


def plain_forward_backward(model, x):
    """(L, gamma [n, S], xi_sum [S, S]) of one read by scipy.special.logsumexp and numpy's exp"""
    from scipy.special import logsumexp
    S, linit, ltrans, c, mu, h = hmm_ref.model_arrays(model)
    e = hmm_ref.emission(c, mu, h, np.asarray(x, dtype=np.float64))
    n = len(x)
    al, be = np.zeros((n, S)), np.zeros((n, S))
    with np.errstate(divide="ignore"):
        al[0] = linit + e[0]
        for t in range(1, n):
            al[t] = logsumexp(al[t - 1][:, None] + ltrans, axis=0) + e[t]
        L = logsumexp(al[n - 1])
        xi = np.zeros((S, S))
        for t in range(n - 2, -1, -1):
            u = ltrans + (e[t + 1] + be[t + 1])[None, :]
            be[t] = logsumexp(u, axis=1)
            xi += np.exp(al[t][:, None] + u - L)
    return L, np.exp(al + be - L), xi


def spiked(seed, n=3200):
    """a planted read cut to n samples (adapter, tail, body) with two spikes, -300 and 3 000"""
    sig, la, lp = planted(seed)
    cut = np.concatenate([sig[:n // 2], sig[la:la + n // 4], sig[la + lp:la + lp + n // 4]]).copy()
    cut[n // 3], cut[n // 2 + 50] = -300, 3000
    return cut


def test_statement_against_a_plain_logsumexp_forward_backward():
    """Two planted reads cut to 3 200 samples with spikes at -300 and 3 000, the "synth_raw" model; and 40 short reads
    under a three-state loop with a -inf linit.

    Measured on the planted reads: loglik equals the scipy route's to the last bit (bound: 4 ulp), gamma differs by at
    most 1.1e-16 (nearly every posterior there is within rounding of 0 or 1), |sum_j gamma_j(t) - 1| is up to 8.8e-10,
    |sum_j occ[j] - n| up to 6.9e-7, the xi row sums differ from occ less the last sample by up to 2.2e-11.  On the
    loop's reads gamma differs by up to 2.3e-13: exp(al + be - L) carries |L| * 2^-53, about 1.3e-13 at |L| = 1 200, in
    its argument on either route.  All of these are rounding errors of log-probabilities of size |L| and grow with it.
    The bounds are the measured values times 4, for other libm and scipy builds."""
    from squigglekit_amd import api
    model = api.polya_model("synth_raw")
    worst = dict(L=0.0, g=0.0, one=0.0, occ=0.0, xi=0.0)
    for seed in (0, 1):
        x = spiked(seed)
        post, cnt, goff, gamma = ref.posterior_reads(model, [x])
        assert not np.isnan(gamma).any() and post["flags"][0] == 0 and post["n_used"][0] == len(x)
        L, g, xi = plain_forward_backward(model, x)
        worst["L"] = max(worst["L"], abs(post["loglik"][0] - L) / abs(L))
        worst["g"] = max(worst["g"], float(np.abs(gamma - g).max()))
        worst["one"] = max(worst["one"], float(np.abs(gamma.sum(axis=1) - 1.0).max()))
        worst["occ"] = max(worst["occ"], abs(float(post["occ"][0].sum()) - len(x)))
        worst["xi"] = max(worst["xi"], float(np.abs(cnt["xi"][0].sum(axis=1) - (post["occ"][0] - post["final_post"][0])).max()))
        assert np.abs(cnt["xi"][0] - xi).max() < 1e-6 * max(1.0, xi.max())
        assert (post["final_post"][0] == gamma[-1]).all() and (cnt["init"][0] == gamma[0]).all()
        assert abs(cnt["n"][0].sum() - len(x)) < 1e-5 and np.allclose(cnt["n"][0].sum(axis=1), post["occ"][0], rtol=0, atol=1e-6)
        assert abs(cnt["sx"][0].sum() - float(x.sum())) < 1e-3 and abs(cnt["sxx"][0].sum() / float((x.astype(np.float64) ** 2).sum()) - 1) < 1e-9
    print("planted reads:", worst)
    assert worst["L"] <= 4 * 2.0 ** -52 and worst["g"] <= 4 * 1.2e-16 and worst["one"] <= 4 * 8.8e-10
    assert worst["occ"] <= 4 * 6.9e-7 and worst["xi"] <= 4 * 2.2e-11
    loop = api.hmm_model([0.6, 0.0, 0.4], [[0.95, 0.05, 0.0], [0.0, 0.9, 0.1], [0.02, 0.0, 0.98]],
                         [[(1.0, 430.0, 30.0)], [(0.9, 560.0, 10.0), (0.1, None, 4000.0)], [(1.0, 530.0, 90.0)]])
    rng = np.random.default_rng(3)
    reads = [np.rint(rng.normal(500, 60, n)) for n in rng.integers(1, 200, 40)]
    post, cnt, goff, gamma = ref.posterior_reads(loop, reads)
    w2 = 0.0
    for r, x in enumerate(reads):
        L, g, xi = plain_forward_backward(loop, x)
        assert abs(post["loglik"][r] - L) <= 4 * np.spacing(abs(L))
        w2 = max(w2, float(np.abs(gamma[goff[r]:goff[r + 1], :3] - g).max()))
        assert not gamma[goff[r]:goff[r + 1], 3:].any()
    print("three-state loop: gamma differs by at most %.3g" % w2)
    assert w2 <= 4 * 2.3e-13


def test_empty_impossible_and_limit():
    from squigglekit_amd import api
    dead = api.HmmModel.from_arrays(2, [0.0, NINF], [[NINF, 0.0], [NINF, NINF]], [[-5.0, NINF], [-5.0, -6.0]],
                                    [[500.0, 0.0], [500.0, 400.0]], [[1e-4, 0.0], [1e-4, 1e-5]])
    reads = [np.zeros(0), np.array([500.0]), np.array([500.0, 400.0]), np.array([500.0, 400.0, 450.0]), np.full(9, 480.0)]
    post, cnt, goff, gamma = ref.posterior_reads(dead, reads)
    assert post["flags"].tolist() == [0, 0, 0, ref.IMPOSSIBLE, ref.IMPOSSIBLE]
    assert post["loglik"][0] == 0.0 and np.isfinite(post["loglik"][1:3]).all() and (post["loglik"][3:] == NINF).all()
    assert not gamma[goff[3]:].any() and not post["occ"][3:].any() and not cnt[3:].tobytes().strip(b"\0")
    assert gamma[:3].tolist() == [[1, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0]] and not np.isnan(gamma).any()
    assert cnt["xi"][2][0][1] == 1.0 and cnt["xi"][2].sum() == 1.0
    lim = ref.posterior_reads(dead, reads, limit=2)
    assert lim[0]["n_used"].tolist() == [0, 1, 2, 2, 2] and (lim[0]["flags"] == 0).all()
    assert lim[0][2].tobytes() == post[2].tobytes() and lim[3][lim[2][3]:lim[2][4]].tolist() == gamma[1:3].tolist()


def test_layouts_and_symbols():
    from squigglekit_amd import _lib, api
    assert api.HMM_POST_DTYPE == ref.POST_DTYPE and api.HMM_POST_DTYPE.itemsize == 112
    assert api.HMM_COUNTS_DTYPE == ref.COUNTS_DTYPE and api.HMM_COUNTS_DTYPE.itemsize == 624
    assert [api.HMM_POST_DTYPE.fields[f][1] for f in ("loglik", "n_used", "flags", "final_post", "occ")] == [0, 8, 12, 16, 64]
    assert [api.HMM_COUNTS_DTYPE.fields[f][1] for f in ("n", "sx", "sxx", "xi", "init")] == [0, 96, 192, 288, 576]
    assert _lib.SK_HMM_POST_IMPOSSIBLE == ref.IMPOSSIBLE == 1
    header = open(os.path.join(ROOT, "include", "squigglekit_hip.h")).read()
    assert re.search(r"#define SK_HMM_POST_IMPOSSIBLE 1\b", header)
    assert re.search(r"typedef struct sk_hmm_post \{\s*/\* 112 bytes \*/\s*double  loglik;\s*int32_t n_used, flags;\s*"
                     r"double  final_post\[SK_HMM_STATES\];\s*double  occ\[SK_HMM_STATES\];\s*\} sk_hmm_post;", header)
    assert re.search(r"typedef struct sk_hmm_counts \{\s*/\* 624 bytes \*/", header)
    L = _lib.load()
    for name in ("sk_hmm_posterior_i16", "sk_hmm_posterior_dev_i16", "sk_hmm_posterior_f64_len"):
        assert name in _lib.ABI and getattr(L, name).argtypes == _lib.ABI[name][1], name
        assert re.search(r"\bint %s\(" % name, header), name
    # the constants of the header, the kernel and the statement are the same bit patterns
    kernel = open(os.path.join(ROOT, "squigglekit_amd", "csrc", "sk_hmm_post.hip")).read()
    consts = [ref.LOG2E, ref.LN2_HI, ref.LN2_LO, ref.SQRT2, ref.LN2] + ref.EXP_C + ref.LOG_D
    for v in consts:
        pat = "0x%016X" % np.array([v]).view(np.uint64)[0]
        assert pat in header and pat in kernel, pat
    from fractions import Fraction
    from math import factorial
    assert ref.EXP_C == [float(Fraction(1, factorial(q))) for q in range(14)]
    assert ref.LOG_D == [float(Fraction(1, q)) for q in range(1, 24, 2)]


def test_invalid_arguments_return_without_a_device():
    """every SK_ERR_INVALID case of the three entry points comes back before a context is asked for"""
    from squigglekit_amd import _lib
    L = _lib.load()
    sig = np.zeros((2, 8), dtype=np.int16)
    lens = np.array([8, 3], dtype=np.int32)
    post = np.zeros(2, dtype=_lib.HMM_POST_DTYPE)
    cnt = np.zeros(2, dtype=_lib.HMM_COUNTS_DTYPE)
    goff = np.array([0, 8, 11], dtype=np.int64)
    gamma = np.zeros((11, 6))
    vals, voff = np.zeros(11), np.array([0, 8, 11], dtype=np.int64)
    p = _lib.ptr

    def calls(m, limit=0, po=post, ln=lens, c=cnt, go=goff, ga=gamma, stride=8, nreads=2):
        mp = C.byref(m) if m is not None else None
        pp, cp, gop, gap = (p(v) if v is not None else None for v in (po, c, go, ga))
        return (L.sk_hmm_posterior_i16(p(sig), stride, p(ln), nreads, None, mp, limit, pp, cp, gop, gap),
                L.sk_hmm_posterior_dev_i16(p(sig), stride, p(ln), nreads, None, mp, limit, pp, cp, gop, gap),
                L.sk_hmm_posterior_f64_len(p(vals), p(voff), nreads, mp, limit, pp, cp, gop, gap))
    inv = (_lib.SK_ERR_INVALID,) * 3
    for what, m in bad_models().items():
        assert calls(m) == inv, what
        assert b"sk_hmm_model" in L.sk_last_error(), what
    assert calls(None) == inv
    assert calls(good_model(), limit=-1) == inv
    assert calls(good_model(), po=None) == inv
    assert calls(good_model(), go=None) == inv                                       # gamma without goff
    assert calls(good_model(), ga=None) == inv                                       # goff without gamma
    assert calls(good_model(), nreads=-1) == inv
    g = C.byref(good_model())
    tail = (g, 0, p(post), p(cnt), p(goff), p(gamma))
    assert L.sk_hmm_posterior_i16(p(sig), 8, p(np.array([9, 0], dtype=np.int32)), 2, None, *tail) == _lib.SK_ERR_INVALID
    assert L.sk_hmm_posterior_i16(p(sig), 0, p(lens), 2, None, *tail) == _lib.SK_ERR_INVALID
    assert L.sk_hmm_posterior_dev_i16(None, 8, p(lens), 2, None, *tail) == _lib.SK_ERR_INVALID
    assert L.sk_hmm_posterior_f64_len(None, p(voff), 2, *tail) == _lib.SK_ERR_INVALID
    assert L.sk_hmm_posterior_f64_len(p(vals), None, 2, *tail) == _lib.SK_ERR_INVALID
    assert L.sk_hmm_posterior_f64_len(p(vals), p(np.array([0, 8, 7], dtype=np.int64)), 2, *tail) == _lib.SK_ERR_INVALID
    # the host forms: a goff that is not the running sum of the samples used, from 0
    for bad in ([1, 9, 12], [0, 8, 12], [0, 7, 10]):
        b = p(np.array(bad, dtype=np.int64))
        assert L.sk_hmm_posterior_i16(p(sig), 8, p(lens), 2, None, g, 0, p(post), p(cnt), b, p(gamma)) == _lib.SK_ERR_INVALID
        assert L.sk_hmm_posterior_f64_len(p(vals), p(voff), 2, g, 0, p(post), p(cnt), b, p(gamma)) == _lib.SK_ERR_INVALID
    assert L.sk_hmm_posterior_i16(p(sig), 8, p(lens), 2, None, g, 5, p(post), p(cnt), p(goff), p(gamma)) == _lib.SK_ERR_INVALID
    if not _lib.is_ready():                  # a good call gets as far as the device -- and none is bound in this process
        assert set(calls(good_model())) == {_lib.SK_ERR_NO_DEVICE}
        assert set(calls(good_model(), c=None, go=None, ga=None)) == {_lib.SK_ERR_NO_DEVICE}
        lim = p(np.array([0, 5, 8], dtype=np.int64))                                 # limit 5: the reads use 5 and 3 samples
        assert L.sk_hmm_posterior_i16(p(sig), 8, p(lens), 2, None, g, 5, p(post), p(cnt), lim, p(gamma)) == _lib.SK_ERR_NO_DEVICE


def short(seed):
    """a planted read cut down: 300 samples of adapter, 200 of tail, 400 of body"""
    sig, la, lp = planted(seed)
    return np.concatenate([sig[:300], sig[la:la + 200], sig[la + lp:la + lp + 400]])


def cut(seed):
    """a planted read cut down for the refit: 400 samples of adapter, up to 800 of tail, 200 of body.  (With the tail
    shorter than the body -- `short` -- POLYA at N(545, 16) settles on the body's levels instead: a local optimum.)"""
    sig, la, lp = planted(seed)
    return np.concatenate([sig[:400], sig[la:la + min(lp, 800)], sig[la + lp:la + lp + 200]])


def ref_decode(batch, model, limit):
    yield ref.posterior_reads(model, batch, limit, dense=False)[:2]


def test_soft_pool_and_em_refit_move_toward_the_planted_levels():
    """The 64 planted reads of test_hmm_host cut to at most 1 400 samples (400 of adapter, up to 800 of tail, 200 of body), the
    "synth_raw" description with ADAPTER set to (0.98, 455, 40) and POLYA to (0.98, 545, 16) as test_hmm_path_host starts
    from; three rounds of hmm_fit_em over (ADAPTER, POLYA) with update ("mean", "sigma"), decoded by the numpy statement.

    Measured: after three rounds POLYA 559.999 / 8.017 and ADAPTER 430.054 / 25.063 (planted: 560 / 8 and 430 / 25), i.e.
    errors of 0.0011, 0.0167, 0.0538 and 0.0635; the total loglik rises every round (-402 574.5, -376 060.6, -366 884.9).
    The bounds are those errors plus 25 %; the start lies 15, 8, 25 and 15 away."""
    from squigglekit_amd import api
    sigs = [cut(s) for s in range(64)]
    total = sum(len(x) for x in sigs)
    spec0 = start_spec()
    model0 = api.hmm_model(*spec0)
    post, counts = next(ref_decode(sigs, model0, 0))
    pooled = api.hmm_soft_pool(post, counts, 6)
    assert pooled["reads"] == 64 and isinstance(pooled["reads"], int)
    for f, shape in (("n", (6, 2)), ("sum", (6, 2)), ("sumsq", (6, 2)), ("trans", (6, 6)), ("init", (6,))):
        assert pooled[f].dtype == np.float64 and pooled[f].shape == shape, f
    assert abs(pooled["n"].sum() - total) < 1e-3 and abs(pooled["init"].sum() - 64) < 1e-6
    assert abs(pooled["trans"].sum() - (total - 64)) < 1e-3
    both = api.hmm_pool_add(pooled, pooled)
    assert both["reads"] == 128 and (both["n"] == 2 * pooled["n"]).all()
    hard = {"n": np.ones((6, 2), dtype=np.int64), "sum": np.ones((6, 2), dtype=np.int64), "sumsq": np.ones((6, 2), dtype=np.int64),
            "trans": np.ones((6, 6), dtype=np.int64), "init": np.ones(6, dtype=np.int64), "reads": 1}
    assert api.hmm_pool_add(hard, pooled)["n"].dtype == np.float64                      # soft and hard counts add up
    one = api.hmm_refit(spec0, pooled, (api.ADAPTER, api.POLYA))
    spec, history = api.hmm_fit_em(sigs, spec0, (api.ADAPTER, api.POLYA), 3, decode=ref_decode)
    assert len(history) == 3 and history[0]["spec"] == one and history[0]["reads"] == 64
    assert history[0]["loglik"] == float(post["loglik"].sum())
    for h in history:
        e = h["spec"][2]
        print("round %d: loglik %.1f, POLYA %.3f / %.3f, ADAPTER %.3f / %.3f" % (
            h["round"] + 1, h["loglik"], e[api.POLYA][0][1], e[api.POLYA][0][2], e[api.ADAPTER][0][1], e[api.ADAPTER][0][2]))
    assert history[0]["loglik"] < history[1]["loglik"] < history[2]["loglik"]
    bounds = {api.POLYA: (560.0, 8.0, 0.0011 * 1.25, 0.0167 * 1.25), api.ADAPTER: (430.0, 25.0, 0.0538 * 1.25, 0.0635 * 1.25)}
    for k, (mu, sd, bm, bs) in bounds.items():
        print("state %d: |mean - planted| %.6f, |sigma - planted| %.6f" % (k, abs(spec[2][k][0][1] - mu), abs(spec[2][k][0][2] - sd)))
        assert abs(spec0[2][k][0][1] - mu) > 1.0 and abs(spec0[2][k][0][2] - sd) > 1.0        # the start: far outside
        assert abs(spec[2][k][0][1] - mu) <= bm and abs(spec[2][k][0][2] - sd) <= bs, (k, spec[2][k])
    # only what was named moved
    assert spec[0] == spec0[0] and spec[1] == spec0[1]
    for k in range(6):
        if k not in bounds:
            assert spec[2][k] == spec0[2][k]
    # soft counts keep the transitions well behaved: rows sum to 1, forbidden stay forbidden
    t = api.hmm_refit(spec0, pooled, range(6), update=("trans",), min_count=1)
    for i in range(6):
        assert abs(sum(t[1][i]) - 1.0) < 1e-12 and all((a == 0.0) == (b == 0.0) for a, b in zip(t[1][i], spec0[1][i]))
    with pytest.raises(ValueError):
        api.hmm_fit_em([], spec0, (api.POLYA,), 1, decode=lambda *a: [])


def test_boundary_interval():
    from squigglekit_amd import api
    g = np.zeros((6, 6))
    g[:, 3] = [0.0, 0.04, 0.3, 0.5, 0.96, 1.0]
    g[:, 5] = [0.0, 0.02, 0.1, 0.2, 0.0, 0.0]
    assert api.hmm_boundary_interval(g, (3,)) == (2, 4)
    assert api.hmm_boundary_interval(g, (3, 5)) == (1, 4)
    assert api.hmm_boundary_interval(g, (3, 5), lo=0.5, hi=0.99) == (3, 5)
    assert api.hmm_boundary_interval(g, (5,), lo=0.05, hi=0.95) == (2, -1)
    assert api.hmm_boundary_interval(np.zeros((0, 6)), (3,)) == (-1, -1)


def test_cli_posterior_interval_and_em(tmp_path, monkeypatch, capsys):
    """dRNA_polya.py -s over a raw TSV, the GPU calls answered by the numpy statements: without the new flags the lines
    are polya_lines' as before; --posterior appends three columns, --interval Q four; --refit N --em writes hmm_fit_em's
    model.  The tool writes no header, so only the column count changes."""
    from squigglekit_amd import _lib, api, polya_cli
    monkeypatch.setattr(_lib, "warm_start", lambda *a, **k: None)
    calls = []

    def fake_post(sig, lens, model, cal2=None, limit=0, counts=False, dense=False):
        calls.append((counts, dense))
        return ref.posterior_batch(model, sig, lens, cal2, limit, counts, dense)
    monkeypatch.setattr(api, "hmm_posterior_batch", fake_post)
    monkeypatch.setattr(api, "hmm_posterior_ragged_f64", lambda *a, **k: pytest.fail("integer reads take the int16 feed"))
    monkeypatch.setattr(api, "hmm_viterbi", lambda reads, model, limit=0: hmm_ref.viterbi_reads(model, reads, limit))
    a, b = short(3), short(4)
    path = tmp_path / "raw.tsv"
    path.write_text("a.fast5\tid0\tx\ty\t" + "\t".join(str(v) for v in a) + "\n" + "b.fast5\tid1\tx\ty\n"
                    + "c.fast5\tid2\tx\ty\t" + "\t".join(str(v) for v in b) + "\n")
    model = api.polya_model("synth_raw")
    names = ["id0", "id1", "id2"]
    rec = hmm_ref.viterbi_reads(model, [a, np.zeros(0, dtype=np.int16), b])
    plain = "".join(polya_cli.polya_lines(names, rec))
    polya_cli.main(["-s", str(path), "--preset", "synth_raw"])
    assert capsys.readouterr()[0] == plain and not calls                         # without the flags: today's bytes
    post, _c, goff, gamma = ref.posterior_reads(model, [a, np.zeros(0), b])
    for batch in ("2", "4096"):
        polya_cli.main(["-s", str(path), "--preset", "synth_raw", "--batch", batch, "--posterior", "--interval", "0.05"])
        so = capsys.readouterr()[0].splitlines()
        assert [ln.split("\t")[:7] for ln in so] == [ln.split("\t") for ln in plain.splitlines()]
        assert [len(ln.split("\t")) for ln in so] == [14, 14, 14]
        assert so[1].split("\t")[7:] == ["."] * 7
        for r in (0, 2):
            cols = so[r].split("\t")[7:]
            assert cols[:3] == ["{}".format(float(post["loglik"][r]) / 900), "{}".format(float(post["occ"][r][api.POLYA])),
                                "{}".format(float(post["final_post"][r][api.TRANSCRIPT]))]
            g = gamma[goff[r]:goff[r + 1]]
            iv = api.hmm_boundary_interval(g, (3, 4, 5), 0.05, 0.95) + api.hmm_boundary_interval(g, (5,), 0.05, 0.95)
            assert cols[3:] == [str(v) for v in iv]
            assert 290 <= iv[0] <= iv[1] <= 310 and 490 <= iv[2] <= iv[3] <= 560  # the tail was planted at [300, 500)
            assert abs(float(cols[1]) - 200) < 60 and float(cols[2]) > 0.99
    assert all(c == (False, True) for c in calls)
    polya_cli.main(["-s", str(path), "--preset", "synth_raw", "--posterior"])
    assert [len(ln.split("\t")) for ln in capsys.readouterr()[0].splitlines()] == [10, 10, 10] and calls[-1] == (False, False)
    # --refit N --em: the model written is hmm_fit_em's
    out_json = tmp_path / "fit.json"
    start = tmp_path / "start.json"
    start.write_text(api.hmm_spec_to_json(start_spec()))
    polya_cli.main(["-s", str(path), "--preset", "synth_raw", "--model", str(start), "--refit", "2", "--em", "--states", "2,3",
                    "--model_out", str(out_json), "--fit_only"])
    assert capsys.readouterr()[0] == "" and calls[-1] == (True, False)
    want_spec, _h = api.hmm_fit_em([a, b], start_spec(), (api.ADAPTER, api.POLYA), 2, decode=ref_decode)
    assert api.hmm_spec_from_json(out_json.read_text()) == (want_spec[0], want_spec[1], [list(c) for c in want_spec[2]])
    for bad in (["--em"], ["--interval", "0.7"], ["--refit", "1", "--em"]):
        with pytest.raises(SystemExit):
            polya_cli.main(["-s", str(path)] + bad)
    two = tmp_path / "two.json"
    two.write_text(api.hmm_spec_to_json(([1.0, 0.0], [[0.9, 0.1], [0.0, 1.0]], [[(1.0, 430.0, 30.0)], [(1.0, 530.0, 90.0)]])))
    with pytest.raises(SystemExit):
        polya_cli.main(["-s", str(path), "--preset", "synth_raw", "--model", str(two), "--posterior"])
