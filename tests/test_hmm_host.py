"""Host: the signal HMM's definition (tests/hmm_ref.py), the model builder, the argument checks and the poly(A) layer.

No GPU: the library is loaded for its argument checks only -- they happen before the device is looked at.
"""
import ctypes as C
import math

import numpy as np
import pytest

import hmm_ref

NINF = -np.inf


def backtrace_viterbi(S, linit, ltrans, c, mu, h, x):
    """Viterbi with stored predecessors and an explicit back-trace, written without looking at hmm_ref: returns
    (score, final_state, path) -- path[t] = the state at sample t -- or None for an empty read."""
    n = len(x)
    if n == 0:
        return None
    gt = lambda a, b: bool(a > b)  # noqa: E731

    def emit(j, xv):
        a = [c[j][m] - ((xv - mu[j][m]) * (xv - mu[j][m])) * h[j][m] for m in range(2)]
        return a[1] if gt(a[1], a[0]) else a[0]
    v = [[0.0] * S for _ in range(n)]
    back = [[0] * S for _ in range(n)]
    with np.errstate(invalid="ignore"):
        for j in range(S):
            v[0][j] = np.float64(linit[j]) + emit(j, np.float64(x[0]))
        for t in range(1, n):
            for j in range(S):
                best, arg = v[t - 1][0] + np.float64(ltrans[0][j]), 0
                for i in range(1, S):
                    cand = v[t - 1][i] + np.float64(ltrans[i][j])
                    if gt(cand, best):
                        best, arg = cand, i
                v[t][j] = best + emit(j, np.float64(x[t]))
                back[t][j] = arg
    f = 0
    for j in range(1, S):
        if gt(v[n - 1][j], v[n - 1][f]):
            f = j
    path = [f]
    for t in range(n - 1, 0, -1):
        path.append(back[t][path[-1]])
    return float(v[n - 1][f]), f, path[::-1]


def enter_of_path(path):
    en = [-1] * 6
    for t, s in enumerate(path):
        if en[s] < 0:
            en[s] = t
    return en


def random_small_case(rng):
    """a model with integer scores (ties everywhere), random -inf patterns, and a short integer read"""
    S = int(rng.integers(1, 7))
    n = int(rng.integers(0, 41))
    linit = rng.integers(-3, 1, S).astype(np.float64)
    linit[rng.random(S) < 0.3] = NINF
    if not np.isfinite(linit).any():
        linit[int(rng.integers(0, S))] = 0.0
    ltrans = rng.integers(-3, 1, (S, S)).astype(np.float64)
    ltrans[rng.random((S, S)) < 0.4] = NINF
    c = rng.integers(-2, 1, (S, 2)).astype(np.float64)
    c[rng.random(S) < 0.5, 1] = NINF
    mu = rng.integers(0, 4, (S, 2)).astype(np.float64)
    h = rng.integers(0, 3, (S, 2)).astype(np.float64)
    x = rng.integers(0, 4, n).astype(np.float64)
    return {"nstates": S, "linit": linit, "ltrans": ltrans, "c": c, "mu": mu, "h": h}, x


def test_ref_equals_backtrace_viterbi():
    """200 random small cases: the forward tuple rule and the tie order against a plain back-trace"""
    rng = np.random.default_rng(20261018)
    ties = 0
    for k in range(200):
        m, x = random_small_case(rng)
        got = hmm_ref.viterbi(m, x)
        want = backtrace_viterbi(m["nstates"], m["linit"], m["ltrans"], m["c"], m["mu"], m["h"], x)
        if want is None:
            assert (got["score"], got["final_state"], got["n_used"]) == (0.0, -1, 0) and (got["enter"] == -1).all(), k
            continue
        score, f, path = want
        assert got["n_used"] == len(x), k
        assert got["final_state"] == f, k
        assert np.float64(got["score"]).tobytes() == np.float64(score).tobytes(), (k, got["score"], score)
        assert got["enter"].tolist() == enter_of_path(path), (k, got["enter"], path)
        ties += 1
    assert ties > 150


def test_ref_batch_forms_agree():
    rng = np.random.default_rng(3)
    m, _ = random_small_case(rng)
    reads = [rng.integers(0, 4, n).astype(np.int16) for n in (0, 1, 5, 17, 40)]
    one = np.array([hmm_ref.viterbi(m, r.astype(np.float64)) for r in reads], dtype=hmm_ref.DTYPE)
    assert hmm_ref.viterbi_reads(m, reads).tobytes() == one.tobytes()
    sig = np.full((5, 48), -12345, dtype=np.int16)
    for i, r in enumerate(reads):
        sig[i, :len(r)] = r
    lens = [len(r) for r in reads]
    assert hmm_ref.viterbi_batch(m, sig, lens).tobytes() == one.tobytes()
    lim = hmm_ref.viterbi_batch(m, sig, lens, limit=5)
    assert lim.tobytes() == hmm_ref.viterbi_reads(m, [r[:5] for r in reads]).tobytes()
    cal = np.tile([2.0, 0.5], (5, 1))
    assert hmm_ref.viterbi_batch(m, sig, lens, cal2=cal).tobytes() == \
        hmm_ref.viterbi_reads(m, [(r.astype(np.float64) + 2.0) * 0.5 for r in reads]).tobytes()


def test_hmm_model_against_hand_computed_values():
    from squigglekit_amd import api
    m = api.hmm_model([1.0, 0.0], [[0.5, 0.5], [0.0, 1.0]],
                      [[(1.0, 10.0, 2.0)], [(0.25, 100.0, 0.5), (0.5, None, 200.0)]])
    a = m.arrays()
    assert a["nstates"] == 2
    assert a["linit"][:2].tolist() == [0.0, NINF]
    assert a["ltrans"][0, :2].tolist() == [math.log(0.5), math.log(0.5)] and a["ltrans"][1, :2].tolist() == [NINF, 0.0]
    # Gaussian: c = log(weight) - log(sigma * sqrt(2 pi)), h = 1 / (2 sigma^2)
    assert a["c"][0, 0] == 0.0 - math.log(2.0 * math.sqrt(2.0 * math.pi)) and a["h"][0, 0] == 0.125 and a["mu"][0, 0] == 10.0
    assert a["c"][1, 0] == math.log(0.25) - math.log(0.5 * math.sqrt(2.0 * math.pi)) and a["h"][1, 0] == 2.0
    assert abs(a["c"][0, 0] - (-1.6120857137646180)) < 1e-15          # -log(2 sqrt(2 pi)), by hand
    # flat: c = log(weight / range), h = 0; absent: c = -inf
    assert a["c"][1, 1] == math.log(0.5 / 200.0) and a["h"][1, 1] == 0.0
    assert a["c"][0, 1] == NINF and a["h"][0, 1] == 0.0
    # everything past S is shut
    assert (a["linit"][2:] == NINF).all() and (a["ltrans"][2:] == NINF).all() and (a["ltrans"][:, 2:] == NINF).all()
    assert C.sizeof(m) == 632 and api.HMM_DTYPE.itemsize == 40 and api.HMM_DTYPE == hmm_ref.DTYPE
    with pytest.raises(ValueError):
        api.hmm_model([1.0] * 7, [[1.0] * 7] * 7, [[(1.0, 0.0, 1.0)]] * 7)
    with pytest.raises(ValueError):
        api.hmm_model([1.0], [[1.0]], [[(1.0, 0.0, 0.0)]])


def good_model():
    from squigglekit_amd import api
    return api.hmm_model([0.5, 0.5], [[0.9, 0.1], [0.0, 1.0]], [[(1.0, 0.0, 1.0)], [(1.0, 5.0, 1.0), (0.1, None, 10.0)]])


def bad_models():
    from squigglekit_amd._lib import HmmModel
    out = {}
    m = good_model(); m.nstates = 0; out["S = 0"] = m
    m = good_model(); m.nstates = 7; out["S = 7"] = m
    m = good_model(); m.mu[1][0] = float("nan"); out["NaN mu"] = m
    m = good_model(); m.mu[0][1] = float("inf"); out["inf mu"] = m
    m = good_model(); m.h[1][0] = -1.0; out["negative h"] = m
    m = good_model(); m.h[0][0] = float("inf"); out["inf h"] = m
    m = good_model(); m.linit[0] = m.linit[1] = NINF; out["all -inf linit"] = m
    m = good_model(); m.c[1][0] = m.c[1][1] = NINF; out["a state with no finite component"] = m
    m = good_model(); m.c[0][0] = float("inf"); out["+inf c"] = m
    m = good_model(); m.ltrans[0][1] = float("nan"); out["NaN ltrans"] = m
    m = good_model(); m.linit[1] = float("inf"); out["+inf linit"] = m
    assert isinstance(m, HmmModel)
    return out


def test_invalid_arguments_return_without_a_device():
    """every SK_ERR_INVALID case comes back before a context is asked for (none exists in this process)"""
    from squigglekit_amd import _lib
    L = _lib.load()
    sig = np.zeros((2, 8), dtype=np.int16)
    lens = np.array([8, 3], dtype=np.int32)
    rec = np.zeros(2, dtype=_lib.HMM_DTYPE)
    vals, off = np.zeros(11), np.array([0, 8, 11], dtype=np.int64)
    p = _lib.ptr

    def calls(m, limit=0, r=rec, ln=lens):
        mp = C.byref(m) if m is not None else None
        rp = p(r) if r is not None else None
        return (L.sk_hmm_viterbi_i16(p(sig), 8, p(ln), 2, None, mp, limit, rp),
                L.sk_hmm_viterbi_dev_i16(p(sig), 8, p(ln), 2, None, mp, limit, rp),
                L.sk_hmm_viterbi_f64_len(p(vals), p(off), 2, mp, limit, rp))
    for what, m in bad_models().items():
        assert calls(m) == (_lib.SK_ERR_INVALID,) * 3, what
        assert b"sk_hmm_model" in L.sk_last_error(), what
    assert calls(None) == (_lib.SK_ERR_INVALID,) * 3
    assert calls(good_model(), limit=-1) == (_lib.SK_ERR_INVALID,) * 3
    assert calls(good_model(), r=None) == (_lib.SK_ERR_INVALID,) * 3
    assert L.sk_hmm_viterbi_i16(p(sig), 8, p(np.array([9, 0], dtype=np.int32)), 2, None, C.byref(good_model()), 0, p(rec)) \
        == _lib.SK_ERR_INVALID                                        # len past the stride (host form)
    assert L.sk_hmm_viterbi_i16(p(sig), 0, p(lens), 2, None, C.byref(good_model()), 0, p(rec)) == _lib.SK_ERR_INVALID
    assert L.sk_hmm_viterbi_f64_len(p(vals), p(off), -1, C.byref(good_model()), 0, p(rec)) == _lib.SK_ERR_INVALID
    if not _lib.is_ready():                  # a good call gets as far as the device -- and none is bound in this process
        assert set(calls(good_model())) == {_lib.SK_ERR_NO_DEVICE}


# ---- the poly(A) layer ------------------------------------------------------------------------------------------
PLANTED_START_MAX, PLANTED_END_MAX = 0, 49            # measured (see test_planted_reads_recover_the_tail)


def planted(seed):
    """adapter N(430, 25) of 1 500 - 6 000 samples, poly(A) N(560, 8) of 300 - 3 000 samples, a squiggle body + 30"""
    from squigglekit_amd import synth
    rng = np.random.default_rng(7000 + seed)
    la, lp = int(rng.integers(1500, 6001)), int(rng.integers(300, 3001))
    body = synth.squiggle_batch(1, 1200, 9000 + seed)[0].astype(np.float64) + 30.0
    sig = np.concatenate([rng.normal(430.0, 25.0, la), rng.normal(560.0, 8.0, lp), body])
    return np.clip(np.rint(sig), -32768, 32767).astype(np.int16), la, lp


@pytest.fixture(scope="module")
def planted_records():
    from squigglekit_amd import api
    reads = [planted(s) for s in range(64)]
    return reads, hmm_ref.viterbi_reads(api.polya_model("synth_raw"), [r[0] for r in reads])


def test_planted_reads_recover_the_tail(planted_records):
    """64 planted reads through the numpy statement with the "synth_raw" preset: all found, polya_start and polya_end
    where they were planted.

    Measured on these 64 seeds with the numpy statement: polya_start is exact on every read (largest error 0 samples);
    polya_end is late by at most 49 samples (a body that begins with levels near 560 reads as tail for a few events) and
    early by at most 2.  The bounds are those figures plus 25 %: 0 samples for the start, 61 for the end."""
    from squigglekit_amd import api
    reads, rec = planted_records
    seg = api.polya_segments(rec)
    assert seg["found"].all()
    es = np.abs(seg["polya_start"] - np.array([la for _, la, _ in reads]))
    ee = np.abs(seg["polya_end"] - np.array([la + lp - 1 for _, la, lp in reads]))
    print("largest |error|: polya_start %d, polya_end %d samples" % (es.max(), ee.max()))
    assert es.max() <= int(PLANTED_START_MAX * 1.25)
    assert ee.max() <= int(PLANTED_END_MAX * 1.25)
    assert (seg["adapter_end"] == seg["polya_start"] - 1).all() and (seg["adapter_start"] >= 0).all()
    assert (seg["polya_samples"] == seg["polya_end"] - seg["polya_start"] + 1).all()


def test_polya_model_shape():
    from squigglekit_amd import api
    for preset in ("rna_pa", "synth_raw"):
        a = api.polya_model(preset).arrays()
        assert a["nstates"] == 6 and api.POLYA_STATES == ("START", "LEADER", "ADAPTER", "POLYA", "CLIFF", "TRANSCRIPT")
        allowed = {(0, 0), (0, 1), (1, 1), (1, 2), (2, 2), (2, 3), (3, 3), (3, 4), (3, 5), (4, 4), (4, 3), (5, 5)}
        for i in range(6):
            for j in range(6):
                assert np.isfinite(a["ltrans"][i, j]) == ((i, j) in allowed), (preset, i, j)
            assert abs(np.exp(a["ltrans"][i]).sum() - 1.0) < 1e-12
        assert np.isfinite(a["linit"]).tolist() == [True, True, False, False, False, False]
        assert a["h"][api.POLYA, 0] > 0 and a["h"][api.POLYA, 1] == 0 and np.isfinite(a["c"][api.POLYA]).all()   # Gaussian + flat
        assert (a["h"][api.TRANSCRIPT] > 0).all() and np.isfinite(a["c"][api.TRANSCRIPT]).all()                   # two Gaussians
    s = api.polya_model("synth_raw").arrays()
    assert s["mu"][api.ADAPTER, 0] == 430.0 and s["h"][api.ADAPTER, 0] == 1.0 / (2 * 25.0 * 25.0)
    assert s["mu"][api.POLYA, 0] == 560.0 and s["h"][api.POLYA, 0] == 1.0 / (2 * 8.0 * 8.0)
    with pytest.raises(ValueError):
        api.polya_model("dna")


def test_polya_segments_and_cli_lines(planted_records):
    """the text of dRNA_polya.py, pinned on records the numpy statement made"""
    from squigglekit_amd import api, polya_cli
    reads, rec = planted_records
    rec = rec[:3].copy()
    rec["final_state"][1] = api.POLYA                                  # a read whose path never reaches the body
    rec["enter"][1][api.TRANSCRIPT] = -1
    lines = polya_cli.polya_lines(["a", "b", 7], rec)
    en = rec["enter"]
    assert lines[0] == "a\t%d\t%d\t%d\t%d\t%d\t%s\n" % (en[0][2], en[0][3] - 1, en[0][3], en[0][5] - 1, en[0][5] - en[0][3],
                                                       repr(float(rec["score"][0]) / int(rec["n_used"][0])))
    assert lines[1] == "b\t.\t.\t.\t.\t0\t%s\n" % repr(float(rec["score"][1]) / int(rec["n_used"][1]))
    assert lines[2].startswith("7\t") and lines[2].count("\t") == 6
    seg = api.polya_segments(rec)
    assert seg["found"].tolist() == [True, False, True]
    assert tuple(seg[1])[:5] == (-1, -1, -1, -1, 0)
    # --rate: two more columns, events as the unit
    rated = polya_cli.polya_lines(["a", "b", 7], rec, rates=[12.0, 12.0, float("nan")])
    assert rated[0] == lines[0][:-1] + "\t12.0\t%s\n" % repr(float(en[0][5] - en[0][3]) / 12.0)
    assert rated[1] == lines[1][:-1] + "\t.\t.\n" and rated[2] == lines[2][:-1] + "\t.\t.\n"
    # samples_per_event: the median length of the events that start at or after the first TRANSCRIPT sample
    t0 = int(en[0][5])
    ev = np.zeros(5, dtype=api.DET_EVENT_DTYPE)
    ev["start"] = [0, t0 - 1, t0, t0 + 9, t0 + 12]
    ev["length"] = [t0 - 1, 1, 9, 3, 30]
    spe = polya_cli.samples_per_event(rec[:2], np.array([0, 5, 5]), ev)
    assert spe[0] == 9.0 and np.isnan(spe[1])
    # an empty read's record
    empty = hmm_ref.viterbi_reads(api.polya_model("synth_raw"), [np.zeros(0)])
    assert polya_cli.polya_lines(["e"], empty) == ["e\t.\t.\t.\t.\t0\t.\n"]


def test_cli_prints_a_line_for_a_read_without_samples(tmp_path, monkeypatch, capsys):
    """dRNA_polya.py -s over a raw TSV, the GPU calls answered by the numpy statements: one line per read, the empty
    read's too (in its place, `.` in every column), and the empty read is sent to neither device call"""
    import detect_ref
    from squigglekit_amd import _lib, api, polya_cli
    monkeypatch.setattr(_lib, "warm_start", lambda *a, **k: None)
    sent = []

    def fake_hmm(reads, model, limit=0):
        sent.append([len(r) for r in reads])
        return hmm_ref.viterbi_reads(model, reads, limit)

    def fake_detect(reads, params=None):
        sent.append([len(r) for r in reads])
        return detect_ref.detect(reads, detect_ref.PRESETS["rna"])
    monkeypatch.setattr(api, "hmm_viterbi", fake_hmm)
    monkeypatch.setattr(api, "detect_events", fake_detect)
    a, b = planted(3)[0], planted(4)[0]
    path = tmp_path / "raw.tsv"
    path.write_text("a.fast5\tid0\tx\ty\t" + "\t".join(str(v) for v in a) + "\n" + "b.fast5\tid1\tx\ty\n"
                    + "c.fast5\tid2\tx\ty\t" + "\t".join(str(v) for v in b) + "\n")
    model = api.polya_model("synth_raw")
    for extra, batch in (([], "2"), (["--rate"], "4096")):
        sent.clear()
        polya_cli.main(["-s", str(path), "--preset", "synth_raw", "--batch", batch] + extra)
        so, se = capsys.readouterr()
        assert se == "dRNA_polya: no samples in read id1 of %s\n" % path
        rec = hmm_ref.viterbi_reads(model, [a, np.zeros(0, dtype=np.int16), b])
        rates = None
        if extra:
            off, ev = detect_ref.detect([a, b], detect_ref.PRESETS["rna"])
            spe = polya_cli.samples_per_event(rec[[0, 2]], off, ev)
            rates = [spe[0], float("nan"), spe[1]]
        assert so == "".join(polya_cli.polya_lines(["id0", "id1", "id2"], rec, rates))
        assert so.splitlines()[1] == "id1\t.\t.\t.\t.\t0\t." + ("\t.\t." if extra else "")
        assert all(n > 0 for call in sent for n in call) and sum(len(call) for call in sent) == (4 if extra else 2)
