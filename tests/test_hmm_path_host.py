"""Host: the state paths' definition (tests/hmm_path_ref.py), the record layouts, the argument checks of the three
sk_hmm_segments_* entry points, the model descriptions and the re-estimation.

No GPU: the library is loaded for its argument checks only -- they happen before the device is looked at.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hmm_path_ref
import hmm_ref
from test_hmm_host import PLANTED_END_MAX, bad_models, good_model, planted, random_small_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = -np.inf


def scalar_segments(S, linit, ltrans, c, mu, h, x):
    """Viterbi with stored predecessors, a back-trace, the cut into runs and the per-component sums, one sample and one
    state at a time, written without looking at hmm_path_ref: a list of (state, start, length, n1, sum0, sum1, sq0, sq1)"""
    n = len(x)
    if n == 0:
        return []

    def comps(j, xv):
        return [c[j][m] - ((xv - mu[j][m]) * (xv - mu[j][m])) * h[j][m] for m in range(2)]
    prev = [0.0] * S
    back = [[0] * S for _ in range(n)]
    with np.errstate(invalid="ignore"):
        for j in range(S):
            a = comps(j, np.float64(x[0]))
            prev[j] = np.float64(linit[j]) + (a[1] if a[1] > a[0] else a[0])
        for t in range(1, n):
            cur = [0.0] * S
            for j in range(S):
                best, who = prev[0] + np.float64(ltrans[0][j]), 0
                for i in range(1, S):
                    cand = prev[i] + np.float64(ltrans[i][j])
                    if cand > best:
                        best, who = cand, i
                a = comps(j, np.float64(x[t]))
                cur[j] = best + (a[1] if a[1] > a[0] else a[0])
                back[t][j] = who
            prev = cur
    f = 0
    for j in range(1, S):
        if prev[j] > prev[f]:
            f = j
    path = [0] * n
    path[n - 1] = f
    for t in range(n - 1, 0, -1):
        path[t - 1] = back[t][path[t]]
    out = []
    t = 0
    while t < n:
        e = t
        while e < n and path[e] == path[t]:
            e += 1
        n1, sm, sq = 0, [0, 0], [0, 0]
        for u in range(t, e):
            with np.errstate(invalid="ignore"):
                a = comps(path[t], np.float64(x[u]))
            m = 1 if a[1] > a[0] else 0
            n1 += m
            sm[m] += int(x[u])
            sq[m] += int(x[u]) * int(x[u])
        out.append((path[t], t, e - t, n1, sm[0], sm[1], sq[0], sq[1]))
        t = e
    return out


def as_tuples(seg):
    return [(int(e["state"]), int(e["start"]), int(e["length"]), int(e["n1"]), e["sum"][0], e["sum"][1], e["sumsq"][0],
             e["sumsq"][1]) for e in seg]


def test_statement_equals_an_independent_back_trace():
    """200 tie-heavy random small cases (integer scores, -inf patterns, S = 1 .. 6, n = 0 .. 40): states, starts, lengths,
    n1 and sums of both feeds' records against the scalar back-trace, and the five invariants on every case"""
    rng = np.random.default_rng(20261019)
    multi = 0
    for k in range(200):
        m, x = random_small_case(rng)
        want = scalar_segments(m["nstates"], m["linit"], m["ltrans"], m["c"], m["mu"], m["h"], x)
        for raw in (True, False):
            rec, off, seg = hmm_path_ref.segments_reads(m, [x], raw=raw)
            assert off.tolist() == [0, len(want)], k
            assert seg.dtype == (hmm_path_ref.SEG_DTYPE if raw else hmm_path_ref.SEGF_DTYPE)
            assert as_tuples(seg) == want, (k, raw)
            assert rec.tobytes() == hmm_ref.viterbi_reads(m, [x]).tobytes(), k
            hmm_path_ref.invariants(m, rec, off, seg)
        multi += len(want) > 1
    assert multi > 50


def test_statement_batch_forms_agree():
    rng = np.random.default_rng(4)
    m, _ = random_small_case(rng)
    reads = [rng.integers(0, 4, n).astype(np.int16) for n in (0, 1, 5, 17, 40)]
    rec, off, seg = hmm_path_ref.segments_reads(m, reads, raw=True)
    sig = np.full((5, 48), -12345, dtype=np.int16)
    for i, r in enumerate(reads):
        sig[i, :len(r)] = r
    lens = [len(r) for r in reads]
    got = hmm_path_ref.segments_batch(m, sig, lens)
    assert [a.tobytes() for a in got] == [rec.tobytes(), off.tobytes(), seg.tobytes()]
    for i, r in enumerate(reads):                                      # ... and read by read
        one = hmm_path_ref.segments_reads(m, [r], raw=True)
        assert one[2].tobytes() == seg[off[i]:off[i + 1]].tobytes(), i
    lim = hmm_path_ref.segments_batch(m, sig, lens, limit=5)
    assert lim[2].tobytes() == hmm_path_ref.segments_reads(m, [r[:5] for r in reads], raw=True)[2].tobytes()
    # a calibration moves the decisions and leaves the sums raw
    cal = np.tile([2.0, 0.5], (5, 1))
    c_rec, c_off, c_seg = hmm_path_ref.segments_batch(m, sig, lens, cal2=cal)
    f_rec, f_off, f_seg = hmm_path_ref.segments_reads(m, [(r.astype(np.float64) + 2.0) * 0.5 for r in reads])
    assert c_rec.tobytes() == f_rec.tobytes() and c_off.tobytes() == f_off.tobytes()
    for f in ("state", "start", "length", "n1"):
        assert (c_seg[f] == f_seg[f]).all(), f
    for i in range(5):
        g = c_seg[c_off[i]:c_off[i + 1]]
        assert g["sum"].sum() == int(reads[i].astype(np.int64).sum())
        assert g["sumsq"].sum() == int((reads[i].astype(np.int64) ** 2).sum())


def test_layouts_and_symbols():
    from squigglekit_amd import _lib, api
    for dt, ref, kind in ((api.HMM_SEG_DTYPE, hmm_path_ref.SEG_DTYPE, "<i8"), (api.HMM_SEGF_DTYPE, hmm_path_ref.SEGF_DTYPE, "<f8")):
        assert dt == ref and dt.itemsize == 48
        assert [dt.fields[f][1] for f in ("state", "start", "length", "n1", "sum", "sumsq")] == [0, 4, 8, 12, 16, 32]
        assert dt.fields["sum"][0] == np.dtype((kind, (2,))) and dt.fields["sumsq"][0] == np.dtype((kind, (2,)))
    header = open(os.path.join(ROOT, "include", "squigglekit_hip.h")).read()
    body = re.search(r"typedef struct sk_hmm_seg \{\s*/\* 48 bytes \*/(.*?)\} sk_hmm_seg;", header, re.S).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "int32_t state, start, length, n1; int64_t sum[2], sumsq[2];"
    assert re.search(r"typedef struct sk_hmm_segf \{.*?int32_t state, start, length, n1;\s*double  sum\[2\], sumsq\[2\];\s*\} sk_hmm_segf;",
                     header, re.S)
    L = _lib.load()
    for name in ("sk_hmm_segments_i16", "sk_hmm_segments_dev_i16", "sk_hmm_segments_f64_len"):
        assert name in _lib.ABI and getattr(L, name).argtypes == _lib.ABI[name][1], name
        assert re.search(r"\bint %s\(" % name, header), name


def test_invalid_arguments_return_without_a_device():
    """every SK_ERR_INVALID case of the three entry points comes back before a context is asked for"""
    from squigglekit_amd import _lib
    L = _lib.load()
    sig = np.zeros((2, 8), dtype=np.int16)
    lens = np.array([8, 3], dtype=np.int32)
    rec = np.zeros(2, dtype=_lib.HMM_DTYPE)
    off = np.zeros(3, dtype=np.int64)
    seg = np.zeros(8, dtype=_lib.HMM_SEG_DTYPE)
    vals, voff = np.zeros(11), np.array([0, 8, 11], dtype=np.int64)
    p = _lib.ptr

    def calls(m, limit=0, r=rec, ln=lens, o=off, s=seg, cap=8, stride=8, nreads=2):
        mp = C.byref(m) if m is not None else None
        rp, op, sp = (p(v) if v is not None else None for v in (r, o, s))
        return (L.sk_hmm_segments_i16(p(sig), stride, p(ln), nreads, None, mp, limit, rp, op, sp, cap),
                L.sk_hmm_segments_dev_i16(p(sig), stride, p(ln), nreads, None, mp, limit, rp, op, sp, cap),
                L.sk_hmm_segments_f64_len(p(vals), p(voff), nreads, mp, limit, rp, op, sp, cap))
    inv = (_lib.SK_ERR_INVALID,) * 3
    for what, m in bad_models().items():
        assert calls(m) == inv, what
        assert b"sk_hmm_model" in L.sk_last_error(), what
    assert calls(None) == inv
    assert calls(good_model(), limit=-1) == inv
    assert calls(good_model(), r=None) == inv
    assert calls(good_model(), o=None) == inv                                        # NULL off
    assert calls(good_model(), s=None) == inv                                        # seg == NULL with cap > 0
    assert calls(good_model(), cap=-1) == inv
    assert calls(good_model(), s=None, cap=-1) == inv
    assert calls(good_model(), nreads=-1) == inv
    g = C.byref(good_model())
    assert L.sk_hmm_segments_i16(p(sig), 8, p(np.array([9, 0], dtype=np.int32)), 2, None, g, 0, p(rec), p(off), p(seg), 8) \
        == _lib.SK_ERR_INVALID                                                   # len past the stride (host form)
    assert L.sk_hmm_segments_i16(p(sig), 0, p(lens), 2, None, g, 0, p(rec), p(off), p(seg), 8) == _lib.SK_ERR_INVALID
    assert L.sk_hmm_segments_dev_i16(None, 8, p(lens), 2, None, g, 0, p(rec), p(off), p(seg), 8) == _lib.SK_ERR_INVALID
    assert L.sk_hmm_segments_f64_len(None, p(voff), 2, g, 0, p(rec), p(off), p(seg), 8) == _lib.SK_ERR_INVALID
    assert L.sk_hmm_segments_f64_len(p(vals), None, 2, g, 0, p(rec), p(off), p(seg), 8) == _lib.SK_ERR_INVALID
    if not _lib.is_ready():                  # a good call gets as far as the device -- and none is bound in this process
        assert set(calls(good_model())) == {_lib.SK_ERR_NO_DEVICE}
        assert set(calls(good_model(), s=None, cap=0)) == {_lib.SK_ERR_NO_DEVICE}    # the counting call is a good call


def test_spec_and_json():
    from squigglekit_amd import api
    for preset in ("rna_pa", "synth_raw"):
        spec = api.polya_spec(preset)
        assert bytes(api.polya_model(preset)) == bytes(api.hmm_model(*spec)), preset
        text = api.hmm_spec_to_json(spec)
        back = api.hmm_spec_from_json(text)
        assert back == (list(spec[0]), [list(r) for r in spec[1]], [[tuple(c) for c in comps] for comps in spec[2]])
        assert bytes(api.hmm_model(*back)) == bytes(api.polya_model(preset))
        assert api.hmm_spec_to_json(back) == text
        assert back[2][api.POLYA][1][1] is None                                  # a flat component: its mean is null
    awkward = ([0.1 + 0.2, 1.0 / 3.0], [[1e-300, 1.0 - 1e-16], [0.0, 1.0]], [[(2.0 / 3.0, -1e-17, 1e300)], [(1.0, None, 7.0 / 9.0)]])
    assert api.hmm_spec_from_json(api.hmm_spec_to_json(awkward)) == (awkward[0], awkward[1], awkward[2])
    with pytest.raises(ValueError):
        api.hmm_spec_from_json('{"init": [1.0]}')
    with pytest.raises(ValueError):
        api.polya_spec("dna")


def test_pool_equals_its_plain_statement():
    from squigglekit_amd import api
    rng = np.random.default_rng(8)
    for k in range(20):
        m, _ = random_small_case(rng)
        S = m["nstates"]
        reads = [rng.integers(0, 4, n).astype(np.int16) for n in (0, 1, 7, 23, 40, 0, 12)]
        rec, off, seg = hmm_path_ref.segments_reads(m, reads, raw=True)
        got, want = api.hmm_pool(rec, off, seg, S), hmm_path_ref.pool(rec, off, seg, S)
        assert got["sum"].dtype == np.int64 and got["reads"] == 5
        for f in ("n", "sum", "sumsq", "trans", "init"):
            assert got[f].tolist() == want[f], (k, f)
        assert got["n"].sum() == sum(len(r) for r in reads) and got["init"].sum() == 5
        assert got["trans"].sum() == sum(max(len(r) - 1, 0) for r in reads)
        cal = np.stack([rng.integers(-3, 4, len(reads)).astype(np.float64), rng.choice([0.5, 0.25, 2.0], len(reads))], axis=1)
        rec, off, seg = hmm_path_ref.segments_batch(m, *_rows(reads), cal2=cal)
        got, want = api.hmm_pool(rec, off, seg, S, cal2=cal), hmm_path_ref.pool(rec, off, seg, S, cal2=cal)
        assert got["sum"].dtype == np.float64
        for f in ("n", "trans", "init"):
            assert got[f].tolist() == want[f], (k, f)
        for f in ("sum", "sumsq"):                                               # (powers of two and small integers: exact)
            assert got[f].tolist() == want[f], (k, f)
        both = api.hmm_pool_add(got, got)
        assert (both["n"] == 2 * got["n"]).all() and both["reads"] == 2 * got["reads"]


def _rows(reads):
    lens = np.array([len(r) for r in reads], dtype=np.int32)
    buf = np.full((len(reads), max(8, int(lens.max()))), -12345, dtype=np.int16)
    for i, r in enumerate(reads):
        buf[i, :len(r)] = r
    return buf, lens


def test_state_path_and_levels():
    from squigglekit_amd import api
    rng = np.random.default_rng(12)
    m, _ = random_small_case(rng)
    reads = [rng.integers(0, 4, n).astype(np.int16) for n in (30, 40)]
    rec, off, seg = hmm_path_ref.segments_reads(m, reads, raw=True)
    arg, f = hmm_path_ref.back_pointers(m, np.stack([np.pad(r, (0, 40 - len(r))) for r in reads]).astype(np.float64), [30, 40])
    s = hmm_path_ref.state_paths(arg, f, [30, 40])
    for i, r in enumerate(reads):
        g = seg[off[i]:off[i + 1]]
        assert api.hmm_state_path(g, len(r)).tolist() == s[i, :len(r)].tolist()
        with pytest.raises(ValueError):
            api.hmm_state_path(g, len(r) + 1)
        mean, stdv = api.hmm_segment_levels(g)
        cm, cs = api.hmm_segment_levels(g, cal=(3.0, 0.25))
        for k, e in enumerate(g):
            x = r[e["start"]:e["start"] + e["length"]].astype(np.float64)
            assert abs(mean[k] - x.mean()) < 1e-12 and abs(stdv[k] - x.std()) < 1e-9
            assert abs(cm[k] - ((x + 3.0) * 0.25).mean()) < 1e-12 and abs(cs[k] - ((x + 3.0) * 0.25).std()) < 1e-9


def start_spec():
    """the "synth_raw" description with ADAPTER and POLYA moved off the planted levels"""
    from squigglekit_amd import api
    init, trans, em = api.polya_spec("synth_raw")
    em[api.ADAPTER] = [(0.98, 455.0, 40.0), em[api.ADAPTER][1]]
    em[api.POLYA] = [(0.98, 545.0, 16.0), em[api.POLYA][1]]
    return init, trans, em


def ref_decode(batch, model, limit):
    yield hmm_path_ref.segments_reads(model, batch, limit, raw=True, records=False) + (None,)


def test_refit_recovers_the_planted_levels():
    """The 64 planted reads of test_hmm_host, the "synth_raw" description with ADAPTER set to (0.98, 455, 40) and POLYA to
    (0.98, 545, 16); three rounds over states (ADAPTER, POLYA) with update ("mean", "sigma"), decoded by the numpy
    statement.  The fitted POLYA must lie within 0.5 of N(560, 8) and ADAPTER within 0.5 of N(430, 25); the start lies
    outside all four bounds.  0.5 is derived: the sampling error of a mean over more than 10^5 samples is about 0.02, and
    at most about 50 of at least 300 tail samples are misassigned per read.

    Measured (sigma_floor 1, min_count 16): POLYA 560.011 / 8.006 and ADAPTER 430.003 / 25.007 after three rounds; the
    largest polya_end error under the fitted model 49 samples (710 under the start); at most 16 segments per read."""
    from squigglekit_amd import api
    reads = [planted(s) for s in range(64)]
    sigs = [r[0] for r in reads]
    end = np.array([la + lp - 1 for _, la, lp in reads])
    spec0 = start_spec()
    truth = {api.POLYA: (560.0, 8.0), api.ADAPTER: (430.0, 25.0)}
    for k, (mu, sd) in truth.items():
        assert abs(spec0[2][k][0][1] - mu) > 0.5 and abs(spec0[2][k][0][2] - sd) > 0.5        # round 0: outside all four

    def end_error(spec):
        rec = hmm_ref.viterbi_reads(api.hmm_model(*spec), sigs)
        seg = api.polya_segments(rec)
        return int(np.where(seg["found"], np.abs(seg["polya_end"] - end), 10 ** 9).max())
    spec, history = api.hmm_fit(sigs, spec0, (api.ADAPTER, api.POLYA), 3, update=("mean", "sigma"), sigma_floor=1.0,
                                min_count=16, decode=ref_decode)
    assert len(history) == 3 and history[0]["reads"] == 64
    for h in history:
        e = h["spec"][2]
        print("round %d: POLYA %.3f / %.3f, ADAPTER %.3f / %.3f, at most %d segments per read" % (
            h["round"] + 1, e[api.POLYA][0][1], e[api.POLYA][0][2], e[api.ADAPTER][0][1], e[api.ADAPTER][0][2], h["max_segments"]))
    e0, e3 = end_error(spec0), end_error(spec)
    print("largest polya_end error: %d samples under the start, %d under the fitted model" % (e0, e3))
    for k, (mu, sd) in truth.items():
        assert abs(spec[2][k][0][1] - mu) <= 0.5 and abs(spec[2][k][0][2] - sd) <= 0.5, (k, spec[2][k])
    assert e3 <= int(PLANTED_END_MAX * 1.25)
    # only what was named moved
    assert spec[0] == spec0[0] and spec[1] == spec0[1]
    for k in range(6):
        if k not in truth:
            assert spec[2][k] == spec0[2][k]
        else:
            assert spec[2][k][0][0] == 0.98 and spec[2][k][1] == spec0[2][k][1]                # weight and the flat component
    assert api.hmm_refit(spec0, history[0]["pooled"], (), update=("mean", "sigma", "weight", "trans")) == \
        (spec0[0], spec0[1], [list(c) for c in spec0[2]])
    untouched = api.hmm_refit(spec0, history[0]["pooled"], (api.POLYA,), min_count=10 ** 9)
    assert untouched[2][api.POLYA] == list(spec0[2][api.POLYA])
    with pytest.raises(ValueError):
        api.hmm_refit(spec0, history[0]["pooled"], (api.POLYA,), update=("means",))


def test_refit_of_transitions_and_weights():
    """update = ("trans",): forbidden transitions stay -inf, every allowed row sums to 1 within 1e-12 and nothing allowed
    becomes zero; ("weight",): the state's total weight stays, both components stay above zero"""
    from squigglekit_amd import api
    sigs = [planted(s)[0][:4000] for s in range(4)]
    spec0 = api.polya_spec("synth_raw")
    model = api.hmm_model(*spec0)
    pooled = None
    for rec, off, seg, _ in ref_decode(sigs, model, 0):
        pooled = api.hmm_pool_add(pooled, api.hmm_pool(rec, off, seg, 6))
    spec = api.hmm_refit(spec0, pooled, range(6), update=("trans",), min_count=1, pseudo=1.0)
    a0, a1 = model.arrays(), api.hmm_model(*spec).arrays()
    assert (np.isfinite(a0["ltrans"]) == np.isfinite(a1["ltrans"])).all()
    assert (np.array(spec[1])[~np.isfinite(a0["ltrans"])] == 0.0).all()
    for i in range(6):
        assert abs(sum(spec[1][i]) - 1.0) < 1e-12, i
    assert spec[1] != spec0[1] and spec[2] == [list(c) for c in spec0[2]] and spec[0] == spec0[0]
    # CLIFF is never visited in these reads: below min_count its row is left alone
    kept = api.hmm_refit(spec0, pooled, range(6), update=("trans",), min_count=16)
    assert pooled["trans"][api.CLIFF].sum() < 16 and kept[1][api.CLIFF] == spec0[1][api.CLIFF]
    # the row of a visited state follows the counts: ADAPTER was left once per read
    A = pooled["trans"][api.ADAPTER]
    want = (A[api.POLYA] + 1.0 * spec0[1][api.ADAPTER][api.POLYA]) / (A.sum() + 1.0)
    assert abs(spec[1][api.ADAPTER][api.POLYA] - want) < 1e-15
    assert A[api.POLYA] == sum(planted(s)[1] < 4000 for s in range(4)) >= 1       # (the reads whose adapter ends inside the cut)
    w = api.hmm_refit(spec0, pooled, (api.POLYA, api.TRANSCRIPT), update=("weight",))
    for k in (api.POLYA, api.TRANSCRIPT):
        assert abs(w[2][k][0][0] + w[2][k][1][0] - 1.0) < 1e-12 and min(w[2][k][0][0], w[2][k][1][0]) > 0.0
        assert w[2][k] != list(spec0[2][k]) and [c[1:] for c in w[2][k]] == [c[1:] for c in spec0[2][k]]
    assert w[1] == spec0[1]


def test_cli_segments_net_and_refit(tmp_path, monkeypatch, capsys):
    """dRNA_polya.py -s over a raw TSV with the new flags, the GPU calls answered by the numpy statement: the segments
    file, the polya_net column, the read without samples, and --refit / --model_out / --model"""
    from squigglekit_amd import _lib, api, polya_cli
    monkeypatch.setattr(_lib, "warm_start", lambda *a, **k: None)

    def fake_batch(sig, lens, model, cal2=None, limit=0):
        return hmm_path_ref.segments_batch(model, sig, lens, cal2, limit)

    def fake_f64(values, off, model, limit=0):
        return hmm_path_ref.segments_reads(model, [values[off[i]:off[i + 1]] for i in range(len(off) - 1)], limit)
    monkeypatch.setattr(api, "hmm_segments_batch", fake_batch)
    monkeypatch.setattr(api, "hmm_segments_ragged_f64", fake_f64)
    monkeypatch.setattr(api, "hmm_viterbi", lambda *a, **k: pytest.fail("the new flags take the state-path route"))
    def short(seed):
        """a planted read cut down: 300 samples of adapter, 200 of tail, 400 of body"""
        sig, la, lp = planted(seed)
        return np.concatenate([sig[:300], sig[la:la + 200], sig[la + lp:la + lp + 400]])
    a, b = short(3), short(4)
    path = tmp_path / "raw.tsv"
    path.write_text("a.fast5\tid0\tx\ty\t" + "\t".join(str(v) for v in a) + "\n" + "b.fast5\tid1\tx\ty\n"
                    + "c.fast5\tid2\tx\ty\t" + "\t".join(str(v) for v in b) + "\n")
    model = api.polya_model("synth_raw")
    rec, off, seg = hmm_path_ref.segments_reads(model, [a, np.zeros(0, dtype=np.int16), b], raw=True)
    segs = tmp_path / "segs.tsv"
    for batch in ("2", "4096"):
        polya_cli.main(["-s", str(path), "--preset", "synth_raw", "--batch", batch, "--segments", str(segs), "--polya_net"])
        so, se = capsys.readouterr()
        assert se == "dRNA_polya: no samples in read id1 of %s\n" % path
        net = polya_cli.polya_net(rec, off, seg)
        assert so == "".join(polya_cli.polya_lines(["id0", "id1", "id2"], rec, net=net))
        assert so.splitlines()[1] == "id1\t.\t.\t.\t.\t0\t.\t0"
        assert segs.read_text() == "".join(polya_cli.segment_lines(["id0", "id1", "id2"], off, seg, api.POLYA_STATES))
    ps = api.polya_segments(rec)
    assert (net[[0, 2]] <= ps["polya_samples"][[0, 2]]).all() and (net[[0, 2]] > 0).all() and net[1] == 0
    line = segs.read_text().splitlines()[0].split("\t")
    g = seg[0]
    x = a[:g["length"]].astype(np.float64)
    assert line[:6] == ["id0", "0", api.POLYA_STATES[g["state"]], "0", str(g["length"] - 1), str(g["length"])]
    assert abs(float(line[6]) - x.mean()) < 1e-9 and abs(float(line[7]) - x.std()) < 1e-9
    # a cliff inside the tail does not count
    rec1, seg1 = rec[:1].copy(), np.zeros(5, dtype=api.HMM_SEG_DTYPE)
    seg1["state"] = [api.LEADER, api.ADAPTER, api.POLYA, api.CLIFF, api.POLYA]
    seg1["start"] = [0, 10, 100, 150, 153]
    seg1["length"] = [10, 90, 50, 3, 47]
    rec1["enter"][0] = [-1, 0, 10, 100, 150, 200]
    rec1["final_state"] = api.TRANSCRIPT
    assert polya_cli.polya_net(rec1, [0, 5], seg1).tolist() == [97] and api.polya_segments(rec1)["polya_samples"][0] == 100
    # --refit: the model written is hmm_fit's, and the lines that follow are decoded under it
    out_json = tmp_path / "fit.json"
    start = tmp_path / "start.json"
    start.write_text(api.hmm_spec_to_json(start_spec()))
    polya_cli.main(["-s", str(path), "--preset", "synth_raw", "--model", str(start), "--refit", "2", "--states", "2,3",
                    "--model_out", str(out_json), "--polya_net"])
    so, _ = capsys.readouterr()
    want_spec, _h = api.hmm_fit([a, b], start_spec(), (api.ADAPTER, api.POLYA), 2)
    assert api.hmm_spec_from_json(out_json.read_text()) == (want_spec[0], want_spec[1], [list(c) for c in want_spec[2]])
    frec, foff, fseg = hmm_path_ref.segments_reads(api.hmm_model(*want_spec), [a, np.zeros(0, dtype=np.int16), b], raw=True)
    assert so == "".join(polya_cli.polya_lines(["id0", "id1", "id2"], frec, net=polya_cli.polya_net(frec, foff, fseg)))
    polya_cli.main(["-s", str(path), "--preset", "synth_raw", "--refit", "1", "--states", "ADAPTER,polya", "--fit_only",
                    "--model_out", str(out_json)])
    assert capsys.readouterr()[0] == ""
    one, _h = api.hmm_fit([a, b], api.polya_spec("synth_raw"), (api.ADAPTER, api.POLYA), 1)
    assert bytes(api.hmm_model(*api.hmm_spec_from_json(out_json.read_text()))) == bytes(api.hmm_model(*one))
    with pytest.raises(SystemExit):
        polya_cli.main(["-s", str(path), "--refit", "1", "--states", "NOPE"])
    with pytest.raises(SystemExit):
        polya_cli.main(["-s", str(path), "--states", "POLYA"])
