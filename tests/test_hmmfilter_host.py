"""Host: the filtered HMM sessions' definition with carried alpha (tests/hmmfilter_ref.py) against the one-shot statement
of the posteriors (tests/hmm_post_ref.py) on every prefix, api.polya_decide_post on hand-made records, and the new
columns of dRNA_polya_stream.py with the statement in the GPU's place.  No GPU."""
import numpy as np
import pytest

import hmm_post_ref as PR
import hmmfilter_ref as FR
import hmmstream_ref as HR

NINF = -np.inf


def prefix_table(model, x):
    """the one-shot statement's (loglik, final_post, flags) of every prefix x[:1] .. x[:n], as rows of one batch"""
    n = len(x)
    post = PR.posterior_rows(model, np.tile(np.asarray(x, dtype=np.float64), (n, 1)), np.arange(1, n + 1), False, False)[0]
    return post


def cases():
    """(label, model, samples int16 or float64, cal2 or None): about 40 reads of at most 60 samples"""
    from squigglekit_amd import api
    rng = np.random.default_rng(20261021)
    out = []
    for k in range(28):                                                  # tie-heavy integer models, S = 1 .. 6
        m = HR.tie_model(rng, S=1 + k % 6)
        out.append(("tie %d" % k, m, rng.integers(0, 4, int(rng.integers(1, 41))).astype(np.int16), None))
    for k in range(5):
        out.append(("synth_raw %d" % k, api.polya_model("synth_raw"), HR.small_drna_read(rng, 60)[:int(rng.integers(30, 61))], None))
    for k in range(5):                                                   # raw counts that the pair turns into pA
        raw = np.rint(HR.small_drna_read(rng, 60).astype(np.float64) / 5.5 / 0.1825 - 3.0).astype(np.int16)
        out.append(("rna_pa %d" % k, api.polya_model("rna_pa"), raw, (3.0, 0.1825)))
    for k in range(3):                                                   # possible for three samples at the most
        out.append(("dead end %d" % k, FR.dead_end_model(), rng.integers(0, 4, 4 + 3 * k).astype(np.int16), None))
    out.append(("loop", FR.loop_model(), rng.integers(0, 4, 60).astype(np.int16), None))
    return out


def test_carried_alpha_equals_the_one_shot_statement_on_every_prefix():
    """slot 0 takes the read one sample per push (every prefix), slot 2 in random cuts with peeks through either feed;
    after every push loglik, flags and post are posterior_rows' loglik, flags and final_post of the prefix by their bits,
    post sums to 1 within 1e-9 where the prefix is possible, and slot 1 was never touched"""
    dead, sizes, checked = 0, set(), 0
    rng = np.random.default_rng(5)
    for label, model, x, cal in cases():
        xs = x.astype(np.float64) if cal is None else (x.astype(np.float64) + cal[0]) * cal[1]
        table = prefix_table(model, xs)
        ses = FR.Session(model, 3)
        if cal is not None:
            ses.reset([0, 2], [cal, cal])
        n = len(x)

        def check(slot, at):
            f = ses.filter([slot])[0]
            if at == 0:
                assert f.tobytes() == FR.empty_filters(1)[0].tobytes(), label
                return
            w = table[at - 1]
            assert f["n_used"] == at == w["n_used"] and f["flags"] == w["flags"], (label, at, f, w)
            assert f["loglik"].tobytes() == w["loglik"].tobytes(), (label, at, f, w)
            assert f["post"].tobytes() == w["final_post"].tobytes(), (label, at, f, w)
            assert not np.isnan(f["post"]).any() and not np.isnan(f["loglik"])
            if f["flags"] == 0:
                assert abs(f["post"].sum() - 1.0) < 1e-9, (label, at, f)
            else:
                assert f["loglik"] == NINF and (f["post"] == 0.0).all(), (label, at, f)

        for t in range(n):
            rec = ses.push([0], [x[t:t + 1]], "i16")
            check(0, t + 1)
            checked += 1
        at = 0
        while at < n:
            step = int(rng.integers(0, 9))
            chunk = x[at:at + step]
            if cal is None and rng.random() < 0.5:
                ses.push([2], [chunk.astype(np.float64)], "f64")
            else:
                ses.push([2], [chunk], "i16")
            at += len(chunk)
            check(2, at)
        assert ses.filter([0, 2])[0].tobytes() == ses.filter([0, 2])[1].tobytes(), label
        assert ses.filter([1]).tobytes() == FR.empty_filters(1).tobytes()
        plain = HR_records(model, x, cal)                                # the Viterbi side is hmmstream_ref's, untouched
        for name in ("score", "final_state", "n_used", "enter", "v"):
            assert rec[name].tobytes() == ses.records([2])[name].tobytes() == plain[name].tobytes(), (label, name)
        sizes.add(int(ses.S))
        dead += int(table["flags"][-1] != 0)
    assert sizes == {1, 2, 3, 4, 5, 6} and dead >= 3 and checked > 1000


def HR_records(model, x, cal):
    """a plain session's record of the whole read in one push"""
    ses = HR.Session(model, 1)
    if cal is not None:
        ses.reset([0], [cal])
    return ses.push([0], [x], "i16")


def test_reset_clears_alpha_and_neighbours_are_independent():
    rng = np.random.default_rng(9)
    m = FR.loop_model()
    x = rng.integers(0, 4, 30).astype(np.int16)
    ses = FR.Session(m, 3)
    ses.push([0, 1, 2], [x[:10], x[:20], x[:0]], "i16")
    ses.reset([1])
    assert ses.filter([1]).tobytes() == FR.empty_filters(1).tobytes() and (ses.alpha[1] == NINF).all()
    ses.push([2, 1], [x[:10], x[:10]], "i16")
    f = ses.filter([0, 1, 2])
    assert f[0].tobytes() == f[1].tobytes() == f[2].tobytes() and f["n_used"].tolist() == [10, 10, 10]


def records(final_state, n_used, enter_t, post_t, loglik, flags=0):
    from squigglekit_amd import api
    r = api.no_hmm_stream_records(1)
    r["final_state"], r["n_used"] = final_state, n_used
    r["enter"][0, api.TRANSCRIPT] = enter_t
    f = np.zeros(1, dtype=api.HMMS_FILT_DTYPE)
    f["n_used"], f["loglik"], f["flags"] = n_used, loglik, flags
    f["post"][0, api.TRANSCRIPT] = post_t
    f["post"][0, api.POLYA] = 1.0 - post_t if flags == 0 else 0.0
    return r, f


def test_polya_decide_post_on_hand_made_records():
    from squigglekit_amd import api
    T, P = api.TRANSCRIPT, api.POLYA
    assert api.HMMS_FILT_DTYPE == FR.FILT_DTYPE and api.HMMS_FILT_DTYPE.itemsize == 64
    kw = dict(min_body=2000, min_post=0.99, give_up=0)
    ok = records(T, 5000, 3000, 0.995, -15000.0)
    assert api.polya_decide_post(*ok, **kw).tolist() == [1] and api.polya_decide_post(*ok, **kw).dtype == np.int8
    # each of the three conditions alone failing: wait
    assert api.polya_decide_post(*records(P, 5000, 3000, 0.995, -15000.0), **kw).tolist() == [0]
    assert api.polya_decide_post(*records(T, 4999, 3000, 0.995, -15000.0), **kw).tolist() == [0]
    assert api.polya_decide_post(*records(T, 5000, 3000, 0.98, -15000.0), **kw).tolist() == [0]
    assert api.polya_decide_post(*records(T, 5000, 3000, 0.99, -15000.0), **kw).tolist() == [1]      # >=, not >
    # the three ways to -1, each alone, and never when accepted
    wait = records(P, 5000, -1, 0.2, -15000.0)
    assert api.polya_decide_post(*wait, 2000, 0.99, 5001).tolist() == [0]
    assert api.polya_decide_post(*wait, 2000, 0.99, 5000).tolist() == [-1]
    assert api.polya_decide_post(*ok, 2000, 0.99, 10).tolist() == [1]
    dead = records(0, 5000, -1, 0.0, NINF, flags=PR.IMPOSSIBLE)
    assert api.polya_decide_post(*dead, **kw).tolist() == [-1]
    assert api.polya_decide_post(*wait, **kw, min_rate=-3.0).tolist() == [0]                          # -3.0 per sample: not below
    assert api.polya_decide_post(*wait, **kw, min_rate=-2.9).tolist() == [-1]
    assert api.polya_decide_post(*wait, 5001, 0.99, 0, min_rate=-2.9).tolist() == [0]                 # fewer than min_body samples
    assert api.polya_decide_post(*ok, **kw, min_rate=-2.9).tolist() == [1]
    assert api.polya_decide_post(*wait, **kw, min_rate=None).tolist() == [0]
    # the empty record waits whatever the thresholds (0 / 0 is no rate)
    empty = api.no_hmm_stream_records(2), np.zeros(2, dtype=api.HMMS_FILT_DTYPE)
    assert api.polya_decide_post(*empty, 0, 0.0, 1, min_rate=100.0).tolist() == [0, 0]
    # several at once, any shape; a filter per record
    rec = np.concatenate([ok[0], wait[0], dead[0], empty[0]])
    filt = np.concatenate([ok[1], wait[1], dead[1], empty[1]])
    assert api.polya_decide_post(rec, filt, 2000, 0.99, 5000).tolist() == [1, -1, -1, 0, 0]
    assert api.polya_decide_post(rec, filt, 2000, 0.99, 0).tolist() == [1, 0, -1, 0, 0]
    assert api.polya_decide_post(rec.reshape(5, 1), filt.reshape(5, 1), 2000, 0.99, 0).shape == (5, 1)
    with pytest.raises(ValueError):
        api.polya_decide_post(rec, filt[:4], 2000, 0.99, 0)


class FakeStream:
    """api.HmmStream's calls on top of the numpy statement"""
    opened = []

    def __init__(self, model, nslots=1, filter=False):                   # noqa: A002
        self.ref = FR.Session(model, nslots)
        self.filtered = filter
        FakeStream.opened.append(filter)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def reset(self, slots, cal2=None):
        self.ref.reset(slots, cal2)

    def push(self, slots, chunks):
        return self.ref.push(slots, [np.asarray(c) for c in chunks], "i16")

    def push_values(self, slots, chunks):
        return self.ref.push(slots, [np.asarray(c, dtype=np.float64) for c in chunks], "f64")

    def filter(self, slots):
        assert self.filtered
        return self.ref.filter(slots)


def run(main, argv):
    import contextlib
    import io
    out, err = io.StringIO(), io.StringIO()
    code = 0
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            main(argv)
        except SystemExit as e:
            code = e.code if isinstance(e.code, int) else 1
    return out.getvalue(), err.getvalue(), code


def test_cli_columns_with_the_statement_in_the_gpus_place(tmp_path, monkeypatch):
    """reads that run to their end: the two new columns are the one-shot statement's loglik / n and final_post[TRANSCRIPT]
    in dRNA_polya.py --posterior's format; without the new flags the session is plain and the lines have ten columns"""
    from squigglekit_amd import api, polya_stream_cli
    from squigglekit_amd.polya_cli import posterior_columns
    rng = np.random.default_rng(20261021)
    reads = np.stack([HR.small_drna_read(rng, 240) for _ in range(5)])
    path = str(tmp_path / "reads.npy")
    np.save(path, reads)
    monkeypatch.setattr(api, "HmmStream", FakeStream)
    FakeStream.opened.clear()
    base = ["--i16", path, "--preset", "synth_raw", "--sample_chunk", "77", "--channels", "3", "--min_body", "1000000000"]
    plain, err, code = run(polya_stream_cli.main, base)
    assert code == 0, err[-300:]
    got, err, code = run(polya_stream_cli.main, base + ["--min_post", "0.99", "--min_margin", "1e9"])
    assert code == 0, err[-300:]
    assert FakeStream.opened == [False, True]
    post = PR.posterior_batch(api.polya_model("synth_raw"), reads, np.full(5, 240), counts=False, dense=False)[0]
    want = posterior_columns(post, None, True, None)
    rows, prow = [ln.split("\t") for ln in got.splitlines()], [ln.split("\t") for ln in plain.splitlines()]
    assert len(rows) == 5 and sorted(r[0] for r in rows) == [str(i) for i in range(5)]
    for r in rows:
        i = int(r[0])
        assert len(r) == 12 and r[7] == "end" and r[10:] == [want[i][0], want[i][2]], (r, want[i])
        assert float(r[11]) > 0.5                                        # the synthetic reads end in their body
    assert sorted(r[:10] for r in rows) == sorted(prow) and all(len(r) == 10 for r in prow)
    # an accepting run: the decision is polya_decide_post's, and the line is written at that moment
    got, err, code = run(polya_stream_cli.main, base[:-2] + ["--min_body", "40", "--min_post", "0.9", "--min_margin", "1e9"])     # (the margin is ignored)
    assert code == 0, err[-300:]
    rows = [ln.split("\t") for ln in got.splitlines()]
    assert len(rows) == 5 and all(r[7] == "accept" and float(r[11]) >= 0.9 and int(r[9]) < 240 for r in rows), rows
    # a rate no read reaches rejects every read once it has --min_body samples; --min_rate alone turns the columns on
    got, err, code = run(polya_stream_cli.main, base[:-2] + ["--min_body", "100", "--min_rate", "0.0"])
    assert code == 0, err[-300:]
    rows = [ln.split("\t") for ln in got.splitlines()]
    assert len(rows) == 5 and all(len(r) == 12 and r[7] in ("reject", "accept") for r in rows) and any(r[7] == "reject" for r in rows)
    out, err, code = run(polya_stream_cli.main, base + ["--min_post", "1.5"])
    assert code == 2 and "--min_post must be in [0, 1]" in err
