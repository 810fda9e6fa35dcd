"""Host: the HMM sessions' definition with carried state (tests/hmmstream_ref.py) against the one-shot definition
(tests/hmm_ref.py) on every prefix, and api.polya_decide on hand-made records.  No GPU."""
import numpy as np

import hmm_ref
import hmmstream_ref as HR

NINF = -np.inf


def test_carried_state_equals_the_one_shot_definition_on_every_prefix():
    """200 tie-heavy integer cases (S = 1 .. 6, -inf transitions, dead states, both emission components): the read goes
    into slot 1 of 3 in random cuts (empty chunks among them) through either feed, and after every push the first 40
    bytes of the record are hmm_ref.viterbi's of the prefix, v the scores behind them"""
    rng = np.random.default_rng(20261020)
    sizes, dead, cuts_seen = set(), 0, 0
    for k in range(200):
        m = HR.tie_model(rng)
        S = m["nstates"]
        n = int(rng.integers(0, 41))
        x = rng.integers(0, 4, n).astype(np.int16)
        ses = HR.Session(m, 3)
        at, pushes = 0, 0
        while True:
            step = int(rng.integers(0, 9)) if at < n else 0
            chunk = x[at:at + step]
            feed = "i16" if rng.random() < 0.5 else "f64"
            rec = ses.push([1], [chunk if feed == "i16" else chunk.astype(np.float64)], feed)[0]
            at += len(chunk)
            pushes += len(chunk) > 0
            want = hmm_ref.viterbi(m, x[:at].astype(np.float64))
            for name in hmm_ref.DTYPE.names:
                assert rec[name].tobytes() == want[name].tobytes(), (k, at, name, rec, want)
            assert rec["pushes"] == pushes and rec["flags"] == 0, (k, rec)
            assert (rec["v"][S:] == NINF).all(), (k, rec)
            if at == 0:
                assert (rec["v"] == NINF).all() and rec.tobytes() == HR.empty_records(1)[0].tobytes()
            else:
                f = int(rec["final_state"])
                assert rec["v"][f].tobytes() == rec["score"].tobytes() and not (rec["v"][:f] >= rec["v"][f]).any() \
                    and not (rec["v"] > rec["v"][f]).any(), (k, rec)
            cuts_seen += 1
            if at >= n and step == 0:
                break
        sizes.add(S)
        dead += bool(n > 0 and rec["score"] == NINF)
        # the neighbours were never touched
        assert ses.records([0, 2]).tobytes() == HR.empty_records(2).tobytes()
    assert sizes == {1, 2, 3, 4, 5, 6} and dead > 5 and cuts_seen > 1000


def test_calibration_pairs_and_reset():
    rng = np.random.default_rng(7)
    m = HR.tie_model(rng, 4)
    x = rng.integers(0, 4, 30).astype(np.int16)
    ses = HR.Session(m, 2)
    ses.reset([1, 0], [[2.0, 0.5], [0.0, 1.0]])
    a = ses.push([0, 1], [x[:11], x[:7]], "i16")
    b = ses.push([1, 0], [x[7:], x[11:]], "i16")
    want_cal = hmm_ref.viterbi(m, (x.astype(np.float64) + 2.0) * 0.5)
    want_raw = hmm_ref.viterbi(m, x.astype(np.float64))
    for name in hmm_ref.DTYPE.names:
        assert b[0][name].tobytes() == want_cal[name].tobytes() and b[1][name].tobytes() == want_raw[name].tobytes()
    assert a["n_used"].tolist() == [11, 7] and b["pushes"].tolist() == [2, 2]
    ses.reset([1])                                                       # a reset without pairs: no calibration from then on
    c = ses.push([1], [x], "i16")[0]
    assert c["score"].tobytes() == want_raw["score"].tobytes() and c["pushes"] == 1 and c["n_used"] == 30


def record(final_state, n_used, enter_t, v):
    from squigglekit_amd import api
    r = api.no_hmm_stream_records(1)
    r["final_state"], r["n_used"] = final_state, n_used
    r["enter"][0, api.TRANSCRIPT] = enter_t
    r["v"][0] = v
    r["score"] = max(v)
    return r


def test_polya_decide_on_hand_made_records():
    from squigglekit_amd import api
    T, P = api.TRANSCRIPT, api.POLYA
    lead = [NINF, NINF, -900.0, -520.0, -700.0, -500.0]                 # TRANSCRIPT leads POLYA by 20
    assert api.HMMS_DTYPE == HR.DTYPE and api.HMMS_DTYPE.itemsize == 96
    ok = record(T, 5000, 3000, lead)
    kw = dict(min_body=2000, min_margin=20.0, give_up=0)
    assert api.polya_decide(ok, **kw).tolist() == [1] and api.polya_decide(ok, **kw).dtype == np.int8
    # each of the three conditions alone failing
    assert api.polya_decide(record(P, 5000, 3000, lead), **kw).tolist() == [0]                # the path ends elsewhere
    assert api.polya_decide(record(T, 4999, 3000, lead), **kw).tolist() == [0]                # body one sample short
    assert api.polya_decide(ok, min_body=2000, min_margin=20.5, give_up=0).tolist() == [0]    # margin too small
    tied = record(T, 5000, 3000, [NINF, NINF, -900.0, -500.0, -700.0, -500.0])
    assert api.polya_decide(tied, min_body=1, min_margin=0.5, give_up=0).tolist() == [0]
    assert api.polya_decide(tied, min_body=1, min_margin=0.0, give_up=0).tolist() == [1]
    # give_up: only when not accepted, from n_used == give_up on; 0 disables it
    wait = record(P, 5000, -1, [NINF, NINF, -900.0, -400.0, -700.0, NINF])
    assert api.polya_decide(wait, 2000, 20.0, 5001).tolist() == [0]
    assert api.polya_decide(wait, 2000, 20.0, 5000).tolist() == [-1]
    assert api.polya_decide(wait, 2000, 20.0, 0).tolist() == [0]
    assert api.polya_decide(ok, 2000, 20.0, 10).tolist() == [1]
    # the empty record waits, whatever the thresholds: no final state, no margin (-inf - -inf), and n_used is 0
    empty = api.no_hmm_stream_records(2)
    assert empty.tobytes() == HR.empty_records(2).tobytes()
    assert api.polya_decide(empty, 0, 0.0, 1).tolist() == [0, 0]
    assert api.polya_decide(empty, 0, -np.inf, 0).tolist() == [0, 0]
    # several at once, any shape; polya_segments reads the same records
    both = np.concatenate([ok, wait, tied, empty])
    assert api.polya_decide(both, 2000, 20.0, 5000).tolist() == [1, -1, -1, 0, 0]     # (tied: no margin, and 5000 samples)
    assert api.polya_decide(both, 2000, 20.0, 5001).tolist() == [1, 0, 0, 0, 0]
    assert api.polya_decide(both.reshape(5, 1), 2000, 20.0, 5000).shape == (5, 1)
    ok["enter"][0, P] = 2500
    seg = api.polya_segments(both[:1].copy())
    assert seg["found"].tolist() == [False]                             # (never went through POLYA: enter[POLYA] is -1)
    seg = api.polya_segments(ok)
    assert seg["found"].tolist() == [True] and seg["polya_start"][0] == 2500 and seg["polya_end"][0] == 2999
