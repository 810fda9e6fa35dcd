"""GPU: six sessions open at once -- an EventStream, an HmmStream, two MapStreams on different targets, a MotifStream and
a LiveMap -- walked one op at a time (tests/session_steps.py) between one-shot calls whose sizes go up and then down
(tests/session_cases.py, part D).  Sessions own most of their buffers, but sk_map_hits selects through c->rowhit, a
mapping push runs k_sdtw and shares the retry and profile state a pair call resets, the guard counters of the event and
HMM sessions live on the context, and the last_* getters are context state.  Every session op against its statement,
every one-shot call against its reference, a call that occurs twice the same bytes both times."""
import numpy as np
import pytest

import band_ref
import evstream_ref as ER
import hmmstream_ref as HR
import live_ref as LR
import pair_hits_ref as PH
import randcases as rc
import session_cases as SC
import session_steps as SS

pytestmark = pytest.mark.gpu


def one_shot(monkeypatch, ora, fam, seed):
    """one call against its reference; returns its result for the comparison with the same call elsewhere"""
    from squigglekit_amd import api
    from test_gpu_random import run_case
    if fam == "band":
        for key in rc.SWITCHES:
            monkeypatch.delenv(key, raising=False)
        case = SC.band_case()
        w_rec, w_off, w_spans, lost = band_ref.records(case["seqs"], case["pairs"], case["band"], case["end"])
        rec, off, spans = api.dtw_band(case["seqs"], case["pairs"], case["band"], case["end"])
        assert PH.same(rec, w_rec) is None, PH.same(rec, w_rec)
        assert np.array_equal(off, w_off) and spans.tobytes() == w_spans.tobytes()
        assert api.last_path_mismatches() == lost
        return rec, off, spans
    if fam == "pairhits":
        for key in rc.SWITCHES:
            monkeypatch.delenv(key, raising=False)
        case = SC.pairhits_case(seed)
        w_hits, w_count, _ = PH.pair_hits(ora, case["seqs"], case["pairs"], case["K"])
        hits, count = api.dtw_pairs_hits(case["seqs"], case["pairs"], case["K"])
        assert PH.same(hits, w_hits) is None, PH.same(hits, w_hits)
        assert np.array_equal(count, w_count)
        return hits, count
    got, _ = run_case(monkeypatch, ora, rc.interleave_case(fam, seed))
    return got


def test_sessions_between_one_shot_calls(gpu, ora, monkeypatch):
    from squigglekit_amd import _lib, api
    sc = SC.interleave_scripts()
    model = api.polya_model(sc["hmm"][0])
    mp = SC.MOTIF_PARAMS
    live_want = LR.run_script(ora, sc["live"]["params"], SC.LIVE_CALIB, SC.live_targets(), sc["live"]["ops"], sc["live"]["nslots"],
                              SC.LIVE_RULE)
    with api.EventStream(_lib.DetParams(*sc["event"]["params"]), sc["event"]["nslots"]) as es, \
            api.HmmStream(model, sc["hmm"][1]["nslots"]) as hs, \
            api.MapStream(sc["mapA"]["targets"], sc["mapA"]["nslots"]) as ma, \
            api.MapStream(sc["mapB"]["targets"], sc["mapB"]["nslots"]) as mb, \
            api.MotifStream(sc["motif"]["motifs"], sc["motif"]["nslots"], mp["mode"], mp["lo"], mp["hi"], calib=mp["W"]) as mo, \
            api.LiveMap(_lib.DetParams(*sc["live"]["params"]), SC.LIVE_CALIB, SC.live_targets(), sc["live"]["nslots"]) as lm:
        walk = {"event": SS.EventSteps(es, sc["event"], ER.run_session(sc["event"])),
                "hmm": SS.HmmSteps(hs, sc["hmm"][1], HR.run_session(model, sc["hmm"][1])),
                "mapA": SS.MapSteps(ma, sc["mapA"], SS.map_expectations(ora, sc["mapA"]), "mapA"),
                "mapB": SS.MapSteps(mb, sc["mapB"], SS.map_expectations(ora, sc["mapB"]), "mapB"),
                "motif": SS.MotifSteps(mo, sc["motif"], SS.motif_expectations(sc["motif"], mp["W"], mp["mode"], mp["lo"], mp["hi"])),
                "live": SS.LiveSteps(lm, sc["live"], live_want, SC.LIVE_RULE)}
        seen, map_hits = {}, []
        for step, (fam, seed) in enumerate(SC.interleave_sequence()):
            try:
                if fam == "session":
                    walk[seed].step()
                    continue
                if fam == "maphits":
                    map_hits.append(walk["mapA"].hits(3, "at step %d" % step))
                    continue
                got = one_shot(monkeypatch, ora, fam, seed)
            except AssertionError as e:
                raise AssertionError("step %d (%s %s) of the walk: %s" % (step, fam, seed, e))
            b = rc.result_bytes(got)
            if (fam, seed) in seen:
                assert b == seen[fam, seed][1], "step %d: %s %s differs from the same call at step %d" % (step, fam, seed, seen[fam, seed][0])
            else:
                seen[fam, seed] = (step, b)
            if fam in ("pairs", "pairpaths", "pairhits"):             # a pair call: the screening counters read zeros
                assert not any(api.last_dtw_guard().values()), (step, fam, seed, api.last_dtw_guard())
        assert all(w.left == 0 for w in walk.values()), {k: w.left for k, w in walk.items()}
        # the hit lists of mapA on both sides of the larger dtw_pairs_hits call: nothing of the session moved in between
        assert len(map_hits) == 2 and rc.result_bytes(map_hits[0]) == rc.result_bytes(map_hits[1])
        assert walk["event"].finish(api) > 0
        assert api.last_event_plan()["guard_hits"] == 0
        assert api.last_hmm_stream_plan()["guard_hits"] == 0
    assert len(seen) < sum(f not in ("session", "maphits") for f, _ in SC.interleave_sequence())
