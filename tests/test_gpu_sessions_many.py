"""GPU: session pushes of thousands of entries (tests/session_cases.py, part A) against the statement modules.  Every
comparison is == on bytes.  The pushes name 4 095, 4 096 and 4 097 slots: k_evs_push runs 65 workgroups, k_live_count and
k_live_fill place their output through a scan whose second block starts at entry 4 096, and a mapping push of 1 024 or
1 025 live slots sits on either side of the lane-layout switch of sk_exact_shape."""
import numpy as np
import pytest

import evstream_ref as ER
import hmmstream_ref as HR
import live_ref as LR
import mapstream_ref as MR
import pair_hits_ref as PH
import session_cases as SC

pytestmark = pytest.mark.gpu


def test_event_session_pushes_around_4096_entries(gpu):
    from squigglekit_amd import api
    sess = SC.event_many()
    assert ER.play_session(api, sess, "event many") == 2049              # the reads the last push ended, against the one-shot call
    plan = api.last_event_plan()
    assert plan["guard_hits"] == 0 and plan["state_bytes"] == SC.MANY_SLOTS * 416


def test_live_session_pushes_around_4096_entries(gpu, ora):
    from squigglekit_amd import api
    sess = SC.live_many()
    got, want = LR.play(api, ora, sess["params"], SC.LIVE_CALIB, SC.live_targets(), sess["ops"], sess["nslots"],
                        rule=SC.LIVE_RULE, label="live many")
    rec, info, best = got[-1]
    assert best.shape == (4097,) and set(best["decision"].tolist()) == {-1, 0, 1}
    assert {LR.CALIBRATING, LR.MAPPING} <= set(info["state"].tolist())
    assert api.last_event_plan()["guard_hits"] == 0
    assert api.last_live_plan()["bridged_levels"] == want[-1]["off"][-1] > 4097


def test_hmm_session_pushes_around_4096_entries(gpu):
    from squigglekit_amd import api
    model, sess = SC.hmm_many()
    assert HR.play_session(api, model, sess, "hmm many") == 8
    assert api.last_hmm_stream_plan() == {"state_bytes": SC.MANY_SLOTS * 224, "guard_hits": 0}


def test_mapping_session_rows_continue_across_the_layout_switch(gpu, ora):
    """pushes of 1 024, 1 025 and 1 024 live slots on two targets: slots 0 .. 1 023 store their rows under 64 lanes,
    continue them under 16 and then under 64 again; the hit lists are read from rows written under both"""
    from squigglekit_amd import api
    case = SC.map_many()
    sh = MR.Shadow(ora, case["targets"], case["nslots"])
    plans = []
    with api.MapStream(case["targets"], case["nslots"]) as ms:
        for j, (_, slots, chunks) in enumerate(case["steps"]):
            diff = MR.first_difference(ms.push(slots, chunks), sh.push(slots, chunks))
            assert diff is None, "push %d: %s" % (j, diff)
            count, shapes = SC.map_shapes(case, j)
            plan = api.last_map_plan()
            assert plan["entries"] == count and plan["launches"] == len(set(shapes.values())), (j, plan, shapes)
            plans.append((plan["launches"], shapes))
            if j == 1:
                named = [s for s in slots if sh.pts[s].size]
                chunks_of = [[st[2][st[1].index(s)] for st in case["steps"][:2] if s in st[1]] for s in named]
                w_hits, w_count = PH.session_hits(chunks_of, case["targets"], 3)
                hits, cnt = ms.hits(named, 3)
                assert np.array_equal(cnt, w_count)
                diff = PH.same(hits, w_hits)
                assert diff is None, "hits: %s" % diff
        every = list(range(case["nslots"]))
        diff = MR.first_difference(ms.peek(every), sh.push(every, [np.zeros(0)] * len(every)))
        assert diff is None, "closing peek: %s" % diff
    # the second push took another plan than the first and the third
    assert [p[0] for p in plans] == [3, 4, 3] and plans[2][1] == plans[0][1]
    lanes = [{shapes[n][0] for n in shapes if 32 <= n <= 64} for _, shapes in plans]
    assert lanes == [{64}, {16}, {64}]
