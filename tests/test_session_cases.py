"""CPU: what the scripts of tests/session_cases.py reach, asserted from the statement modules alone (no GPU) -- as
tests/test_random_cases.py does for the committed seeds.  These are conditions, not measurements: if a script misses one,
the script changes and the assertion stays."""
import numpy as np

import evstream_ref as ER
import hmmstream_ref as HR
import live_ref as LR
import mapstream_ref as MR
import randcases as rc
import session_cases as SC


def samples_of(ops):
    return sum(len(c) for op in ops if op[0] == "push" for c in op[2])


def test_event_script_emits_on_both_sides_of_entry_4096():
    sess = SC.event_many()
    pushes = [op for op in sess["ops"] if op[0] == "push"]
    assert [len(op[1]) for op in pushes] == [4095, 1, 4096, 1, 4097, 1, 4097] and sess["nslots"] == SC.MANY_SLOTS
    assert samples_of(sess["ops"]) <= rc.DET_SAMPLES
    want = ER.run_session(sess)
    stage = set()
    for op, (off, rec) in zip(pushes, want):
        m = len(op[1])
        assert np.unique(op[1]).size == m
        stage.add(m)
        if m == 1:
            continue
        lens = np.array([len(c) for c in op[2]])
        assert (lens <= 20).sum() > 3500 and 200 <= ((lens >= 60) & (lens <= 300)).sum() <= 400 and lens.max() == 300
        cnt = np.diff(off)
        assert (cnt[SC.LONG_FROM:min(m, SC.SEAM)] > 0).all()            # every entry 4 030 .. 4 095 emits
        assert (cnt[:SC.LONG_FROM] > 0).sum() > 200 and (cnt == 0).sum() > 200   # empty spans between the others
        if m > SC.SEAM:
            assert (cnt[SC.SEAM:] > 0).all()                            # and the entries of the scan's second block
    last = pushes[-1]
    assert last[3].tolist() == [1, 0] * 2048 + [1]
    assert stage == {1, 4095, 4096, 4097}                               # stage and off shrink and grow


def test_live_script_holds_the_three_outcomes_in_one_push(ora):
    sess = SC.live_many()
    pushes = sess["ops"]
    assert [len(op[1]) for op in pushes] == [4095, 1, 4096, 1, 4097]
    assert samples_of(pushes) <= rc.DET_SAMPLES
    want = LR.run_script(ora, sess["params"], SC.LIVE_CALIB, SC.live_targets(), pushes, sess["nslots"], SC.LIVE_RULE)
    before = {}
    for op, w in zip(pushes[:-1], want[:-1]):
        for s, i in zip(op[1], w["info"]):
            before[int(s)] = (int(i["state"]), int(i["held"]))
    op, w = pushes[-1], want[-1]
    info, out = w["info"], np.diff(w["off"])
    was = np.array([before.get(int(s), (LR.CALIBRATING, 0)) for s in op[1]])
    stays = (info["state"] == LR.CALIBRATING) & (info["held"] > 0) & (out == 0)
    becomes = (was[:, 0] == LR.CALIBRATING) & (was[:, 1] > 0) & (info["state"] == LR.MAPPING) & (info["new_events"] > 0)
    already = (was[:, 0] == LR.MAPPING) & (info["new_events"] > 0)
    assert stays.sum() > 500 and becomes.sum() > 100 and already.sum() > 100
    assert (out[becomes] == was[becomes, 1] + info["new_events"][becomes]).all()       # held levels in front of fresh ones
    assert (out[:SC.SEAM] > 0).sum() > 100 and (out[SC.SEAM:] > 0).all() and len(out) == SC.SEAM + 1
    assert set(w["best"]["decision"].tolist()) == {-1, 0, 1}


def test_hmm_script_names_the_three_entry_counts_in_both_feeds():
    model, sess = SC.hmm_many()
    assert model["nstates"] == 3
    pushes = [op for op in sess["ops"] if op[0] == "push"]
    assert {(len(op[1]), op[3]) for op in pushes} >= {(4095, "i16"), (4096, "f64"), (4097, "i16"), (4097, "f64"), (1, "i16"), (1, "f64")}
    assert all(0 <= len(c) <= 40 for op in pushes for c in op[2])
    assert any(op[0] == "reset" and op[2] is not None for op in sess["ops"])
    last = HR.run_session(model, sess)[-2]
    assert np.isfinite(last["score"]).all() and (last["n_used"] > 40).any()


def test_mapping_script_crosses_the_layout_switch_twice():
    case = SC.map_many()
    T = len(case["targets"])
    assert [len(t) for t in case["targets"]] == [40, 65] and case["nslots"] == 1100
    counts, lanes, across = [], [], None
    rows = np.zeros(case["nslots"], dtype=np.int64)
    cells = 0
    for j, (_, slots, chunks) in enumerate(case["steps"]):
        lens = np.array([len(c) for c in chunks])
        assert (lens == 0).sum() == 2 and (lens == 31).sum() == 3 and (lens == 257).sum() == 3
        count, shapes = SC.map_shapes(case, j)
        counts.append(count)
        lanes.append({shapes[n][0] for n in shapes if 32 <= n <= 64})
        assert shapes[31][0] == 16 and shapes[257][0] == 64 and len(set(shapes.values())) >= 3   # several (L, R) groups per piece index
        mid = {s for s, n in zip(slots, lens) if 32 <= n <= 64}
        across = mid if across is None else across & mid
        for s, n in zip(slots, lens):
            if n:
                rows[s] += n
                cells += int(rows[s]) * sum(len(t) for t in case["targets"])
    assert counts == [1024 * T, 1025 * T, 1024 * T] == [2048, 2050, 2048]
    assert lanes == [{64}, {16}, {64}]
    assert len(across) >= 1000                                          # rows written under one layout and continued under the other
    assert cells <= MR.CELLS


def vec_of(stride, shift):
    """a.vec of k_evs_push for rows at a 16-byte aligned allocation + shift bytes"""
    return shift % 16 == 0 and stride % 8 == 0


def test_layout_script_reaches_every_seam_under_every_feed(ora):
    sess = SC.layout_script()
    assert sess["nslots"] == 70 == 64 + 6 and samples_of(sess["ops"]) <= rc.DET_SAMPLES
    assert [vec_of(*lay) for lay in SC.LAYOUTS] == [True, False, False, False, False]
    assert {lay[0] % 8 for lay in SC.LAYOUTS} == {0, 7, 5} and {lay[1] for lay in SC.LAYOUTS} == {0, 2, 6, 8}
    assert [SC.pad_of(lay) for lay in SC.LAYOUTS].count(32767) == 1 and SC.PAD == -12345
    n = np.zeros(70, dtype=np.int64)
    reached = set()
    for op in sess["ops"]:
        assert max(len(c) for c in op[2]) <= min(lay[0] for lay in SC.LAYOUTS)
        for s, c in zip(op[1], op[2]):
            if n[s] % 2 == 1:
                reached.add(len(c))
            n[s] += len(c)
    assert reached >= set(SC.SEAM_LENS)
    # the script moves all three sessions: events in every push, slots that calibrate and map, a filter that drops samples
    want = ER.run_session(sess)
    assert all(off[-1] > 0 for off, _ in want)
    live = LR.run_script(ora, sess["params"], SC.LIVE_CALIB, SC.live_targets(), sess["ops"], 70, SC.LIVE_RULE)
    states = [set(w["info"]["state"].tolist()) for w in live]
    assert LR.CALIBRATING in states[0] and LR.MAPPING in states[1] and (live[-1]["info"]["ended"] == 1).all()
    x = np.concatenate([c for op in sess["ops"] for c in op[2]])
    kept = ((x > 0) & (x < 1200)).mean()
    assert 0.5 < kept < 0.999


def test_contract_script_holds_every_clamp_skip_and_ended_slot():
    S, st = SC.CONTRACT_SLOTS, SC.CONTRACT_STRIDE
    pushes = SC.contract_script()
    seen = set()
    ended = set()
    for j, p in enumerate(pushes):
        if j == SC.CONTRACT_RESET_BEFORE:
            assert 5 in ended
            ended.discard(5)
            seen.add("reset")
        assert p["rows"].shape == (len(p["slots"]), st)
        for s, n, e, c in zip(p["slots"], p["len"], p["end"], p["chunks"]):
            if s in (-1, S):
                assert c is None
                seen.add("slot %d" % s)
                continue
            assert 0 <= s < S
            if s in ended and n > 0:
                assert len(c) == 0
                seen.add("ended")
            elif n < 0:
                assert len(c) == 0
                seen.add("negative")
            elif n > st:
                assert len(c) == st
                seen.add("above")
            else:
                assert len(c) == n
                if j >= SC.CONTRACT_RESET_BEFORE and s == 5 and n > 0:
                    seen.add("works again")
            if e:
                ended.add(s)
    assert seen == {"reset", "slot -1", "slot %d" % S, "ended", "negative", "above", "works again"}
    assert ended == set(range(S))
    # without END (HMM, MotifSeq) the samples behind slot 5's flag count
    assert len(SC.contract_script(False)[2]["chunks"][0]) == st and len(pushes[2]["chunks"][0]) == 0
    ops, keep = SC.contract_ops(True)
    assert [len(k) for k in keep] == [6, 4, 3, 2, 6] and [op[0] for op in ops].count("reset") == 1
    assert any(off[-1] > 0 for off, _ in ER.run_session({"params": SC.DNA, "nslots": S, "ops": ops}))


def test_hmm_device_test_runs_every_layout():
    """the draw of test_gpu_hmmstream.test_device_forms_give_the_bytes_of_the_host_forms has an int16 push per layout"""
    import test_gpu_hmmstream as T
    sess = HR.draw_session(np.random.default_rng(10), nslots=70, budget=100000, maxlen=300, draw_chunk=T.levels)
    assert sum(op[0] == "push" and op[3] == "i16" for op in sess["ops"]) >= len(T.LAYOUTS)
    assert set(T.LAYOUTS) >= set(SC.LAYOUTS)


def test_interleaved_walk_puts_pushes_on_both_sides_of_the_large_calls():
    seq = SC.interleave_sequence()
    scripts = SC.interleave_scripts()
    assert 40 <= len(seq) <= 55
    shots = [s for s in seq if s[0] != "session"]
    assert shots == SC.ONESHOT
    assert {f for f, _ in shots} == {"pairs", "pairpaths", "hits", "detect", "hmm", "panel", "drna", "band", "pairhits", "maphits"}
    assert shots.count(("pairhits", 0)) == 2 and shots.count(("band", 0)) == 2
    big = [k for k, s in enumerate(seq) if s in (("pairs", 9), ("pairpaths", 145), ("hits", 1), ("detect", 27), ("hmm", 35),
                                                 ("panel", 4), ("drna", 14), ("pairhits", 1))]
    between = 0
    for name in SC.SESSIONS:
        at = [k for k, s in enumerate(seq) if s == ("session", name)]
        ops = SC.session_ops(scripts, name)
        assert len(at) == len(ops)
        pushes = [k for k, op in zip(at, ops) if op[0] == "push"]
        assert pushes[0] < big[0] and pushes[-1] > big[-1], name
        between += any(big[0] < k < big[-1] for k in at)
    assert between >= 3                                                # and some sessions are pushed between the large calls
    k = seq.index(("pairhits", 1))
    assert seq[k - 1] == seq[k + 1] == ("maphits", 0)
    # the larger list has more rows than the session's hit list names: c->rowhit grows between the two reads
    a = scripts["mapA"]
    assert len(SC.pairhits_case(1)["pairs"]) > len(a["targets"]) * a["nslots"] > len(SC.pairhits_case(0)["pairs"])
    assert any(len(c) for st in a["steps"][:1] for c in st[2])
