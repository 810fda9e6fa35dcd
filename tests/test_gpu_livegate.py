"""GPU: gated live mapping sessions (sk_live_open_gated, api.LiveMap(gate=...)) against tests/livegate_ref.py --
hmmstream_ref for the HMM record a slot's decision is taken on, evstream_ref for the events a push emits, the gate and its
ring in plain Python, live_ref.Slot and the oracle's dtw_subsequence behind it.  Every comparison is == on bytes, after
every push: records, info, fetch, best, the gate record and the HMM record.  guard_hits is 0 after every test."""
import ctypes as C

import numpy as np
import pytest

import detect_ref
import hmmstream_ref as HR
import live_ref as LR
import livegate_ref as GR

pytestmark = pytest.mark.gpu

DNA, RNA = detect_ref.PRESETS["dna"], detect_ref.PRESETS["rna"]
_rng = np.random.default_rng(2025)
TARGETS = [_rng.normal(size=n) for n in (300, 600)]
LIVE_RULE = (40, 1.5, 0.01, 120)
EMPTY = np.zeros(0, dtype=np.int16)
_cache = {}


@pytest.fixture(autouse=True)
def no_guard_hit(gpu):
    yield
    from squigglekit_amd import api
    assert api.last_event_plan()["guard_hits"] == 0
    assert api.last_hmm_stream_plan()["guard_hits"] == 0


def polya():
    from squigglekit_amd import api
    if "polya" not in _cache:
        _cache["polya"] = api.polya_model("synth_raw")
    return _cache["polya"]


def read(seed, n):
    if (seed, n) not in _cache:
        _cache[(seed, n)] = HR.small_drna_read(np.random.default_rng(seed), n)
    return _cache[(seed, n)]


def script(reads, chunk, end=True, slots=None):
    """every read pushed `chunk` samples at a time (chunk: one number, or one per read), all the slots that still have
    samples in one push; the last chunk of a read carries END"""
    S = len(reads)
    slots = list(range(S)) if slots is None else slots
    chunk = [chunk] * S if np.isscalar(chunk) else chunk
    at, ops = [0] * S, []
    while any(at[i] < len(reads[i]) for i in range(S)):
        sl, ch, en = [], [], []
        for i in range(S):
            if at[i] < len(reads[i]):
                c = reads[i][at[i]:at[i] + chunk[i]]
                at[i] += len(c)
                sl.append(slots[i]); ch.append(c); en.append(int(end and at[i] >= len(reads[i])))
        ops.append(("push", np.array(sl, dtype=np.int32), ch, np.array(en, dtype=np.int32)))
    return ops


def opened(want, slots_n):
    """per slot the gate record after the last push that named it"""
    last = {}
    for op_want in want:
        if op_want is not None:
            for i, g in enumerate(op_want["gate"]):
                last[op_want["slots"][i]] = (g, op_want["info"][i])
    return [last[s] for s in range(slots_n)]


def run(api, ora, params, calib, model, rule, ops, S, label, live_rule=None):
    want = GR.run_script(ora, params, calib, TARGETS, model, rule, ops, S, live_rule)
    for op, w in zip(ops, want):
        if w is not None:
            w["slots"] = [int(s) for s in op[1]]
    got, _ = GR.play(api, ora, params, calib, TARGETS, model, rule, ops, S, live_rule, label=label, want=want)
    return got, want


@pytest.mark.parametrize("n,chunk,min_body,calib", [(1500, 200, 200, 8), (3000, 250, 400, 129), (3000, 250, 400, 8)])
def test_the_gate_opens_and_the_mapping_side_starts_at_t0(gpu, ora, n, chunk, min_body, calib):
    """seeds 0 - 5, one slot each: every gate opens near the planted body start and at least calib levels are mapped"""
    from squigglekit_amd import api
    reads = [read(seed, n) for seed in range(6)]
    rule = GR.rule_of(5, min_body, 20.0, 0, 64)
    got, want = run(api, ora, RNA, calib, polya(), rule, script(reads, chunk), 6, "opens n=%d" % n, LIVE_RULE)
    planted = n - (n - (n // 25 + n // 15 + n // 4 + n // 10 + 6 + n // 10))
    for s, (g, info) in enumerate(opened(want, 6)):
        assert g["state"] == GR.OPEN and abs(int(g["t0"]) - planted) <= 35 and g["flags"] == 0, (s, g)
        assert info["state"] == LR.MAPPING and info["mapped"] >= calib and info["mapped"] == g["released"], (s, info)
    rec, info = got[-1][0], got[-1][1]
    assert (rec["rows"] == info["mapped"][None, :]).all() and np.isfinite(rec["dist"]).all()


@pytest.mark.parametrize("chunk", [1, 63, 64, 65, 200, 1500])
def test_the_opening_push_at_every_position_of_a_chunk_cut(gpu, ora, chunk):
    from squigglekit_amd import api
    reads = [read(seed, 1500) for seed in (range(2) if chunk == 1 else range(6))]
    rule = GR.rule_of(5, 200, 20.0, 0, 64)
    S = len(reads)
    got, want = run(api, ora, RNA, 8, polya(), rule, script(reads, chunk), S, "chunk %d" % chunk)
    for s, (g, info) in enumerate(opened(want, S)):
        assert g["state"] == GR.OPEN and info["state"] == LR.MAPPING and info["mapped"] >= 8, (s, g, info)


@pytest.mark.parametrize("hold", [64, 16, 4, 1])
def test_the_ring(gpu, ora, hold):
    """64 events cover the stretch between t0 and the decision; 4 and 1 never do and 16 not always: TRUNCATED exactly
    when an event from t0 on had been overwritten, and what is still held is released -- the reference's suffix.  The
    last slot gets its read in one push: nothing passes through its ring."""
    from squigglekit_amd import api
    reads = [read(seed, 1500) for seed in range(6)]
    rule = GR.rule_of(5, 200, 20.0, 0, hold)
    chunks = [200, 200, 150, 150, 70, 1500]
    got, want = run(api, ora, RNA, 8, polya(), rule, script(reads, chunks), 6, "hold %d" % hold)
    truncated = []
    for s, (g, info) in enumerate(opened(want, 6)):
        ev = detect_ref.events(reads[s], RNA)
        mine = [w["gate"][w["slots"].index(s)] for w in want if s in w["slots"]]
        at = next(j for j, q in enumerate(mine) if q["state"] == GR.OPEN)
        before = int(mine[at - 1]["events_cut"]) if at else 0           # the events cut before the opening push
        lost = ev[:max(0, before - hold)]
        assert g["state"] == GR.OPEN and g["dropped"] == len(lost), (s, g)
        truncated.append(bool((lost["start"] >= g["t0"]).any()))
        assert bool(g["flags"] & GR.TRUNCATED) == truncated[-1], (s, g)
        assert info["mapped"] == g["released"] >= 8
    assert not truncated[5] and sum(truncated) >= {64: 0, 16: 1, 4: 3, 1: 3}[hold] and (hold < 64 or not any(truncated))


@pytest.mark.parametrize("chunk,min_body", [(200, 200), (5, 5)])
def test_an_event_that_straddles_t0_is_dropped(gpu, ora, chunk, min_body):
    """a constant stretch planted across the start: the event that holds t0 is cut before the decision under chunks of
    200 samples and after it under chunks of 5 with min_body 5"""
    from squigglekit_amd import api
    x = read(0, 1500).copy()
    x[801:881] = 545
    rule = GR.rule_of(5, min_body, 20.0, 0, 64)
    got, want = run(api, ora, RNA, 8, polya(), rule, script([x], chunk), 1, "straddle %d" % chunk)
    g = want[-1]["gate"][0]
    ev = detect_ref.events(x, RNA)
    st = np.flatnonzero((ev["start"] < g["t0"]) & (ev["start"] + ev["length"] > g["t0"]))
    assert g["state"] == GR.OPEN and len(st) == 1                       # the premise
    at = next(j for j, w in enumerate(want) if w["gate"][0]["state"] == GR.OPEN)
    cut_at = next(j for j, w in enumerate(want) if w["gate"][0]["events_cut"] > st[0])
    assert (cut_at < at) == (chunk == 200) and cut_at != at
    keep = ev[ev["start"] >= g["t0"]]
    assert g["released"] == len(keep) == len(ev) - st[0] - 1 == got[-1][1]["events"][0]
    assert np.concatenate([w["released"][0] for w in want]).tobytes() == keep.tobytes()


def test_end_while_gating_give_up_reset_and_calibration_pairs(gpu, ora):
    """slot 0 ends while gating, slot 1 is given up on and gets samples afterwards, slot 2 opens, is reset with a
    calibration pair and reused with a read in other units; slot 3 is peeked at throughout"""
    from squigglekit_amd import api
    a, b, c = read(0, 1500), read(1, 1500), read(2, 1500)
    c2 = (2 * c.astype(np.int32) + 6).astype(np.int16)                 # (raw + -6) * 0.5 is c again, exactly
    i32 = lambda *v: np.array(v, dtype=np.int32)                        # noqa: E731
    rule = GR.rule_of(5, 200, 20.0, 1500, 64)
    ops = [("push", i32(3, 0), [EMPTY, EMPTY], None)]                   # peeks before any sample
    for k in range(5):
        ops.append(("push", i32(0, 3, 2), [a[k * 180:(k + 1) * 180], EMPTY, c[k * 300:(k + 1) * 300]], i32(k == 4, 0, k == 4)))
    ops.append(("push", i32(0, 2, 3), [EMPTY, EMPTY, EMPTY], i32(0, 1, 1)))     # ended slots, and END for a slot with nothing
    ops.append(("reset", i32(2, 0), np.array([[-6.0, 0.5], [0.0, 1.0]])))
    # slot 1: poly(A)-like samples only, given up on at 1 500; then more samples
    flat = np.clip(np.rint(np.random.default_rng(8).normal(560, 8, 2400)), 0, 32767).astype(np.int16)
    for k in range(5):
        ops.append(("push", i32(2, 1, 0), [c2[k * 300:(k + 1) * 300], flat[k * 400:(k + 1) * 400], b[k * 300:(k + 1) * 300]],
                    i32(k == 4, k == 4, k == 4)))
    ops.append(("reset", i32(1), None))
    ops.append(("push", i32(1, 2), [b, EMPTY], i32(1, 0)))
    got, want = run(api, ora, RNA, 8, polya(), rule, ops, 4, "end, give-up, reset", LIVE_RULE)
    g, info = want[5]["gate"], want[5]["info"]
    assert (g["state"][0], g["flags"][0], info["state"][0], info["events"][0]) == (GR.REJECTED, GR.ENDED, LR.UNDECIDABLE, 0)
    assert g["state"][2] == GR.OPEN and info["state"][2] == LR.MAPPING
    assert want[6]["gate"]["state"][2] == GR.REJECTED and want[6]["gate"]["flags"][2] == GR.ENDED      # slot 3: END, no sample
    gs1 = [int(w["gate"]["state"][1]) for w in want[8:13]]
    assert gs1 == [GR.GATING] * 3 + [GR.REJECTED] * 2 and want[12]["gate"]["flags"][1] == 0
    assert [int(w["info"]["state"][1]) for w in want[8:13]] == [LR.CALIBRATING] * 4 + [LR.UNDECIDABLE]
    assert want[12]["hrec"]["n_used"][1] == 1600 == want[12]["gate"]["decided_n"][1]
    # slot 2 again, in other units under the same cuts: the same decision on the same scores; other levels
    assert want[12]["gate"]["t0"][0] == want[5]["gate"]["t0"][2] and want[12]["gate"]["state"][0] == GR.OPEN
    assert want[12]["hrec"]["v"][0].tobytes() == want[5]["hrec"]["v"][2].tobytes()
    assert want[12]["info"]["mean"][0] != want[5]["info"]["mean"][2]
    assert want[14]["gate"]["state"][0] == GR.OPEN and want[14]["info"]["mapped"][0] >= 8   # slot 1 after its reset: one push


def test_wave_mates(gpu, ora):
    """65 slots in one push: gating, opening, open, rejected at END, given up on, ended and peeked-at slots side by side"""
    from squigglekit_amd import api
    rng = np.random.default_rng(31)
    reads, chunks = [], []
    for s in range(65):
        x = read(s % 6, 1500)
        if s % 9 == 4:
            x = x[:600 + 3 * s]                                         # ends while gating
        reads.append(x)
        chunks.append(int(rng.choice([90, 150, 200, 260, 400])))
    rule = GR.rule_of(5, 200, 20.0, 1000, 8)                            # 1 000 samples without a 200-sample body: given up on
    ops = script(reads, chunks, slots=[int(s) for s in rng.permutation(65)])
    every = np.arange(65, dtype=np.int32)
    ops.insert(3, ("push", every, [EMPTY] * 65, None))
    ops.insert(7, ("reset", every[::7].copy(), None))
    ops.append(("push", every, [EMPTY] * 65, np.ones(65, dtype=np.int32)))
    got, want = run(api, ora, RNA, 8, polya(), rule, ops, 65, "wave mates", LIVE_RULE)
    mixed = [set(w["gate"]["state"].tolist()) for w in want if w is not None and len(w["gate"]) > 40]
    assert any(m == {GR.GATING, GR.OPEN, GR.REJECTED} for m in mixed)
    flags = set()
    for w in want:
        if w is not None:
            flags |= set(w["gate"]["flags"].tolist())
    assert flags >= {0, GR.TRUNCATED, GR.ENDED}
    last = want[-1]["gate"]
    assert (last["state"] != GR.GATING).all()
    assert ((last["state"] == GR.REJECTED) & (last["flags"] == 0) & (last["decided_n"] >= 1000)).sum() >= 5     # given up on


def test_a_tie_model_whose_margin_lands_on_the_threshold(gpu, ora):
    """integer scores: the opening push has margin == min_margin exactly; state 2 of 6"""
    from squigglekit_amd import api
    rng = np.random.default_rng(427)
    model = HR.tie_model(rng, S=6)
    s = int(rng.integers(0, 5))
    x = rng.integers(-1, 5, 400).astype(np.int16)
    rule = GR.rule_of(s, 5, 1.0, 0, 16)
    got, want = run(api, ora, DNA, 8, model, rule, script([x], 37), 1, "tie model")
    at = next(j for j, w in enumerate(want) if w["gate"][0]["state"] == GR.OPEN)
    v = want[at]["hrec"]["v"][0]
    assert s == 2 and at == 2 and v[s] - np.delete(v, s).max() == 1.0 and want[at]["gate"]["t0"][0] == 90
    assert want[-1]["info"]["state"][0] == LR.MAPPING and want[-1]["info"]["mapped"][0] >= 8


def test_device_form_gives_the_host_form_bytes(gpu):
    from squigglekit_amd import api, _lib
    L = _lib.load()
    S, stride = 6, 256
    reads = [read(seed, 1500) for seed in range(6)]
    ops = script(reads, [250, 200, 150, 256, 90, 256])
    T = len(TARGETS)
    rule = api.live_rule(*LIVE_RULE)
    gate = GR.lib_gate(api, polya(), GR.rule_of(5, 200, 20.0, 1400, 8))
    sizes = (S * stride * 2, S * 4, S * 4, S * 4, T * S * 32, S * 40, S * 40, S * 32, S * 96)
    bufs = [L.sk_dev_alloc(n) for n in sizes]
    d_rows, d_slots, d_len, d_end, d_out, d_info, d_best, d_gate, d_hrec = bufs
    params = _lib.DetParams(*RNA)
    states = set()

    def gate_of(handle, m):
        """sk_live_gate_fetch into arrays of the push's m entries"""
        g, h = np.zeros(m, dtype=api.GATE_DTYPE), np.zeros(m, dtype=api.HMMS_DTYPE)
        _lib.check(L.sk_live_gate_fetch(handle, _lib.ptr(g), _lib.ptr(h)))
        return g, h

    def fetch_of(handle, m, cap):
        """sk_live_fetch likewise: off [m + 1] and up to cap values"""
        off, z = np.zeros(m + 1, dtype=np.int64), np.zeros(cap)
        _lib.check(L.sk_live_fetch(handle, _lib.ptr(off), _lib.ptr(z), cap))
        return off, z[:int(off[m])]

    try:
        with api.LiveMap(params, 8, TARGETS, S, gate=gate) as dev, api.LiveMap(params, 8, TARGETS, S, gate=gate) as host:
            for j, (_, slots, chunks, end) in enumerate(ops):
                m = len(slots)
                rows = np.zeros((m, stride), dtype=np.int16)
                lens = np.array([len(c) for c in chunks], dtype=np.int32)
                for i, c in enumerate(chunks):
                    rows[i, :len(c)] = c
                for d, a in ((d_rows, rows), (d_slots, slots), (d_len, lens), (d_end, end)):
                    _lib.check(L.sk_dev_upload(d, _lib.ptr(a), a.nbytes))
                _lib.check(L.sk_live_push_dev_i16(dev.handle, d_slots, m, d_rows, stride, d_len, d_end, C.byref(rule), d_out,
                                                  d_info, d_best))
                _lib.check(L.sk_live_gate_fetch_dev(dev.handle, d_gate, d_hrec))
                rec = np.zeros((T, m), dtype=api.MAPREC_DTYPE)
                info = np.zeros(m, dtype=api.LIVEINFO_DTYPE)
                best = np.zeros(m, dtype=api.LIVEBEST_DTYPE)
                g = np.zeros(m, dtype=api.GATE_DTYPE)
                hrec = np.zeros(m, dtype=api.HMMS_DTYPE)
                for a, d in ((rec, d_out), (info, d_info), (best, d_best), (g, d_gate), (hrec, d_hrec)):
                    _lib.check(L.sk_dev_download(_lib.ptr(a), d, a.nbytes))
                h_rec, h_info, h_best = host.push(slots, chunks, end=end, rule=rule)
                h_gate, h_hrec = host.gate()
                assert rec.tobytes() == h_rec.tobytes() and info.tobytes() == h_info.tobytes() and best.tobytes() == h_best.tobytes(), j
                assert g.tobytes() == h_gate.tobytes() and hrec.tobytes() == h_hrec.tobytes(), j
                d_g2, d_h2 = gate_of(dev.handle, m)
                assert d_g2.tobytes() == g.tobytes() and d_h2.tobytes() == hrec.tobytes(), j
                h_fetch = host.fetch()
                d_fetch = fetch_of(dev.handle, m, max(1, len(h_fetch[1])))
                assert d_fetch[0].tobytes() == h_fetch[0].tobytes() and d_fetch[1].tobytes() == h_fetch[1].tobytes(), j
                states |= set(g["state"].tolist())
            assert states == {GR.GATING, GR.OPEN}
            # samples for ended slots: the device form ignores them in both inner sessions, the host form refuses them
            every = np.arange(S, dtype=np.int32)
            rows = np.full((S, stride), 500, dtype=np.int16)
            for d, a in ((d_rows, rows), (d_slots, every), (d_len, np.full(S, 200, dtype=np.int32)), (d_end, np.zeros(S, dtype=np.int32))):
                _lib.check(L.sk_dev_upload(d, _lib.ptr(a), a.nbytes))
            before = host.push(every, [EMPTY] * S)
            before_gate = host.gate()
            _lib.check(L.sk_live_push_dev_i16(dev.handle, d_slots, S, d_rows, stride, d_len, d_end, None, d_out, d_info, None))
            after_gate = gate_of(dev.handle, S)
            rec = np.zeros((T, S), dtype=api.MAPREC_DTYPE)
            info = np.zeros(S, dtype=api.LIVEINFO_DTYPE)
            for a, d in ((rec, d_out), (info, d_info)):
                _lib.check(L.sk_dev_download(_lib.ptr(a), d, a.nbytes))
            assert rec.tobytes() == before[0].tobytes() and info.tobytes() == before[1].tobytes()
            assert after_gate[0].tobytes() == before_gate[0].tobytes() and after_gate[1].tobytes() == before_gate[1].tobytes()
            with pytest.raises(_lib.SquiggleKitError) as ei:
                dev.push([0], [np.ones(5, dtype=np.int16)])
            assert "has ended" in str(ei.value)
    finally:
        for b in bufs:
            L.sk_dev_free(b)


def test_plan_refusals_and_an_ungated_session_beside(gpu, ora):
    """the plan's bytes; what the session refuses, each leaving it as it was; an ungated session opened beside the gated
    one gives what live_ref expects, and takes neither calibration pairs nor a gate read-out"""
    from squigglekit_amd import api, _lib
    L = _lib.load()
    S, calib, hold = 5, 8, 16
    reads = [read(seed, 1500) for seed in range(3)]
    params = _lib.DetParams(*RNA)
    rule = GR.rule_of(5, 200, 20.0, 0, hold)
    i32 = lambda *v: np.array(v, dtype=np.int32)                        # noqa: E731
    err = lambda: L.sk_last_error().decode()                            # noqa: E731
    ops = script(reads, 300)
    with api.LiveMap(params, calib, TARGETS, S, gate=GR.lib_gate(api, polya(), rule)) as lm, \
            api.LiveMap(params, calib, TARGETS, S) as plain:
        g0 = lm.gate()
        assert len(g0[0]) == 0 and len(g0[1]) == 0                      # before the first push
        want = GR.run_script(ora, RNA, calib, TARGETS, polya(), rule, ops, S)
        want_plain = LR.run_script(ora, RNA, calib, TARGETS, GR.event_ops(ops), S)
        for j, op in enumerate(ops[:4]):
            res = lm.push(op[1], op[2], end=op[3])
            d = GR.check_push(res, lm.gate(), lm.fetch(), want[j])
            assert d is None, (j, d)
            plan = api.last_live_plan()
            inner = api.last_event_plan()["state_bytes"] + api.last_map_plan()["state_bytes"] + api.last_hmm_stream_plan()["state_bytes"]
            assert api.last_hmm_stream_plan()["state_bytes"] == S * 224
            assert plan["state_bytes"] == inner + S * (calib * 8 + 40) + S * (hold * 24 + 40)
            assert plan["bridged_levels"] == int(want[j]["off"][-1])
            res = plain.push(op[1], op[2], end=op[3])
            d = LR.check_push(res[0], res[1], plain.fetch(), None, want_plain[j])
            assert d is None, (j, d)
            plan = api.last_live_plan()
            assert plan["state_bytes"] == api.last_event_plan()["state_bytes"] + api.last_map_plan()["state_bytes"] + S * (calib * 8 + 40)
        # launches: a push of peeks hands nothing to the sweep in either session, so what differs is the gated session's
        # own three kernels -- the chunk lengths, the HMM push, the gate; with a rule both add the summary
        plain.push([0, 1, 2], [EMPTY] * 3)
        plain_launches = api.last_live_plan()["launches"]
        plain.push([0, 1, 2], [EMPTY] * 3, rule=LIVE_RULE)
        assert api.last_live_plan()["launches"] == plain_launches + 1
        state = (lm.push([0, 1, 2], [EMPTY] * 3), lm.gate())
        assert api.last_live_plan()["launches"] == plain_launches + 3 and api.last_live_plan()["bridged_levels"] == 0
        lm.push([0, 1, 2], [EMPTY] * 3, rule=LIVE_RULE)
        assert api.last_live_plan()["launches"] == plain_launches + 4
        # the ungated session: no pairs, no gate
        cal = np.array([[0.0, 1.0]])
        assert L.sk_live_reset_cal(plain.handle, _lib.ptr(i32(0)), 1, _lib.ptr(cal)) == _lib.SK_ERR_INVALID and "has no gate" in err()
        for fn in (L.sk_live_gate_fetch, L.sk_live_gate_fetch_dev):
            assert fn(plain.handle, None, None) == _lib.SK_ERR_INVALID and "has no gate" in err()
        with pytest.raises(ValueError):
            plain.reset([0], cal)
        with pytest.raises(ValueError):
            plain.gate()
        # the gated one: unknown handles, a slot outside, a stride whose events with the ring could pass the chunk limit
        assert L.sk_live_gate_fetch(7, None, None) == _lib.SK_ERR_INVALID and "unknown live session handle 7" in err()
        assert L.sk_live_reset_cal(lm.handle, _lib.ptr(i32(5)), 1, _lib.ptr(cal)) == _lib.SK_ERR_INVALID and "slot 5 is outside [0, 5)" in err()
        with api.LiveMap(params, _lib.SK_LIVE_MAX_CALIB, TARGETS[:1], 2,
                         gate=GR.lib_gate(api, polya(), GR.rule_of(5, 200, 20.0, 0, _lib.SK_LIVE_MAX_GATE_HOLD))) as big, \
                api.LiveMap(params, _lib.SK_LIVE_MAX_CALIB, TARGETS[:1], 2) as big_plain:
            # w_short 7: 4 samples per event at most -> 212 992 samples make 53 248 + 4 rows: inside with calib - 1, outside with hold
            n = 4 * (_lib.SK_MAP_MAX_CHUNK - _lib.SK_LIVE_MAX_CALIB - _lib.SK_LIVE_MAX_GATE_HOLD)
            wide = np.zeros((1, n), dtype=np.int16)
            out, info = np.full(32, 0xAB, dtype=np.uint8), np.full(40, 0xAB, dtype=np.uint8)
            args = (_lib.ptr(i32(0)), 1, _lib.ptr(wide), n, _lib.ptr(i32(16)), None, None, _lib.ptr(out), _lib.ptr(info), None)
            assert L.sk_live_push_i16(big.handle, *args) == _lib.SK_ERR_UNSUPPORTED and "hold = 4096 gated events" in err()
            assert np.all(out == 0xAB) and np.all(info == 0xAB)
            assert L.sk_live_push_i16(big_plain.handle, *args) == 0, err()
            _, binfo = big.push([0], [np.zeros(16, dtype=np.int16)])
            assert binfo["events"][0] == 0 and big.gate()[0]["events_cut"][0] == 0 and big.gate()[1]["n_used"][0] == 16
        # nothing moved
        again = (lm.push([0, 1, 2], [EMPTY] * 3), lm.gate())
        for a, b in zip(state[0] + state[1], again[0] + again[1]):
            assert a.tobytes() == b.tobytes()
        # a reset with pairs named twice is the event session's business as in an ungated session; NaN pairs never arrive
        for j, op in enumerate(ops[4:], 4):
            res = lm.push(op[1], op[2], end=op[3])
            d = GR.check_push(res, lm.gate(), lm.fetch(), want[j])
            assert d is None, (j, d)
        assert (lm.gate()[0]["state"] == GR.OPEN).all()
