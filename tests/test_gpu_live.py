"""GPU: live mapping sessions (sk_live_*, api.LiveMap) against tests/live_ref.py -- evstream_ref for the events a push
emits, numpy for levels, hold-back and normalisation, the oracle's dtw_subsequence for the records.  Every comparison is
== on bytes: the definition has no tolerance.  guard_hits is 0 after every test."""
import ctypes as C

import numpy as np
import pytest

import detect_ref
import evstream_ref as ER
import live_ref as LR

pytestmark = pytest.mark.gpu

DNA, RNA = detect_ref.PRESETS["dna"], detect_ref.PRESETS["rna"]
_rng = np.random.default_rng(2024)
TARGETS = [_rng.normal(size=n) for n in (150, 400, 1100)]            # one row passes 1 024 columns, one stays short
RULES = {"accept at once": (0, 1e30, -1e30, 2 ** 31 - 1), "never": (10 ** 9, 0.5, 0.05, 10 ** 9),
         "give up at 74": (10 ** 9, 0.5, 0.05, 74)}
_cache = {}


@pytest.fixture(autouse=True)
def no_guard_hit(gpu):
    yield
    from squigglekit_amd import api
    assert api.last_event_plan()["guard_hits"] == 0


def walk_read():
    if "walk" not in _cache:
        _cache["walk"] = ER.draw_read(np.random.default_rng(3), 6000, "walk")
    return _cache["walk"]


def mates(S):
    """the two wave-mates scripts of S slots (drawn once): shuffled subsets, empty chunks, ENDs and resets -- the first
    under the dna preset (many events: slots calibrate, map and are reset while mapping), the second under the
    parameters drawn with it"""
    if ("mates", S) not in _cache:
        rng = np.random.default_rng(140 + S)
        pair = [ER.draw_session(rng, nslots=S, budget=12000, maxlen=300) for _ in range(2)]
        pair[0]["params"] = DNA
        _cache[("mates", S)] = pair
    return _cache[("mates", S)]


def script_of_cuts(params, reads, cuts_per_read, end_with_last=True):
    from test_gpu_evstream import script_of_cuts as soc
    return soc(params, reads, cuts_per_read, end_with_last)


def even_cuts(n, c):
    return [c] * (n // c) + ([n % c] if n % c else [])


def levels(x, params):
    return LR.levels_of(detect_ref.events(x, params))


@pytest.mark.parametrize("preset", ["dna", "rna"])
@pytest.mark.parametrize("C", [2, 7, 8, 9, 40, 127, 128, 129, 300, 1000])
def test_calibration_grid(gpu, ora, preset, C):
    """one read pushed 500 samples at a time under every calibration length at an edge of numpy's summation: the serial
    loop (< 8), the unrolled leaf (<= 128), its first split"""
    from squigglekit_amd import api
    params = detect_ref.PRESETS[preset]
    x = walk_read()
    assert len(detect_ref.events(x, params)) > (1000 if preset == "dna" else 300)
    sess = script_of_cuts(params, [x], [even_cuts(len(x), 500)])
    got, want = LR.play(api, ora, params, C, TARGETS, sess["ops"], 1, label="calibration %s C=%d" % (preset, C))
    last = want[-1]["info"][0]
    assert last["state"] == LR.MAPPING and last["mapped"] == last["events"] and np.isfinite(last["mean"]) and last["sd"] > 0
    assert got[-1][1]["mean"].tobytes() == want[-1]["info"]["mean"].tobytes()
    assert got[-1][1]["sd"].tobytes() == want[-1]["info"]["sd"].tobytes()


def test_cuts_do_not_matter(gpu, ora):
    """the same read under seven sample cuts, one slot each: the final records are equal, and the oracle's on the
    normalised levels of the whole read"""
    from squigglekit_amd import api, _lib
    from squigglekit_amd.mapstream_cli import normalise
    x = walk_read()
    cuts = [[1] * 200 + even_cuts(len(x) - 200, 2000)] + [even_cuts(len(x), c) for c in (63, 64, 65, 777, 2000, len(x))]
    sess = script_of_cuts(DNA, [x] * len(cuts), cuts)
    final = {}
    with api.LiveMap(_lib.DetParams(*DNA), 40, TARGETS, len(cuts)) as lm:
        for op in sess["ops"]:
            rec, info = lm.push(op[1], op[2], end=op[3])
            for i, s in enumerate(op[1]):
                final[int(s)] = (rec[:, i].copy(), info[i].copy())
    z = normalise(levels(x, DNA), 40)
    fields = ["dist", "start", "end", "n", "flags", "rows"]             # (pushes differ with the cuts)
    for s in range(len(cuts)):
        rec, info = final[s]
        assert info["ended"] == 1 and info["state"] == LR.MAPPING and info["mapped"] == len(z)
        for f in fields:
            assert rec[f].tobytes() == final[0][0][f].tobytes(), (s, f)
        for t, y in enumerate(TARGETS):
            assert (rec["dist"][t], rec["start"][t], rec["end"][t]) == ora.dtw_subsequence(z, y), (s, t)
            assert rec["rows"][t] == len(z)


@pytest.mark.parametrize("end_with_last", [True, False])
def test_ends_before_calibration(gpu, ora, end_with_last):
    """reads that end with fewer than C levels: head is all of them; fewer than 2 events is UNDECIDABLE; later pushes to an
    ended slot change nothing"""
    from squigglekit_amd import api
    rng = np.random.default_rng(11)
    lens = [0, 1, 5, 11, 12, 300]
    reads = [ER.draw_read(rng, n, "steps") for n in lens]
    sess = script_of_cuts(DNA, reads, [[n] if n else [] for n in lens], end_with_last)
    S = len(lens)
    every = np.arange(S, dtype=np.int32)
    ops = sess["ops"] + [("push", every, [np.zeros(0, dtype=np.int16)] * S, np.zeros(S, dtype=np.int32)),
                         ("push", every[::-1].copy(), [np.zeros(0, dtype=np.int16)] * S, np.ones(S, dtype=np.int32))]
    got, want = LR.play(api, ora, DNA, 200, TARGETS, ops, S, label="ends before calibration")
    rec, info = got[-2][0], got[-2][1]
    for s, x in enumerate(reads):
        lev = levels(x, DNA)
        assert info["events"][s] == len(lev) and info["ended"][s] == 1 and info["held"][s] == 0
        if len(lev) < 2 or not lev.std() > 0:
            assert info["state"][s] == LR.UNDECIDABLE and np.isnan(info["mean"][s]) and np.isnan(info["sd"][s])
            assert np.isnan(rec["dist"][:, s]).all() and (rec["rows"][:, s] == 0).all() and (rec["start"][:, s] == -1).all()
        else:
            assert info["state"][s] == LR.MAPPING and info["mapped"][s] == len(lev)
            assert info["mean"][s] == lev.mean() and info["sd"][s] == lev.std()
    assert (info["state"][:2] == LR.UNDECIDABLE).all() and info["state"][5] == LR.MAPPING
    assert got[-1][0][:, ::-1].tobytes() == rec.tobytes()               # nothing moved


@pytest.mark.parametrize("seed,kind", [(10, "ties"), (124, "steps")])
def test_no_deviation(gpu, ora, seed, kind):
    """the first two levels are equal: UNDECIDABLE under C = 2, mapped under C = 3"""
    from squigglekit_amd import api
    x = ER.draw_read(np.random.default_rng(seed), 300, kind)
    lev = levels(x, DNA)
    assert len(lev) > 3 and lev[0] == lev[1] and lev[:3].std() > 0      # the premise
    sess = script_of_cuts(DNA, [x], [even_cuts(len(x), 100)])
    got, _ = LR.play(api, ora, DNA, 2, TARGETS, sess["ops"], 1, label="no deviation C=2")
    assert got[-1][1]["state"][0] == LR.UNDECIDABLE and got[-1][1]["events"][0] == len(lev) and got[-1][1]["mapped"][0] == 0
    assert np.isnan(got[-1][0]["dist"]).all()
    got, _ = LR.play(api, ora, DNA, 3, TARGETS, sess["ops"], 1, label="no deviation C=3")
    assert got[-1][1]["state"][0] == LR.MAPPING and got[-1][1]["mapped"][0] == len(lev)


@pytest.mark.parametrize("S", [1, 64, 65, 130])
def test_wave_mates_and_reset(gpu, ora, S):
    """pushes that name a shuffled subset: calibrating, mapping, undecidable and ended slots and empty chunks in one push,
    resets mid-calibration and mid-mapping"""
    from squigglekit_amd import api
    states = set()
    for k, sess in enumerate(mates(S)):
        got, want = LR.play(api, ora, sess["params"], 5, TARGETS, sess["ops"], S, label="wave mates S=%d/%d" % (S, k))
        for w in want:
            if w is not None:
                states |= set(w["info"]["state"].tolist())
    assert states == {LR.CALIBRATING, LR.MAPPING, LR.UNDECIDABLE}


def test_more_than_1024_levels_in_one_chunk(gpu, ora):
    """one push whose first chunk passes the mapping side's piece limit"""
    from squigglekit_amd import api
    x = walk_read()
    ops = [("push", np.array([0], dtype=np.int32), [x], np.array([1], dtype=np.int32))]
    got, want = LR.play(api, ora, DNA, 1000, TARGETS, ops, 1, label="1197 levels at once")
    assert got[0][1]["mapped"][0] == len(want[0]["z"]) > 1024 and got[0][0]["pushes"][0, 0] == 1


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("rule", sorted(RULES))
def test_decision_summary(gpu, rule, T):
    """best is map_lines' choice and map_decide's decision on the records the same push returned, byte for byte"""
    from squigglekit_amd import api, _lib
    seen = set()
    for S, k in ((1, 0), (64, 0), (65, 1), (130, 0)):
        sess = mates(S)[k]
        with api.LiveMap(_lib.DetParams(*sess["params"]), 5, TARGETS[:T], S) as lm:
            for j, op in enumerate(sess["ops"]):
                if op[0] == "reset":
                    lm.reset(op[1])
                    continue
                rec, info, best = lm.push(op[1], op[2], end=op[3], rule=RULES[rule])
                d = LR.same_bytes(best, LR.best_of(rec, RULES[rule]))
                assert d is None, "S=%d op %d: %s" % (S, j, d)
                b, dec = api.map_decide(rec, *RULES[rule])
                assert np.array_equal(best["target"], b) and np.array_equal(best["decision"], dec)
                seen |= set(best["decision"].tolist())
    assert seen == {"accept at once": {0, 1}, "never": {0}, "give up at 74": {0, -1}}[rule]


def test_device_form_gives_the_host_form_bytes(gpu):
    from squigglekit_amd import api, _lib
    L = _lib.load()
    S, stride = 65, 304
    sess = mates(S)[0]
    params = _lib.DetParams(*sess["params"])
    T = len(TARGETS)
    rule = api.live_rule(*RULES["give up at 74"])
    sizes = (S * stride * 2, S * 4, S * 4, S * 4, T * S * 32, S * 40, S * 40)
    bufs = [L.sk_dev_alloc(n) for n in sizes]
    d_rows, d_slots, d_len, d_end, d_out, d_info, d_best = bufs
    try:
        with api.LiveMap(params, 5, TARGETS, S) as dev, api.LiveMap(params, 5, TARGETS, S) as host:
            for j, op in enumerate(sess["ops"]):
                if op[0] == "reset":
                    dev.reset(op[1])
                    host.reset(op[1])
                    continue
                _, slots, chunks, end = op
                m = len(slots)
                rows = np.zeros((m, stride), dtype=np.int16)
                lens = np.array([len(c) for c in chunks], dtype=np.int32)
                for i, c in enumerate(chunks):
                    rows[i, :len(c)] = c
                for d, a in ((d_rows, rows), (d_slots, np.ascontiguousarray(slots, dtype=np.int32)), (d_len, lens),
                             (d_end, np.ascontiguousarray(end, dtype=np.int32))):
                    _lib.check(L.sk_dev_upload(d, _lib.ptr(a), a.nbytes))
                _lib.check(L.sk_live_push_dev_i16(dev.handle, d_slots, m, d_rows, stride, d_len, d_end, C.byref(rule), d_out,
                                                  d_info, d_best))
                rec = np.zeros((T, m), dtype=api.MAPREC_DTYPE)
                info = np.zeros(m, dtype=api.LIVEINFO_DTYPE)
                best = np.zeros(m, dtype=api.LIVEBEST_DTYPE)
                for a, d in ((rec, d_out), (info, d_info), (best, d_best)):
                    _lib.check(L.sk_dev_download(_lib.ptr(a), d, a.nbytes))
                dev._last_m = m
                h_rec, h_info, h_best = host.push(slots, chunks, end=end, rule=rule)
                assert rec.tobytes() == h_rec.tobytes() and info.tobytes() == h_info.tobytes(), j
                assert best.tobytes() == h_best.tobytes(), j
                d_fetch, h_fetch = dev.fetch(), host.fetch()
                assert d_fetch[0].tobytes() == h_fetch[0].tobytes() and d_fetch[1].tobytes() == h_fetch[1].tobytes(), j
            # the host form after device-form pushes: it knows which slots have ended (the script's last op ended all)
            with pytest.raises(_lib.SquiggleKitError) as ei:
                dev.push([0], [np.ones(5, dtype=np.int16)])
            assert "has ended" in str(ei.value)
            # the device form checks the slot numbers it reads back
            bad = np.array([S, 0], dtype=np.int32)
            _lib.check(L.sk_dev_upload(d_slots, _lib.ptr(bad), bad.nbytes))
            assert L.sk_live_push_dev_i16(dev.handle, d_slots, 2, d_rows, stride, d_len, d_end, None, d_out, d_info, None) == \
                _lib.SK_ERR_INVALID and "slot %d is outside [0, %d)" % (S, S) in L.sk_last_error().decode()
    finally:
        for b in bufs:
            L.sk_dev_free(b)


def test_refusals_that_need_the_session(gpu, ora):
    """a handle that is not open, a slot at or above nslots, samples for an ended slot, a ninth session, a stride whose
    events could pass SK_MAP_MAX_CHUNK: each refused with its words, each leaving the session and the outputs as they were"""
    from squigglekit_amd import api, _lib
    L = _lib.load()
    rng = np.random.default_rng(12)
    params = _lib.DetParams(*DNA)
    i32 = lambda *v: np.array(v, dtype=np.int32)                        # noqa: E731
    reads = [ER.draw_read(rng, 900, "steps") for _ in range(3)]
    T = len(TARGETS)

    def raw_push(handle, slots, rows, lens, end=None):
        out = np.full(T * len(slots) * 32, 0xAB, dtype=np.uint8)
        info = np.full(len(slots) * 40, 0xAB, dtype=np.uint8)
        rc = L.sk_live_push_i16(handle, _lib.ptr(slots), len(slots), _lib.ptr(rows), rows.shape[1], _lib.ptr(lens),
                                None if end is None else _lib.ptr(end), None, _lib.ptr(out), _lib.ptr(info), None)
        return rc, L.sk_last_error().decode(), bool(np.all(out == 0xAB) and np.all(info == 0xAB))

    with api.LiveMap(params, 8, TARGETS, 4) as lm:
        rec0, info0 = lm.push([0, 1, 2], reads, end=[0, 0, 1])
        assert info0["ended"].tolist() == [0, 0, 1] and (info0["events"] > 8).all() and (info0["state"] == LR.MAPPING).all()
        rows = np.zeros((2, 16), dtype=np.int16)
        for handle in range(8):
            if handle != lm.handle:
                rc, words, clean = raw_push(handle, i32(0, 1), rows, i32(16, 16))
                assert rc == _lib.SK_ERR_INVALID and "unknown live session handle %d" % handle in words and clean
        rc, words, clean = raw_push(lm.handle, i32(0, 4), rows, i32(16, 16))
        assert rc == _lib.SK_ERR_INVALID and "entry 1: slot 4 is outside [0, 4)" in words and clean
        rc, words, clean = raw_push(lm.handle, i32(0, 2), rows, i32(16, 16))
        assert rc == _lib.SK_ERR_INVALID and "entry 1: slot 2 has ended" in words and clean
        wide = np.zeros((1, 1 << 17), dtype=np.int16)
        with api.LiveMap(params, _lib.SK_LIVE_MAX_CALIB, TARGETS[:1], 2) as big:
            rc, words, clean = raw_push(big.handle, i32(0), wide, i32(16))
            assert rc == _lib.SK_ERR_UNSUPPORTED and "above %d points" % _lib.SK_MAP_MAX_CHUNK in words and clean
            _, binfo = big.push([0], [np.zeros(16, dtype=np.int16)])
            assert binfo["events"][0] == 0 and binfo["new_events"][0] == 0      # (nothing had been walked)
        # nothing moved: the slots answer an empty push with what they had
        rec1, info1 = lm.push([0, 1, 2], [np.zeros(0, dtype=np.int16)] * 3)
        assert rec1.tobytes() == rec0.tobytes()
        info0["new_events"] = 0
        assert info1.tobytes() == info0.tobytes()
        # a ninth session (the live table; each one also holds an event-session and a mapping-session handle)
        more = []
        try:
            for _ in range(_lib.SK_LIVE_MAX_SESSIONS - 1):
                more.append(api.LiveMap(params, 8, TARGETS[:1], 1))
            with pytest.raises(_lib.SquiggleKitError) as ei:
                api.LiveMap(params, 8, TARGETS[:1], 1)
            assert "8 live sessions are open" in str(ei.value)
        finally:
            for x in more:
                x.close()
        rec2, _ = lm.push([0, 1, 2], [np.zeros(0, dtype=np.int16)] * 3)
        assert rec2.tobytes() == rec0.tobytes()
    with pytest.raises(ValueError):
        lm.push([0], [np.zeros(0, dtype=np.int16)])                     # closed


def test_hits_and_plan(gpu):
    from squigglekit_amd import api, _lib
    rng = np.random.default_rng(13)
    S, Cal = 6, 9
    reads = [ER.draw_read(rng, n, "steps") for n in (900, 700, 4, 1200)]
    with api.LiveMap(_lib.DetParams(*DNA), Cal, TARGETS, S) as lm:
        slots = [4, 0, 2, 5]
        rec, info = lm.push(slots, reads, end=[0, 1, 0, 0])
        assert info["state"].tolist() == [LR.MAPPING, LR.MAPPING, LR.CALIBRATING, LR.MAPPING]
        plan = api.last_live_plan()
        inner = api.last_event_plan()["state_bytes"] + api.last_map_plan()["state_bytes"]
        assert plan["state_bytes"] == inner + S * (Cal * 8 + api.LIVEINFO_DTYPE.itemsize)
        off, z = lm.fetch()
        assert plan["bridged_levels"] == off[-1] == len(z) == int(info["mapped"].sum()) and plan["launches"] >= 3
        hits, count = lm.hits(slots, 2)
        assert hits.shape == (len(TARGETS), 4, 2)
        mapped = [0, 1, 3]
        assert np.ascontiguousarray(hits[:, mapped, 0]).tobytes() == np.ascontiguousarray(api.map_hits(rec)[:, mapped]).tobytes()
        assert (count[:, mapped] >= 1).all() and (count[:, 2] == 0).all()
    # context-manager use closed it; a second close is harmless
    lm.close()
