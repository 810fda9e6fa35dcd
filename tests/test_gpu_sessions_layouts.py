"""GPU: the device-form session pushes as a C caller uses them (tests/session_cases.py, parts B and C) against the
statement modules.  Every comparison is == on bytes.

Part B: one fixed script of 70 slots through sk_evs_push_dev_i16, sk_live_push_dev_i16 and sk_stream_push_dev_i16 under
five row layouts (stride, byte shift of the base): only (304, 0) and (304, 16 k) take the 16-byte loads of k_evs_push,
every other layout takes its 2-byte feed.  The padding behind every row's len is -12345 (32767 under one layout): a
sample read from there changes the records.
Part C: what include/squigglekit_hip.h says of the device forms: len is clamped into [0, stride], an entry whose slot is
outside the session is skipped, samples for an ended slot are ignored."""
import ctypes as C

import numpy as np
import pytest

import evstream_ref as ER
import hmmstream_ref as HR
import live_ref as LR
import session_cases as SC
import session_steps as SS

pytestmark = pytest.mark.gpu

_base = {}                           # what the (304, 0) layout gave, per session kind
MOTIF_W = 60


@pytest.fixture(autouse=True)
def no_guard_hit(gpu):
    yield
    from squigglekit_amd import api
    assert api.last_event_plan()["guard_hits"] == 0 and api.last_hmm_stream_plan()["guard_hits"] == 0


class Device:
    """device buffers for pushes of at most m entries of `stride` samples: freed on exit"""

    def __init__(self, m, stride, out_bytes):
        from squigglekit_amd import _lib
        self.lib, self.L = _lib, _lib.load()
        self.names = ("rows", "slots", "len", "end", "off", "out", "info", "best")
        sizes = (m * stride * 2 + 16, m * 4, m * 4, m * 4, (m + 1) * 8, out_bytes, m * 40, m * 40)
        self.p = {}
        for n, b in zip(self.names, sizes):
            self.p[n] = self.L.sk_dev_alloc(b)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.p.values():
            self.L.sk_dev_free(p)
        return False

    def up(self, name, a, shift=0):
        a = np.ascontiguousarray(a)
        if a.nbytes:
            self.lib.check(self.L.sk_dev_upload(self.p[name] + shift, self.lib.ptr(a), a.nbytes))

    def down(self, name, a):
        if a.nbytes:
            self.lib.check(self.L.sk_dev_download(self.lib.ptr(a), self.p[name], a.nbytes))
        return a

    def entries(self, step, shift):
        """upload one ("dev", slots, rows, lens, end) step; returns (m, stride, the rows' device address)"""
        _, slots, rows, lens, end = step
        self.up("rows", rows, shift)
        self.up("slots", np.asarray(slots, dtype=np.int32))
        self.up("len", np.asarray(lens, dtype=np.int32))
        self.up("end", np.asarray(end, dtype=np.int32))
        return len(slots), rows.shape[1], self.p["rows"] + shift


def steps_of(ops, stride, pad):
    """a statement script as device steps: ("reset", slots) and ("dev", slots, rows, lens, end)"""
    out = []
    for op in ops:
        if op[0] == "reset":
            out.append(op)
        else:
            rows, lens = SC.rows_of(op[2], stride, pad)
            out.append(("dev", op[1], rows, lens, op[3]))
    return out


def contract_steps():
    out = []
    for j, p in enumerate(SC.contract_script()):
        if j == SC.CONTRACT_RESET_BEFORE:
            out.append(("reset", np.array([5], dtype=np.int32)))
        out.append(("dev", p["slots"], p["rows"], p["len"], p["end"]))
    return out


def max_entries(steps):
    return max(len(st[1]) for st in steps)


# ---- the three sessions through their device forms ----------------------------------------------------------------------------
def event_dev(params, nslots, steps, shift=0):
    """[(off, rec)] of the device steps on a session of its own"""
    from squigglekit_amd import _lib, api
    m_max, stride = max_entries(steps), max(st[2].shape[1] for st in steps if st[0] == "dev")
    cap = m_max * ((stride + params[1]) // (params[0] // 2 + 1) + 3)
    got = []
    with Device(m_max, stride, cap * 24) as dv, api.EventStream(_lib.DetParams(*params), nslots) as es:
        for st in steps:
            if st[0] == "reset":
                es.reset(st[1])
                continue
            m, stride, d_rows = dv.entries(st, shift)
            _lib.check(dv.L.sk_evs_push_dev_i16(es.handle, dv.p["slots"], m, d_rows, stride, dv.p["len"], dv.p["end"],
                                                dv.p["off"], dv.p["out"], cap))
            off = dv.down("off", np.zeros(m + 1, dtype=np.int64))
            assert 0 <= off[m] <= cap
            got.append((off, dv.down("out", np.zeros(cap, dtype=api.DET_EVENT_DTYPE))[:int(off[m])]))
    return got


def live_dev(params, nslots, steps, shift=0):
    """[(rec, info, best, (off, z))] of the device steps on a session of its own"""
    from squigglekit_amd import _lib, api
    targets, T = SC.live_targets(), len(SC.live_targets())
    m_max, stride = max_entries(steps), max(st[2].shape[1] for st in steps if st[0] == "dev")
    rule = api.live_rule(*SC.LIVE_RULE)
    got = []
    with Device(m_max, stride, T * m_max * 32) as dv, api.LiveMap(_lib.DetParams(*params), SC.LIVE_CALIB, targets, nslots) as lm:
        for st in steps:
            if st[0] == "reset":
                lm.reset(st[1])
                continue
            m, stride, d_rows = dv.entries(st, shift)
            _lib.check(dv.L.sk_live_push_dev_i16(lm.handle, dv.p["slots"], m, d_rows, stride, dv.p["len"], dv.p["end"],
                                                 C.byref(rule), dv.p["out"], dv.p["info"], dv.p["best"]))
            rec = dv.down("out", np.zeros((T, m), dtype=api.MAPREC_DTYPE))
            info = dv.down("info", np.zeros(m, dtype=api.LIVEINFO_DTYPE))
            best = dv.down("best", np.zeros(m, dtype=api.LIVEBEST_DTYPE))
            lm._last_m = m
            got.append((rec, info, best, lm.fetch()))
    return got


def motifs():
    from squigglekit_amd import synth
    return [synth.synthetic_motif(17, seed=2), synth.synthetic_motif(40, seed=3)]


def motif_dev(nslots, steps, shift=0):
    """[rec STREAM_DTYPE [K, m]] of the device steps on a session of its own (END flags mean nothing to it)"""
    from squigglekit_amd import _lib, api
    K = len(motifs())
    m_max, stride = max_entries(steps), max(st[2].shape[1] for st in steps if st[0] == "dev")
    got = []
    with Device(m_max, stride, K * m_max * 40) as dv, api.MotifStream(motifs(), nslots, "medmad", 0, 1200, calib=MOTIF_W) as ms:
        for st in steps:
            if st[0] == "reset":
                ms.reset(st[1])
                continue
            m, stride, d_rows = dv.entries(st, shift)
            _lib.check(dv.L.sk_stream_push_dev_i16(ms.handle, dv.p["slots"], m, d_rows, stride, dv.p["len"], dv.p["out"]))
            got.append(dv.down("out", np.zeros((K, m), dtype=_lib.STREAM_DTYPE)))
    return got


# ---- the statements, once per process ---------------------------------------------------------------------------------------
def want_event(ops, nslots):
    return ER.run_session({"params": SC.DNA, "nslots": nslots, "ops": ops})


def want_live(ora, ops, nslots):
    return [w for w in LR.run_script(ora, SC.DNA, SC.LIVE_CALIB, SC.live_targets(), ops, nslots, SC.LIVE_RULE) if w is not None]


def check_event(got, want, label):
    assert len(got) == len(want)
    for j, ((off, rec), (w_off, w_rec)) in enumerate(zip(got, want)):
        assert np.array_equal(off, w_off) and rec.tobytes() == w_rec.tobytes(), "%s push %d: off %s want %s" % (label, j, off[:12], w_off[:12])


def check_live(got, want, label):
    assert len(got) == len(want)
    for j, ((rec, info, best, fetch), w) in enumerate(zip(got, want)):
        d = LR.check_push(rec, info, fetch, best, w)
        assert d is None, "%s push %d: %s" % (label, j, d)


def check_motif(got, ops, nslots, label):
    """against stream_ref.record on every slot's samples so far"""
    want = SS.motif_expectations({"motifs": motifs(), "nslots": nslots, "ops": ops}, MOTIF_W, "medmad", 0, 1200)
    pushes = [op for op in ops if op[0] != "reset"]
    assert len(got) == len(want) == len(pushes)
    for j, (rec, w, op) in enumerate(zip(got, want, pushes)):
        SS.check_motif_records(rec, w, op[1], "%s push %d" % (label, j))


def same_runs(a, b):
    """two runs' outputs byte for byte (nested tuples / lists of arrays)"""
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and a.tobytes() == b.tobytes()
    return len(a) == len(b) and all(same_runs(x, y) for x, y in zip(a, b))


def base_run(kind):
    if kind not in _base:
        sess = SC.layout_script()
        steps = steps_of(sess["ops"], 304, SC.PAD)
        _base[kind] = {"event": lambda: event_dev(SC.DNA, sess["nslots"], steps),
                       "live": lambda: live_dev(SC.DNA, sess["nslots"], steps),
                       "motif": lambda: motif_dev(sess["nslots"], steps)}[kind]()
    return _base[kind]


# ---- part B ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", SC.LAYOUTS, ids=lambda v: "stride%d+%d" % v)
def test_event_session_row_layouts(gpu, layout):
    sess = SC.layout_script()
    stride, shift = layout
    got = event_dev(SC.DNA, sess["nslots"], steps_of(sess["ops"], stride, SC.pad_of(layout)), shift)
    check_event(got, want_event(sess["ops"], sess["nslots"]), "event %r" % (layout,))
    assert same_runs(got, base_run("event"))


@pytest.mark.parametrize("layout", SC.LAYOUTS, ids=lambda v: "stride%d+%d" % v)
def test_live_session_row_layouts(gpu, ora, layout):
    sess = SC.layout_script()
    stride, shift = layout
    got = live_dev(SC.DNA, sess["nslots"], steps_of(sess["ops"], stride, SC.pad_of(layout)), shift)
    check_live(got, want_live(ora, sess["ops"], sess["nslots"]), "live %r" % (layout,))
    assert same_runs(got, base_run("live"))


@pytest.mark.parametrize("layout", SC.LAYOUTS, ids=lambda v: "stride%d+%d" % v)
def test_motifseq_session_row_layouts(gpu, ora, layout):
    sess = SC.layout_script()
    stride, shift = layout
    got = motif_dev(sess["nslots"], steps_of(sess["ops"], stride, SC.pad_of(layout)), shift)
    check_motif(got, sess["ops"], sess["nslots"], "motifseq %r" % (layout,))
    assert same_runs(got, base_run("motif"))


@pytest.mark.parametrize("kind", ["event", "live", "motif"])
def test_host_form_takes_rows_of_stride_303(gpu, ora, kind):
    """a (rows, lens) tuple goes through the wrappers as it is: the host forms copy rows of an odd pitch"""
    from squigglekit_amd import _lib, api
    sess = SC.layout_script()
    S, ops = sess["nslots"], sess["ops"]
    params = _lib.DetParams(*SC.DNA)
    got = []
    if kind == "event":
        with api.EventStream(params, S) as es:
            for op in ops:
                got.append(es.push(op[1], SC.rows_of(op[2], 303, SC.PAD_ONE), end=op[3]))
        check_event(got, want_event(ops, S), "event, host form")
    elif kind == "live":
        with api.LiveMap(params, SC.LIVE_CALIB, SC.live_targets(), S) as lm:
            for op in ops:
                got.append(lm.push(op[1], SC.rows_of(op[2], 303, SC.PAD_ONE), end=op[3], rule=SC.LIVE_RULE) + (lm.fetch(),))
        check_live(got, want_live(ora, ops, S), "live, host form")
    else:
        with api.MotifStream(motifs(), S, "medmad", 0, 1200, calib=MOTIF_W) as ms:
            for op in ops:
                got.append(ms.push(op[1], SC.rows_of(op[2], 303, SC.PAD_ONE)))
        check_motif(got, ops, S, "motifseq, host form")
    assert same_runs(got, base_run(kind))


# ---- part C ---------------------------------------------------------------------------------------------------------------
def kept_of(keep, m):
    return np.array(keep, dtype=np.int64), np.array([i for i in range(m) if i not in keep], dtype=np.int64)


def test_event_device_form_contract(gpu):
    """sk_evs_push_dev_i16: len -5 is 0 and stride + 9 is stride; an entry whose slot is -1 or nslots is ignored -- its
    span is empty and every other entry has the records it has without it; samples for an ended slot change nothing, and
    after a reset the slot works"""
    ops, keep = SC.contract_ops(True)
    want = want_event(ops, SC.CONTRACT_SLOTS)
    got = event_dev(SC.DNA, SC.CONTRACT_SLOTS, contract_steps())
    assert len(got) == len(want) == len(keep)
    for j, ((off, rec), (w_off, w_rec), p) in enumerate(zip(got, want, SC.contract_script())):
        k, skipped = kept_of(keep[j], len(p["slots"]))
        cnt = np.diff(off)
        assert (cnt[skipped] == 0).all(), (j, cnt)
        assert np.array_equal(cnt[k], np.diff(w_off)) and rec.tobytes() == w_rec.tobytes(), (j, cnt, np.diff(w_off))


def test_live_device_form_contract(gpu, ora):
    """sk_live_push_dev_i16: clamping and the ended slot as in the event session; the slots are read back and checked, so
    an entry outside the session is refused and nothing is written"""
    from squigglekit_amd import _lib, api
    ops, keep = SC.contract_ops(True)
    steps, j = [], 0
    for st in contract_steps():                                          # the entries that name a slot, as the caller wrote them
        if st[0] == "dev":
            k = keep[j]
            st = ("dev", [st[1][i] for i in k], st[2][k], [st[3][i] for i in k], [st[4][i] for i in k])
            j += 1
        steps.append(st)
    check_live(live_dev(SC.DNA, SC.CONTRACT_SLOTS, steps), want_live(ora, ops, SC.CONTRACT_SLOTS), "live contract")
    # the refusal
    T, S, st = len(SC.live_targets()), SC.CONTRACT_SLOTS, SC.CONTRACT_STRIDE
    p = SC.contract_script()[0]
    with Device(6, st, T * 6 * 32) as dv, api.LiveMap(_lib.DetParams(*SC.DNA), SC.LIVE_CALIB, SC.live_targets(), S) as lm:
        first = lm.push(p["slots"], (p["rows"], np.full(6, st, dtype=np.int32)))
        for bad in (-1, S):
            slots = [3, bad, 0, 1, 5, 2]
            dv.entries(("dev", slots, p["rows"], [st] * 6, [0] * 6), 0)
            fill = np.full(T * 6 * 32, 0xAB, dtype=np.uint8)
            dv.up("out", fill)
            dv.up("info", fill[:6 * 40])
            rc = dv.L.sk_live_push_dev_i16(lm.handle, dv.p["slots"], 6, dv.p["rows"], st, dv.p["len"], dv.p["end"], None,
                                           dv.p["out"], dv.p["info"], None)
            assert rc == _lib.SK_ERR_INVALID and "entry 1: slot %d is outside [0, %d)" % (bad, S) in dv.L.sk_last_error().decode()
            assert (dv.down("out", np.zeros_like(fill)) == 0xAB).all() and (dv.down("info", np.zeros(6 * 40, dtype=np.uint8)) == 0xAB).all()
        again = lm.push(p["slots"], [np.zeros(0, dtype=np.int16)] * 6)   # nothing moved
        first[1]["new_events"] = 0
        assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()


def test_motifseq_device_form_contract(gpu, ora):
    """sk_stream_push_dev_i16: clamping; an entry whose slot is out of range is skipped: NaN, -1 and zero counts"""
    from squigglekit_amd import _lib
    ops, keep = SC.contract_ops(False)
    got = motif_dev(SC.CONTRACT_SLOTS, contract_steps())
    empty = np.zeros(1, dtype=_lib.STREAM_DTYPE)
    empty["dist"], empty["tail"], empty["start"], empty["end"] = np.nan, np.nan, -1, -1
    inside = []
    for j, (rec, p) in enumerate(zip(got, SC.contract_script(False))):
        k, skipped = kept_of(keep[j], len(p["slots"]))
        for i in skipped:
            for row in rec[:, i]:
                assert LR.same_bytes(row.reshape(1), empty) is None, (j, i, row)
        inside.append(np.ascontiguousarray(rec[:, k]))
    check_motif(inside, ops, SC.CONTRACT_SLOTS, "motifseq contract")


@pytest.mark.parametrize("feed", ["i16", "f64"])
def test_hmm_device_form_contract(gpu, feed):
    """sk_hmms_push_dev_i16 / _f64: len is clamped (the float64 form takes offsets: nothing to clamp); an entry whose
    slot is outside gets the empty record and nobody else is touched"""
    from squigglekit_amd import _lib, api
    model = api.polya_model("synth_raw")
    ops, keep = SC.contract_ops(False)
    ref = HR.Session(model, SC.CONTRACT_SLOTS)
    st = SC.CONTRACT_STRIDE
    with Device(6, st, 6 * 96) as dv, api.HmmStream(model, SC.CONTRACT_SLOTS) as hs:
        d_vals = dv.L.sk_dev_alloc(6 * st * 8 + 8)
        try:
            j = 0
            for op, step in zip(ops, contract_steps()):
                if op[0] == "reset":
                    hs.reset(op[1])
                    ref.reset(op[1])
                    continue
                _, slots, rows, lens, _ = step
                m = len(slots)
                if feed == "i16":
                    dv.entries(step, 0)
                    _lib.check(dv.L.sk_hmms_push_dev_i16(hs.handle, dv.p["slots"], m, dv.p["rows"], st, dv.p["len"], dv.p["out"]))
                else:
                    parts = [rows[i, :min(max(int(n), 0), st)].astype(np.float64) for i, n in enumerate(lens)]
                    off = np.zeros(m + 1, dtype=np.int64)
                    off[1:] = np.cumsum([len(c) for c in parts])
                    vals = np.concatenate(parts + [np.zeros(1)])
                    dv.up("slots", np.asarray(slots, dtype=np.int32))
                    dv.up("off", off)
                    _lib.check(dv.L.sk_dev_upload(d_vals, _lib.ptr(vals), vals.nbytes))
                    _lib.check(dv.L.sk_hmms_push_dev_f64(hs.handle, dv.p["slots"], m, d_vals, dv.p["off"], dv.p["out"]))
                got = dv.down("out", np.zeros(m, dtype=api.HMMS_DTYPE))
                k, skipped = kept_of(keep[j], m)
                assert got[skipped].tobytes() == HR.empty_records(len(skipped)).tobytes(), (j, got[skipped])
                chunks = op[2] if feed == "i16" else [c.astype(np.float64) for c in op[2]]
                HR.assert_records(np.ascontiguousarray(got[k]), ref.push(op[1], chunks, feed), op[1], "hmm contract %s push %d" % (feed, j))
                j += 1
            assert j == len(keep)
            assert hs.peek(np.arange(SC.CONTRACT_SLOTS)).tobytes() == ref.records(np.arange(SC.CONTRACT_SLOTS)).tobytes()
        finally:
            dv.L.sk_dev_free(d_vals)
