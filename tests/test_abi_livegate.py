"""CPU: the C ABI of the gated live mapping sessions -- the header declares the entries with the signatures _lib.ABI
binds, the built library exports them, the rule is 24 bytes and the gate record 32, and every refusal the arguments alone
decide is made before a device is looked for: the same codes and messages on any machine.  No compute calls here."""
import ctypes as C
import os
import re

import numpy as np

import hmmstream_ref as HR
from conftest import ROOT

ENTRIES = ("sk_live_open_gated", "sk_live_reset_cal", "sk_live_gate_fetch", "sk_live_gate_fetch_dev", "sk_live_gate_last_ms")
CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}


def err(L):
    return L.sk_last_error().decode()


def test_header_declares_and_library_exports_the_entries():
    from squigglekit_amd import _lib, api
    text = open(os.path.join(ROOT, "include", "squigglekit_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
        assert m, name
        res, argt = _lib.ABI[name]
        assert res is C.c_int
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == len(argt), (name, args)
        for a, t in zip(args, argt):                                   # pointers bind as pointers, numbers by type
            if "*" in a:
                assert t is C.c_void_p or issubclass(t, C._Pointer), (name, a, t)
            else:
                assert t is CTYPE[a.split()[0]], (name, a, t)
    assert re.search(r"#define\s+SK_LIVE_MAX_GATE_HOLD\s+4096\b", code) and _lib.SK_LIVE_MAX_GATE_HOLD == 4096
    assert re.search(r"enum\s*\{\s*SK_LIVE_GATE_GATING\s*=\s*0\s*,\s*SK_LIVE_GATE_OPEN\s*=\s*1\s*,\s*SK_LIVE_GATE_REJECTED\s*=\s*2\s*\}", code)
    assert re.search(r"enum\s*\{\s*SK_LIVE_GATE_TRUNCATED\s*=\s*1\s*,\s*SK_LIVE_GATE_ENDED\s*=\s*2\s*\}", code)
    assert (_lib.SK_LIVE_GATE_GATING, _lib.SK_LIVE_GATE_OPEN, _lib.SK_LIVE_GATE_REJECTED) == (0, 1, 2)
    assert (_lib.SK_LIVE_GATE_TRUNCATED, _lib.SK_LIVE_GATE_ENDED) == (1, 2)
    _lib.build()
    lib = C.CDLL(_lib.SO_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert api.live_gate and api.LiveMap.gate
    assert _lib.GATE_DTYPE.itemsize == 32 and C.sizeof(_lib.LiveGate) == 24 and _lib.HMMS_DTYPE.itemsize == 96
    # the structs as the header spells them: field names in order
    for struct, names in (("sk_live_gate_info", _lib.GATE_DTYPE.names), ("sk_live_gate", tuple(f[0] for f in _lib.LiveGate._fields_))):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), code, flags=re.S).group(1)
        got = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
        assert tuple(got) == tuple(names), (struct, got)


def test_the_python_gate_is_the_rule_in_polya_decides_argument_order():
    from squigglekit_amd import api
    model, g = api.live_gate(api.polya_model("synth_raw"), 200, 20.0)
    assert (g.state, g.min_body, g.give_up, g.hold, g.min_margin) == (api.TRANSCRIPT, 200, 0, 1024, 20.0)
    model, g = api.live_gate(model, 5, -1.5, give_up=900, hold=7, state=2)
    assert (g.state, g.min_body, g.give_up, g.hold, g.min_margin) == (2, 5, 900, 7, -1.5)


def test_open_refusals_come_from_the_arguments_alone():
    from squigglekit_amd import _lib, api
    L = _lib.load()
    INV = _lib.SK_ERR_INVALID
    h = C.c_int32(-7)
    good = _lib.DetParams()
    tg = np.zeros(30, dtype=np.float64)
    toff = np.array([0, 10, 30], dtype=np.int64)
    polya = api.polya_model("synth_raw")
    rule = _lib.LiveGate(5, 200, 0, 64, 20.0)

    def op(p=good, calib=40, t=tg, o=toff, T=2, S=4, mdl=polya, g=rule, hd=h):
        q = lambda a: None if a is None else _lib.ptr(a)                # noqa: E731
        r = lambda a: None if a is None else C.byref(a)                 # noqa: E731
        return L.sk_live_open_gated(r(p), calib, q(t), q(o), T, S, r(mdl), r(g), r(hd))

    # sk_live_open's, in its order
    assert op(p=_lib.DetParams(0, 6, 1.4, 9.0, 0.2)) == INV and "1 <= w_short <= w_long <= 64" in err(L)
    assert op(hd=None) == INV and "NULL handle" in err(L)
    assert op(calib=1) == INV and "calib = 1 is outside 2 .. 8192" in err(L)
    assert op(t=None) == INV and "NULL targets/target_off" in err(L)
    assert op(S=0) == INV and "nslots = 0 is outside 1 .. 65536" in err(L)
    assert op(o=np.array([0, 10, 10], dtype=np.int64)) == INV and "target 1 is empty" in err(L)
    # then the model and the gate
    assert op(mdl=None) == INV and "NULL model/gate" in err(L)
    assert op(g=None) == INV and "NULL model/gate" in err(L)
    tie = HR.tie_model(np.random.default_rng(0), S=3)
    for broken, words in ((dict(tie, nstates=0), "nstates must lie in [1, 6]"),      # sk_hmms_open's rules and messages
                          (dict(tie, nstates=7), "nstates must lie in [1, 6]"),
                          (dict(tie, linit=np.full(3, -np.inf)), "at least one linit must be finite"),
                          (dict(tie, mu=np.full((3, 2), np.nan)), "mu must be finite")):
        mdl = _lib.HmmModel.from_arrays(broken["nstates"], broken["linit"], broken["ltrans"], broken["c"], broken["mu"], broken["h"])
        assert op(mdl=mdl) == INV and "sk_hmm_model: " + words in err(L), err(L)
        assert L.sk_hmms_open(C.byref(mdl), 4, C.byref(h)) == INV and "sk_hmm_model: " + words in err(L)
    three = HR.lib_model(tie)
    for state, S in ((-1, 6), (6, 6), (3, 3), (5, 3)):
        mdl = polya if S == 6 else three
        assert op(mdl=mdl, g=_lib.LiveGate(state, 200, 0, 64, 20.0)) == INV and \
            "gate: state = %d is outside [0, nstates = %d)" % (state, S) in err(L), err(L)
    for mb in (0, -4):
        assert op(g=_lib.LiveGate(5, mb, 0, 64, 20.0)) == INV and "gate: min_body = %d is below 1" % mb in err(L)
    for hold in (0, -1, 4097):
        assert op(g=_lib.LiveGate(5, 200, 0, hold, 20.0)) == INV and "gate: hold = %d is outside 1 .. 4096" % hold in err(L)
    assert op(g=_lib.LiveGate(5, 200, 0, 64, float("nan"))) == INV and "gate: min_margin must be a number" in err(L)
    # the order: the live session's arguments before the model, the model before the gate, state before min_body before hold
    assert op(calib=1, mdl=None) == INV and "calib = 1" in err(L)
    assert op(mdl=None, g=_lib.LiveGate(9, 0, 0, 0, 20.0)) == INV and "NULL model/gate" in err(L)
    assert op(g=_lib.LiveGate(9, 0, 0, 0, float("nan"))) == INV and "state = 9" in err(L)
    assert op(g=_lib.LiveGate(5, 0, 0, 0, float("nan"))) == INV and "min_body = 0" in err(L)
    assert op(g=_lib.LiveGate(5, 1, 0, 0, float("nan"))) == INV and "hold = 0" in err(L)
    assert h.value == -7
    # give_up <= 0 and an infinite margin are rules, not mistakes
    if L.sk_device_count() <= 0:
        assert op() == _lib.SK_ERR_NO_DEVICE, err(L)
        assert op(g=_lib.LiveGate(0, 1, -5, 1, float("inf"))) == _lib.SK_ERR_NO_DEVICE, err(L)


def test_reset_cal_and_gate_fetch_refusals_come_from_the_arguments_alone():
    from squigglekit_amd import _lib
    L = _lib.load()
    INV = _lib.SK_ERR_INVALID
    i32 = lambda *v: np.array(v, dtype=np.int32)                        # noqa: E731
    cal = np.array([[0.0, 1.0], [3.0, 0.5]])
    gate = np.full(2 * 32, 0xAB, dtype=np.uint8)
    rec = np.full(2 * 96, 0xAB, dtype=np.uint8)
    for handle in (-1, 8, 99):
        assert L.sk_live_reset_cal(handle, _lib.ptr(i32(0, 1)), 2, _lib.ptr(cal)) == INV and \
            "live session handle %d is outside [0, 8)" % handle in err(L)
        for fn in (L.sk_live_gate_fetch, L.sk_live_gate_fetch_dev):
            assert fn(handle, _lib.ptr(gate), _lib.ptr(rec)) == INV and "live session handle %d is outside [0, 8)" % handle in err(L)
    assert L.sk_live_reset_cal(0, _lib.ptr(i32(0)), -1, _lib.ptr(cal)) == INV and "m < 0" in err(L)
    assert L.sk_live_reset_cal(0, None, 2, _lib.ptr(cal)) == INV and "NULL slots" in err(L)
    assert L.sk_live_reset_cal(0, _lib.ptr(i32(0, 1)), 2, None) == INV and "NULL cal2" in err(L)
    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, 1, 2, 3):
            c2 = cal.copy()
            c2.reshape(-1)[at] = bad
            assert L.sk_live_reset_cal(0, _lib.ptr(i32(0, 1)), 2, _lib.ptr(c2)) == INV and \
                "entry %d: the calibration pair {offset, unit} must be finite" % (at // 2) in err(L), err(L)
    assert np.all(gate == 0xAB) and np.all(rec == 0xAB)
    if L.sk_device_count() <= 0:
        assert L.sk_live_reset_cal(0, _lib.ptr(i32(0, 1)), 2, _lib.ptr(cal)) == _lib.SK_ERR_NO_DEVICE, err(L)
        assert L.sk_live_gate_fetch(0, None, None) == _lib.SK_ERR_NO_DEVICE, err(L)
