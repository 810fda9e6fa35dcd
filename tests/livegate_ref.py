"""The gated-live-session contract (include/squigglekit_hip.h, "Gated live sessions") in numpy and plain Python, on top
of hmmstream_ref (the HMM record of a slot), evstream_ref (which events a push emits), live_ref.Slot (hold-back and
normalisation) and mapstream_ref.Shadow (the oracle's record of what a slot has been handed).  A helper, not a test;
nothing here calls the library under test.

Per slot, since its reset: the gate is GATING, t0 = -1, the ring empty, the HMM slot fresh with the reset's pair.  A push:
  1. the chunk goes to the HMM slot only while the gate is GATING and the slot has not ended;
  2. while GATING, accept() on the HMM record -- api.polya_decide's three tests with `state` for TRANSCRIPT -- opens the
     gate at t0 = enter[state]; else n_used >= give_up > 0 rejects; else END rejects with flag ENDED;
  3. on the opening push the ring's events with start >= t0, oldest first, then the push's own with start >= t0 are
     released (TRUNCATED iff the ring had overwritten an event with start >= t0); an OPEN gate releases the push's events
     with start >= t0; a gate that stays GATING appends the push's events to its ring of the last G;
  4. the released events' levels are what live_ref.Slot.take is given, with the push's END flag.

run_script() returns what every op of a script must return."""
import numpy as np

import evstream_ref as ER
import hmmstream_ref as HR
import live_ref as LR
import mapstream_ref as MR

GATING, OPEN, REJECTED = 0, 1, 2
TRUNCATED, ENDED = 1, 2
GATE = np.dtype([("state", "<i4"), ("t0", "<i4"), ("decided_n", "<i4"), ("events_cut", "<i4"), ("released", "<i4"),
                 ("ring", "<i4"), ("dropped", "<i4"), ("flags", "<i4")])


def rule_of(state, min_body, min_margin, give_up=0, hold=1024):
    return {"state": int(state), "min_body": int(min_body), "min_margin": float(min_margin), "give_up": int(give_up),
            "hold": int(hold)}


def accept(rec, rule):
    """one HMM record (hmmstream_ref.DTYPE scalar): polya_decide's accept with rule["state"] in place of TRANSCRIPT"""
    s = rule["state"]
    v = np.asarray(rec["v"], dtype=np.float64)
    others = np.delete(v, s).max()
    with np.errstate(invalid="ignore"):
        margin = v[s] - others                                       # (-inf - -inf = NaN: the test fails)
        return bool(int(rec["final_state"]) == s and int(rec["n_used"]) - int(rec["enter"][s]) >= rule["min_body"]
                    and margin >= rule["min_margin"])


class Gate:
    def __init__(self, G):
        self.G = G
        self.state, self.t0, self.decided_n = GATING, -1, -1
        self.events_cut = self.released = self.dropped = self.flags = 0
        self.ring = []                                               # the last G events, oldest first
        self.last_drop = -1                                          # the start of the event overwritten last

    def take(self, hrec, new, end, rule):
        """the slot's HMM record after the push, the events the push cut and its END flag -> the released events"""
        was_gating = self.state == GATING
        if was_gating:
            if accept(hrec, rule):
                self.state, self.t0, self.decided_n = OPEN, int(hrec["enter"][rule["state"]]), int(hrec["n_used"])
            elif rule["give_up"] > 0 and int(hrec["n_used"]) >= rule["give_up"]:
                self.state, self.decided_n = REJECTED, int(hrec["n_used"])
            elif end:
                self.state, self.decided_n = REJECTED, int(hrec["n_used"])
                self.flags |= ENDED
        out = new[:0]
        if self.state == OPEN:
            cand = list(self.ring) + list(new) if was_gating else list(new)
            keep = [e for e in cand if int(e["start"]) >= self.t0]
            if was_gating and self.dropped > 0 and self.last_drop >= self.t0:
                self.flags |= TRUNCATED
            out = np.array(keep, dtype=new.dtype) if keep else new[:0]
            self.ring = []
        elif self.state == GATING:
            for e in new:
                self.ring.append(e)
                if len(self.ring) > self.G:
                    self.last_drop = int(self.ring.pop(0)["start"])
                    self.dropped += 1
        else:
            self.ring = []
        self.events_cut += len(new)
        self.released += len(out)
        return out

    def info(self):
        return (self.state, self.t0, self.decided_n, self.events_cut, self.released, len(self.ring), self.dropped, self.flags)


def event_ops(ops):
    """the script as evstream_ref reads it: resets without their pairs, an END flag per entry"""
    return [("reset", op[1]) if op[0] == "reset" else
            (op[0], op[1], op[2], np.zeros(len(op[1]), dtype=np.int32) if op[3] is None else op[3]) for op in ops]


def run_script(ora, params, C, targets, model, rule, ops, nslots, live_rule=None):
    """What every op of the script must give.  ops: ("reset", slots, cal2 or None) and ("push", slots, chunks, end or None).
    None for a reset; for a push a dict: rec, info, off, z, best as live_ref.run_script's, gate (GATE [m]), hrec
    (hmmstream_ref.DTYPE [m]) and released (the released event records per entry)."""
    events = iter(ER.run_session({"params": params, "nslots": nslots, "ops": event_ops(ops)}))
    hmm = HR.Session(model, nslots)
    shadow = MR.Shadow(ora, targets, nslots)
    slot = [LR.Slot() for _ in range(nslots)]
    gate = [Gate(rule["hold"]) for _ in range(nslots)]
    want = []
    for op in ops:
        if op[0] == "reset":
            sl = [int(s) for s in op[1]]
            for s in sl:
                slot[s], gate[s] = LR.Slot(), Gate(rule["hold"])
            hmm.reset(sl, op[2])
            shadow.reset(sl)
            want.append(None)
            continue
        _, slots, chunks, end = op
        m = len(slots)
        end = np.zeros(m, dtype=np.int32) if end is None else end
        eoff, erec = next(events)
        empty = np.zeros(0, dtype=np.int16)
        fed = [np.asarray(c) if gate[int(s)].state == GATING and not slot[int(s)].ended else empty
               for s, c in zip(slots, chunks)]
        hrec = hmm.push([int(s) for s in slots], fed, "i16") if m else HR.empty_records(0)
        zs, info, ginfo, released = [], np.zeros(m, dtype=LR.INFO), np.zeros(m, dtype=GATE), []
        for i, s in enumerate(slots):
            s = int(s)
            new = erec[int(eoff[i]):int(eoff[i + 1])]
            rel = gate[s].take(hrec[i], new, bool(end[i]), rule)
            released.append(rel)
            zs.append(slot[s].take(LR.levels_of(rel), end[i], C))
            info[i] = slot[s].info(len(rel))
            ginfo[i] = gate[s].info()
        rec = shadow.push([int(s) for s in slots], zs)
        off = np.zeros(m + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(z) for z in zs])
        want.append({"rec": rec, "info": info, "off": off, "z": np.concatenate(zs) if zs else np.zeros(0),
                     "best": None if live_rule is None else LR.best_of(rec, live_rule), "gate": ginfo, "hrec": hrec,
                     "released": released})
    return want


def describe_session(params, nslots, rule, ops):
    return "gate %r\n%s" % (rule, ER.describe_session({"params": params, "nslots": nslots, "ops": event_ops(ops)}))


def check_push(got, got_gate, got_fetch, want):
    """None, or what differs between a gated LiveMap push (rec, info[, best]), its gate() and fetch() and run_script's"""
    d = LR.check_push(got[0], got[1], got_fetch, got[2] if len(got) > 2 else None, want)
    if d is not None:
        return d
    if got_gate is not None:
        d = LR.same_bytes(got_gate[0], want["gate"])
        if d is not None:
            return "gate: " + d
        if got_gate[1].tobytes() != want["hrec"].tobytes():
            bad = [i for i in range(len(want["hrec"])) if got_gate[1][i].tobytes() != want["hrec"][i].tobytes()]
            return "hmm record %d: got %r, want %r" % (bad[0], got_gate[1][bad[0]], want["hrec"][bad[0]])
    return None


def lib_gate(api, model, rule):
    return api.live_gate(HR.lib_model(model), rule["min_body"], rule["min_margin"], rule["give_up"], rule["hold"], rule["state"])


def play(api, ora, params, C, targets, model, rule, ops, nslots, live_rule=None, label="", fetch=True, want=None):
    """Run the script on a gated api.LiveMap and compare every push -- records, info, fetch, best, gate(), the HMM records --
    with run_script; returns (the list of push results, run_script's list)."""
    from squigglekit_amd import _lib
    if want is None:
        want = run_script(ora, params, C, targets, model, rule, ops, nslots, live_rule)
    got = []
    with api.LiveMap(_lib.DetParams(*params), C, targets, nslots, gate=lib_gate(api, model, rule)) as lm:
        for j, op in enumerate(ops):
            if op[0] == "reset":
                lm.reset(op[1], op[2])
                got.append(None)
                continue
            res = lm.push(op[1], op[2], end=op[3], rule=live_rule)
            d = check_push(res, lm.gate(), lm.fetch() if fetch else None, want[j])
            assert d is None, "%s op %d: %s\n%s" % (label, j, d, describe_session(params, nslots, rule, ops))
            got.append(res)
    return got, want
