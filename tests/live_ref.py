"""The live-mapping-session contract (include/squigglekit_hip.h, "Live mapping sessions") in numpy and plain Python, on
top of evstream_ref (which events a push emits) and mapstream_ref.Shadow (the oracle's record of what a slot has been
handed).  A helper, not a test; nothing here calls the library under test.

Per slot, since its reset, lev[0 .. E) are the levels sum / length of the events emitted so far.  CALIBRATING: levels are
held back until there are C of them or the read has ended; then head = lev[:min(C, E)], mean = np.mean(head),
sd = np.std(head); fewer than 2 levels or not (sd > 0) makes the slot UNDECIDABLE, otherwise it is MAPPING and the chunk
handed on is (lev[0:E] - mean) / sd.  MAPPING: the chunk is (new levels - mean) / sd.  UNDECIDABLE: nothing is mapped.

run_script() returns what every op of a script must return; best_of() is the decision summary."""
import numpy as np

import evstream_ref as ER
import mapstream_ref as MR

CALIBRATING, MAPPING, UNDECIDABLE = 0, 1, 2
INFO = np.dtype([("mean", "<f8"), ("sd", "<f8"), ("events", "<i4"), ("mapped", "<i4"), ("held", "<i4"), ("state", "<i4"),
                 ("ended", "<i4"), ("new_events", "<i4")])
BEST = np.dtype([("dist", "<f8"), ("second_dist", "<f8"), ("target", "<i4"), ("start", "<i4"), ("end", "<i4"),
                 ("rows", "<i4"), ("second_target", "<i4"), ("decision", "<i4")])


def levels_of(rec):
    return rec["sum"].astype(np.float64) / rec["length"].astype(np.float64)


class Slot:
    def __init__(self):
        self.lev = np.zeros(0)
        self.state, self.mean, self.sd = CALIBRATING, np.nan, np.nan
        self.mapped, self.held, self.ended = 0, 0, False

    def take(self, new, end, C):
        """the new levels of a push and its END flag -> the chunk handed to the mapping side"""
        self.lev = np.concatenate([self.lev, new])
        self.ended = self.ended or bool(end)
        E = len(self.lev)
        chunk = np.zeros(0)
        if self.state == CALIBRATING:
            if E < C and not self.ended:
                self.held = E
            else:
                head = self.lev[:min(C, E)]
                sd = head.std() if head.size >= 2 else 0.0
                self.held = 0
                if not sd > 0:
                    self.state = UNDECIDABLE
                else:
                    self.state, self.mean, self.sd = MAPPING, head.mean(), sd
                    chunk = (self.lev - self.mean) / self.sd
        elif self.state == MAPPING:
            chunk = (np.asarray(new, dtype=np.float64) - self.mean) / self.sd
        self.mapped += len(chunk)
        return chunk

    def info(self, new_events):
        return (self.mean, self.sd, len(self.lev), self.mapped, self.held, self.state, int(self.ended), new_events)


def best_of(rec, rule):
    """BEST [m] of records [T, m]: map_lines' choice of the best and the second target per entry, map_decide's decision
    under rule = (min_rows, max_dist_per_row, min_margin, give_up_rows), one entry at a time in plain float64"""
    rec = np.asarray(rec)
    T, m = rec.shape
    min_rows, max_dpr, min_margin, give_up = rule
    out = np.zeros(m, dtype=BEST)
    for i in range(m):
        col = rec[:, i]
        d = np.where(np.isnan(col["dist"]), np.inf, col["dist"])
        b = int(np.argmin(d))
        has = not bool(np.isnan(col["dist"]).all())
        rest = d.copy()
        rest[b] = np.inf
        s = int(np.argmin(rest)) if T > 1 else -1
        rows = np.float64(col[b]["rows"])
        with np.errstate(invalid="ignore", divide="ignore"):
            accept = has and rows >= int(min_rows) and bool(d[b] / rows <= float(max_dpr))
            if T > 1:
                accept = accept and bool((rest[s] - d[b]) / rows >= float(min_margin))
        dec = 1 if accept else (-1 if has and rows >= int(give_up) else 0)
        out[i] = (col[b]["dist"] if has else np.nan, col[s]["dist"] if s >= 0 else np.nan, b if has else -1,
                  col[b]["start"] if has else -1, col[b]["end"] if has else -1, col[b]["rows"], s, dec)
    return out


def run_script(ora, params, C, targets, ops, nslots=None, rule=None):
    """What every op of the script must give: None for a ("reset", slots), and for a ("push", slots, chunks, end) a dict
    rec (MAPREC [T, m]), info (INFO [m]), off / z (the normalised chunks, compact) and best (BEST [m], or None without a
    rule)."""
    if nslots is None:
        nslots = 1 + max(int(np.max(op[1])) for op in ops if len(op[1]))
    events = iter(ER.run_session({"params": params, "nslots": nslots, "ops": ops}))
    shadow = MR.Shadow(ora, targets, nslots)
    slot = [Slot() for _ in range(nslots)]
    want = []
    for op in ops:
        if op[0] == "reset":
            for s in op[1]:
                slot[int(s)] = Slot()
            shadow.reset([int(s) for s in op[1]])
            want.append(None)
            continue
        _, slots, chunks, end = op
        end = np.zeros(len(slots), dtype=np.int32) if end is None else end
        eoff, erec = next(events)
        lev = levels_of(erec)
        zs, info = [], np.zeros(len(slots), dtype=INFO)
        for i, s in enumerate(slots):
            new = lev[int(eoff[i]):int(eoff[i + 1])]
            zs.append(slot[int(s)].take(new, end[i], C))
            info[i] = slot[int(s)].info(len(new))
        rec = shadow.push([int(s) for s in slots], zs)
        off = np.zeros(len(slots) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(z) for z in zs])
        want.append({"rec": rec, "info": info, "off": off, "z": np.concatenate(zs) if zs else np.zeros(0),
                     "best": None if rule is None else best_of(rec, rule)})
    return want


def same_bytes(got, want, names=None):
    """None, or a text naming the first field and index whose bytes differ"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "shape %s != %s" % (got.shape, want.shape)
    for f in names or want.dtype.names:
        a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        if a.dtype.kind == "f":
            a, b = a.view(np.uint64), b.view(np.uint64)
        if not np.array_equal(a, b):
            idx = tuple(int(v) for v in np.argwhere(a != b)[0])
            return "%s%s: got %r, want %r" % (f, list(idx), got[f][idx], want[f][idx])
    return None


def check_push(got_rec, got_info, got_fetch, got_best, want):
    """None, or what differs between a LiveMap push (and its fetch) and run_script's entry for it"""
    d = MR.first_difference(got_rec, want["rec"])
    if d is not None:
        return "rec: " + d
    d = same_bytes(got_info, want["info"])
    if d is not None:
        return "info: " + d
    if got_fetch is not None:
        off, z = got_fetch
        if not np.array_equal(off, want["off"]):
            return "fetch off %s, want %s" % (off[:12], want["off"][:12])
        if z.tobytes() != want["z"].tobytes():
            return "fetch values differ (%d values)" % len(z)
    if want["best"] is not None:
        d = same_bytes(got_best, want["best"])
        if d is not None:
            return "best: " + d
    return None


def play(api, ora, params, C, targets, ops, nslots, rule=None, label="", fetch=True):
    """Run the script on an api.LiveMap and compare every push with run_script; returns the list of (rec, info, best)."""
    from squigglekit_amd import _lib
    want = run_script(ora, params, C, targets, ops, nslots, rule)
    got = []
    with api.LiveMap(_lib.DetParams(*params), C, targets, nslots) as lm:
        for j, op in enumerate(ops):
            if op[0] == "reset":
                lm.reset(op[1])
                got.append(None)
                continue
            res = lm.push(op[1], op[2], end=op[3], rule=rule)
            d = check_push(res[0], res[1], lm.fetch() if fetch else None, res[2] if rule is not None else None, want[j])
            assert d is None, "%s op %d: %s\n%s" % (label, j, d, ER.describe_session({"params": params, "nslots": nslots, "ops": ops}))
            got.append(res)
    return got, want
