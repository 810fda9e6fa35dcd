"""The reference pile-up, stated in numpy (the contract of sk_pileup / api.pileup: "Reference pile-up" in
include/squigglekit_hip.h).  Plain numpy, no library, no oracle.

Inputs: span_off int64 [P + 1] and spans int32 [E, 2] in the layout of dtw_pairs_paths / dtw_band / map_paths (row e of
pair p covers the target points spans[e, 0] .. spans[e, 1]; a negative first entry: no path), value float64 [E], dwell
int32 [E], target int32 [P] (negative: the pair is left out), shift int32 [P], use [P] (0: left out), tlen int64 [T].
Point j of target t has the flat index toff[t] + j with toff = cumsum(tlen).

A row is USED when target[p] >= 0, use[p] != 0 and spans[e, 0] >= 0; a used row is one entry of every point
spans[e, 0] + shift[p] .. spans[e, 1] + shift[p] of target[p].  A point's list is ordered by ascending row.
"""
import numpy as np

PILE_DTYPE = np.dtype([("level", "<f8"), ("level_sd", "<f8"), ("vmin", "<f8"), ("vmax", "<f8"), ("dwell_mean", "<f8"),
                       ("dwell_sd", "<f8"), ("depth", "<i4"), ("n", "<i4"), ("shared", "<i4"), ("pad", "<i4")])


class Refused(ValueError):
    """The call is refused: `pair` is the lowest offending pair index (None: no pair is to blame), `what` says why."""

    def __init__(self, pair, what):
        super().__init__("%s (pair %s)" % (what, pair))
        self.pair, self.what = pair, what


def _inputs(span_off, spans, value, dwell, target, shift, use, tlen):
    span_off = np.asarray(span_off, dtype=np.int64).reshape(-1)
    P = span_off.size - 1
    spans = np.asarray(spans, dtype=np.int32).reshape(-1, 2)
    E = len(spans)
    value = np.asarray(value, dtype=np.float64).reshape(-1)
    dwell = np.ones(E, dtype=np.int32) if dwell is None else np.asarray(dwell, dtype=np.int32).reshape(-1)
    target = np.zeros(P, dtype=np.int32) if target is None else np.asarray(target, dtype=np.int32).reshape(-1)
    shift = np.zeros(P, dtype=np.int32) if shift is None else np.asarray(shift, dtype=np.int32).reshape(-1)
    use = np.ones(P, dtype=np.uint8) if use is None else (np.asarray(use).reshape(-1) != 0).astype(np.uint8)
    tlen = np.asarray(tlen, dtype=np.int64).reshape(-1)
    assert value.size == E and dwell.size == E and target.size == P and shift.size == P and use.size == P
    return span_off, spans, value, dwell, target, shift, use, tlen, P, E


def check(span_off, spans, value, dwell=None, target=None, shift=None, use=None, tlen=None):
    """Raises Refused for what the library refuses, in the library's order: a negative tlen; then span_off (span_off[0]
    != 0, a decrease, span_off[P] != E -- the lowest pair of these); then, the lowest pair of: target[p] >= T, a used row
    with b < a, a used row whose shifted span leaves [0, tlen[t])."""
    span_off, spans, value, dwell, target, shift, use, tlen, P, E = _inputs(span_off, spans, value, dwell, target, shift,
                                                                           use, tlen)
    if np.any(tlen < 0):
        raise Refused(None, "negative tlen at target %d" % int(np.flatnonzero(tlen < 0)[0]))
    if P == 0 or E == 0:
        return
    bad = []
    if span_off[0] != 0:
        bad.append(0)
    bad += [int(p) for p in np.flatnonzero(np.diff(span_off) < 0)]
    if span_off[P] != E:
        bad.append(P - 1)
    if bad:
        raise Refused(min(bad), "span_off")
    T = tlen.size
    worst = None
    for p in range(P):
        why = None
        if target[p] >= T:
            why = "target"
        elif target[p] >= 0 and use[p]:
            for e in range(span_off[p], span_off[p + 1]):
                a, b = int(spans[e, 0]), int(spans[e, 1])
                if a < 0:
                    continue
                if b < a:
                    why = "order"
                elif a + int(shift[p]) < 0 or b + int(shift[p]) >= tlen[target[p]]:
                    why = "range"
                if why:
                    break
        if why:
            worst = (p, why)
            break
    if worst:
        raise Refused(*worst)


def entries(span_off, spans, target=None, shift=None, use=None, tlen=None):
    """(ent_off int64 [Mtot + 1], ent_row int32): the inverted index of a call that check() passes."""
    E = len(np.asarray(spans).reshape(-1, 2))
    span_off, spans, _, _, target, shift, use, tlen, P, E = _inputs(span_off, spans, np.zeros(E), None, target, shift, use,
                                                                   tlen)
    toff = np.concatenate([[0], np.cumsum(tlen)]).astype(np.int64)
    mtot = int(toff[-1])
    pts, rows = [], []
    if P and E:
        for p in range(P):
            if target[p] < 0 or not use[p]:
                continue
            for e in range(span_off[p], span_off[p + 1]):
                a, b = int(spans[e, 0]), int(spans[e, 1])
                if a < 0:
                    continue
                lo = int(toff[target[p]]) + a + int(shift[p])
                pts.append(np.arange(lo, lo + b - a + 1, dtype=np.int64))
                rows.append(np.full(b - a + 1, e, dtype=np.int64))
    pts = np.concatenate(pts) if pts else np.zeros(0, dtype=np.int64)
    rows = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
    order = np.lexsort((rows, pts))                              # by point, then by ascending row
    ent_off = np.zeros(mtot + 1, dtype=np.int64)
    ent_off[1:] = np.cumsum(np.bincount(pts, minlength=mtot)) if mtot else 0
    return ent_off, rows[order].astype(np.int32)


def pileup_ref(span_off, spans, value, dwell=None, target=None, shift=None, use=None, tlen=None):
    """(pile PILE_DTYPE [Mtot], ent_off, ent_row), or Refused."""
    check(span_off, spans, value, dwell, target, shift, use, tlen)
    span_off, spans, value, dwell, target, shift, use, tlen, P, E = _inputs(span_off, spans, value, dwell, target, shift,
                                                                           use, tlen)
    ent_off, ent_row = entries(span_off, spans, target, shift, use, tlen)
    mtot = ent_off.size - 1
    pile = np.zeros(mtot, dtype=PILE_DTYPE)
    for name in ("level", "level_sd", "vmin", "vmax", "dwell_mean", "dwell_sd"):
        pile[name] = np.nan
    pair_of_row = np.repeat(np.arange(P), np.diff(span_off)) if P and E else np.zeros(0, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for m in np.flatnonzero(np.diff(ent_off) > 0):
            rows = ent_row[ent_off[m]:ent_off[m + 1]]
            v, d = value[rows], dwell[rows]
            n = rows.size
            r = pile[m]
            r["level"], r["level_sd"] = np.mean(v), np.std(v)
            r["vmin"], r["vmax"] = np.min(v), np.max(v)
            r["dwell_mean"] = np.sum(d, dtype=np.int64) / n
            r["dwell_sd"] = np.std(d.astype(np.float64))
            r["depth"] = np.unique(pair_of_row[rows]).size
            r["n"] = n
            r["shared"] = int(np.count_nonzero(spans[rows, 1] > spans[rows, 0]))
    return pile, ent_off, ent_row


def naive_sum(v):
    """Left to right: what a kernel that ignores numpy's pairwise order would compute."""
    s = 0.0
    for x in np.asarray(v, dtype=np.float64):
        s += x
    return s


def format_table(names, strands, targets, pile, tlen):
    """The text squiggle_map.py --pileup writes: a header, then one line per point of every target."""
    cols = "target strand pos ref_z depth events shared level level_sd min max dwell_mean dwell_sd".split()
    lines = ["\t".join(cols)]
    toff = np.concatenate([[0], np.cumsum(tlen)]).astype(np.int64)
    for t in range(len(tlen)):
        for j in range(int(tlen[t])):
            r = pile[toff[t] + j]
            stats = ["."] * 6 if r["n"] == 0 else ["{}".format(float(r[k])) for k in
                                                   ("level", "level_sd", "vmin", "vmax", "dwell_mean", "dwell_sd")]
            lines.append("\t".join([names[t], strands[t], str(j), "{}".format(float(targets[t][j])), str(int(r["depth"])),
                                    str(int(r["n"])), str(int(r["shared"]))] + stats))
    return "\n".join(lines) + "\n"
