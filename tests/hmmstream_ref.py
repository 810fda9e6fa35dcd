"""The definition of the HMM sessions, stated in numpy with carried state (a helper, not a test).

A session has one model (tests/hmm_ref.py: S, linit, ltrans, c, mu, h) and `nslots` slots.  A slot carries
    v[S] float64, E[S][6] int32, n (samples since its reset), pushes, and its calibration pair (offset, unit)
-- at reset v = -inf, E = -1, n = pushes = 0 and the pair is the one the reset names, (0.0, 1.0) without one.
A push appends a chunk to each named slot.  Its samples are x = (float64(raw) + offset) * unit for an int16 chunk (with
the slot's pair) or the values themselves for a float64 chunk; sample number t = n, n + 1, .. of the slot takes
    t == 0:  v_j = linit[j] + e_j(x),  E_j[j] = 0
    t >= 1:  b_j = max over i in rising i of v_i + ltrans[i][j] (strictly greater replaces), v_j = b_j + e_j(x),
             E_j = the winner's tuple, then E_j[j] = t if it is still -1
with hmm_ref's emission and max.  Nothing else is kept: no sample, no look-ahead.  A chunk of length 0 changes nothing.
The record (DTYPE, 96 bytes) after a push: f = the lowest j with the largest v_j; score = v_f, final_state = f, n_used = n,
enter = E_f; v = the six scores (-inf at and above S); pushes = the pushes of length > 0; flags = 0.  n == 0: score 0.0,
final_state -1, every enter -1, every v -inf.

The slots of a push are advanced together (arrays [m, S]); every slot's arithmetic is the statement above.
"""
import numpy as np

import hmm_ref

STATES = 6
DTYPE = np.dtype([("score", "<f8"), ("final_state", "<i4"), ("n_used", "<i4"), ("enter", "<i4", (STATES,)),
                  ("v", "<f8", (STATES,)), ("pushes", "<i4"), ("flags", "<i4")])
NINF = -np.inf


class Session:
    def __init__(self, model, nslots):
        self.S, self.linit, self.ltrans, self.c, self.mu, self.h = hmm_ref.model_arrays(model)
        self.nslots = nslots
        self.v = np.full((nslots, self.S), NINF)
        self.E = np.full((nslots, self.S, STATES), -1, dtype=np.int32)
        self.n = np.zeros(nslots, dtype=np.int64)
        self.pushes = np.zeros(nslots, dtype=np.int64)
        self.cal = np.tile(np.array([0.0, 1.0]), (nslots, 1))

    def reset(self, slots, cal2=None):
        slots = np.asarray(slots, dtype=np.int64)
        self.v[slots] = NINF
        self.E[slots] = -1
        self.n[slots] = 0
        self.pushes[slots] = 0
        self.cal[slots] = np.array([0.0, 1.0]) if cal2 is None else np.asarray(cal2, dtype=np.float64).reshape(-1, 2)

    def push(self, slots, chunks, feed):
        """feed "i16": integer chunks through the slots' calibration pairs; "f64": float64 values as they are"""
        slots = np.asarray(slots, dtype=np.int64)
        m, S = slots.size, self.S
        lens = np.array([len(c) for c in chunks], dtype=np.int64)
        top = int(lens.max(initial=0))
        X = np.zeros((m, max(top, 1)))
        for i, ch in enumerate(chunks):
            x = np.asarray(ch).astype(np.float64)
            if feed == "i16":
                x = (x + self.cal[slots[i], 0]) * self.cal[slots[i], 1]
            X[i, :len(ch)] = x
        v, E, n0 = self.v[slots].copy(), self.E[slots].copy(), self.n[slots]
        rows, diag = np.arange(m), np.arange(S)
        for p in range(top):
            act = lens > p
            t = n0 + p
            e = hmm_ref.emission(self.c, self.mu, self.h, X[:, p])
            # t == 0
            fv = self.linit[None, :] + e
            fE = E.copy()
            fE[:, diag, diag] = 0
            # t >= 1
            with np.errstate(invalid="ignore"):
                cand = v[:, :, None] + self.ltrans[None, :, :]      # [m, from, to]
            b = cand[:, 0, :].copy()
            arg = np.zeros((m, S), dtype=np.int64)
            for i in range(1, S):
                w = cand[:, i, :] > b
                b = np.where(w, cand[:, i, :], b)
                arg = np.where(w, i, arg)
            NE = E[rows[:, None], arg]
            for j in range(S):
                NE[:, j, j] = np.where(NE[:, j, j] < 0, t, NE[:, j, j])
            with np.errstate(invalid="ignore"):
                nv = b + e
            first = t == 0
            nv = np.where(first[:, None], fv, nv)
            NE = np.where(first[:, None, None], fE, NE)
            v[act] = nv[act]
            E[act] = NE[act]
        self.v[slots], self.E[slots] = v, E
        self.n[slots] += lens
        self.pushes[slots] += lens > 0
        return self.records(slots)

    def records(self, slots):
        slots = np.asarray(slots, dtype=np.int64)
        m, S = slots.size, self.S
        rec = np.zeros(m, dtype=DTYPE)
        rec["final_state"], rec["enter"], rec["v"] = -1, -1, NINF
        v, E, n = self.v[slots], self.E[slots], self.n[slots]
        best = v[:, 0].copy()
        f = np.zeros(m, dtype=np.int64)
        for j in range(1, S):
            w = v[:, j] > best
            best = np.where(w, v[:, j], best)
            f = np.where(w, j, f)
        ok = n > 0
        rec["score"][ok] = best[ok]
        rec["final_state"][ok] = f[ok]
        rec["enter"][ok] = E[np.arange(m), f][ok]
        rec["n_used"] = n
        rec["v"][:, :S] = v
        rec["pushes"] = self.pushes[slots]
        return rec


def empty_records(m):
    rec = np.zeros(m, dtype=DTYPE)
    rec["final_state"], rec["enter"], rec["v"] = -1, -1, NINF
    return rec


# ---- models and reads ------------------------------------------------------------------------------------------------
def tie_model(rng, S=None):
    """integer ltrans, c, mu and h = 0 or small integers: with integer samples every score is an exact integer and ties
    are everywhere; random -inf transitions (dead states, unreachable states) and absent second components"""
    S = int(rng.integers(1, 7)) if S is None else S
    linit = rng.integers(-3, 1, S).astype(np.float64)
    linit[rng.random(S) < 0.3] = NINF
    if not np.isfinite(linit).any():
        linit[int(rng.integers(0, S))] = 0.0
    ltrans = rng.integers(-3, 1, (S, S)).astype(np.float64)
    ltrans[rng.random((S, S)) < 0.4] = NINF
    c = rng.integers(-2, 1, (S, 2)).astype(np.float64)
    c[rng.random(S) < 0.5, 1] = NINF
    mu = rng.integers(0, 4, (S, 2)).astype(np.float64)
    h = rng.integers(0, 3, (S, 2)).astype(np.float64)
    return {"nstates": S, "linit": linit, "ltrans": ltrans, "c": c, "mu": mu, "h": h}


def lib_model(model):
    """the _lib.HmmModel of a dict model (an HmmModel is returned as it is)"""
    from squigglekit_amd import _lib
    if hasattr(model, "arrays"):
        return model
    return _lib.HmmModel.from_arrays(model["nstates"], model["linit"], model["ltrans"], model["c"], model["mu"], model["h"])


def small_drna_read(rng, n=1500):
    """a synth.drna_reads-like read shrunk to about n samples, in the synth_raw preset's units: a stretch of open pore,
    leader, adapter N(430, 25), poly(A) N(560, 8) with one cliff, then a body of event levels -- every state is visited"""
    parts = [rng.normal(900, 60, n // 25), rng.normal(500, 60, n // 15), rng.normal(430, 25, n // 4),
             rng.normal(560, 8, n // 10), rng.normal(480, 20, 6), rng.normal(560, 8, n // 10)]
    left = n - sum(len(p) for p in parts)
    levels = rng.normal(530, 80, left // 8 + 1)
    parts.append(np.repeat(levels, 8)[:left] + rng.normal(0, 6, left))
    return np.clip(np.rint(np.concatenate(parts)), -32768, 32767).astype(np.int16)


# ---- session scripts -------------------------------------------------------------------------------------------------
def draw_session(rng, nslots, budget, maxlen, draw_chunk, cal_prob=0.5):
    """A script: {"nslots", "ops"}; ops are ("push", slots int32 [m], chunks, feed) -- chunks int16 arrays for feed "i16",
    float64 arrays for "f64" -- and ("reset", slots, cal2 or None).  Pushes name shuffled subsets; a chunk is empty (a
    peek) about one time in six; resets come in mid-read, half of them with calibration pairs."""
    ops, used = [], 0
    subset = lambda: int(rng.integers(1, nslots + 1)) if rng.random() < 0.7 else nslots   # noqa: E731
    while used < budget:
        if rng.random() < 0.12:
            slots = rng.permutation(nslots)[:subset()].astype(np.int32)
            cal2 = None
            if rng.random() < cal_prob:
                cal2 = np.stack([rng.integers(-8, 9, slots.size).astype(np.float64),
                                 rng.choice([0.5, 1.0, 0.1825, 2.0], slots.size)], axis=1)
            ops.append(("reset", slots, cal2))
            continue
        slots = rng.permutation(nslots)[:subset()].astype(np.int32)
        feed = "i16" if rng.random() < 0.6 else "f64"
        chunks = []
        for _ in slots:
            u = rng.random()
            n = 0 if u < 0.15 else (1 if u < 0.25 else int(rng.integers(0, maxlen + 1)))
            n = min(n, max(budget - used, 0) + 1)
            ch = draw_chunk(rng, n)
            chunks.append(ch if feed == "i16" else ch.astype(np.float64))
            used += n
        ops.append(("push", slots, chunks, feed))
        used += 1
    ops.append(("push", np.arange(nslots, dtype=np.int32), [np.zeros(0, dtype=np.int16)] * nslots, "i16"))   # a peek at all
    return {"nslots": nslots, "ops": ops}


def run_session(model, sess):
    """what every push of the script must return: one DTYPE [m] array per "push" op, in order"""
    ref = Session(model, sess["nslots"])
    want = []
    for op in sess["ops"]:
        if op[0] == "reset":
            ref.reset(op[1], op[2])
        else:
            want.append(ref.push(op[1], op[2], op[3]))
    return want


def assert_records(got, want, slots, label, sess=None):
    assert got.dtype == DTYPE and got.shape == want.shape, label
    if got.tobytes() != want.tobytes():
        bad = [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()]
        raise AssertionError("%s: entry %d slot %d (%d entries differ)\n got  %r\n want %r\n%s" % (
            label, bad[0], int(slots[bad[0]]), len(bad), got[bad[0]], want[bad[0]], describe_session(sess) if sess else ""))


def iter_session(hs, model, sess, label=""):
    """Run the script on the api.HmmStream hs, one op per step of the generator: every push's records equal
    run_session's byte for byte."""
    want = run_session(model, sess)
    j = 0
    for step, op in enumerate(sess["ops"]):
        if op[0] == "reset":
            hs.reset(op[1], op[2])
        else:
            _, slots, chunks, feed = op
            got = hs.push(slots, chunks) if feed == "i16" else hs.push_values(slots, chunks)
            assert_records(got, want[j], slots, "%s op %d (%s)" % (label, step, feed), sess)
            j += 1
        yield step


def play_session(api, model, sess, label=""):
    """iter_session to its end on a session of its own; returns the number of pushes."""
    with api.HmmStream(lib_model(model), sess["nslots"]) as hs:
        for _ in iter_session(hs, model, sess, label):
            pass
    return sum(op[0] == "push" for op in sess["ops"])


def describe_session(sess):
    """one line per op: what to look at when a seed fails"""
    lines = ["%d slots, %d ops" % (sess["nslots"], len(sess["ops"]))]
    for j, op in enumerate(sess["ops"]):
        if op[0] == "reset":
            lines.append("%3d reset %s%s" % (j, list(map(int, op[1]))[:12], "" if op[2] is None else " cal"))
        else:
            _, slots, chunks, feed = op
            lines.append("%3d push %s %s" % (j, feed, " ".join("%d:%d" % (int(s), len(c)) for s, c in list(zip(slots, chunks))[:12])
                                             + (" ..." if len(slots) > 12 else "")))
    return "\n".join(lines[:60])
