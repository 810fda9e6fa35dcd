"""The definition of a filtered HMM session, stated in numpy with carried state (a helper, not a test).

hmmstream_ref.Session carries the Viterbi pass from push to push.  A filtered session carries, beside it, the forward
variables of hmm_post_ref: alpha[S] float64 per slot, -inf after a reset.  A push appends samples t = n, n + 1, .. of a
slot, for either feed, and x is the value the Viterbi step of the same sample sees:
    t == 0:  alpha_j = linit[j] + e_j(x)
    t >= 1:  alpha_j = lse_i(alpha_i + ltrans[i][j]) + e_j(x)
with hmm_post_ref's sk_exp, sk_log, lse and components, operation for operation.  The Viterbi side is hmmstream_ref's,
untouched.  The filter of a slot (FILT_DTYPE, 64 bytes): n == 0: all zero; else L = lse_j alpha_j in rising j,
loglik = L, post[j] = sk_exp((alpha_j + 0.0) - L) for j < S and 0.0 above; L == -inf: loglik -inf, flags IMPOSSIBLE,
every post 0.0.  Since beta(n - 1) = 0.0 in the one-shot statement, this is hmm_post_ref.posterior_rows' loglik and
final_post of the samples the slot has had since its reset.

The slots of a push are advanced together (arrays [m, S]); every slot's arithmetic is the statement above.
"""
import numpy as np

import hmm_post_ref as PR
import hmmstream_ref as HR

STATES = 6
IMPOSSIBLE = PR.IMPOSSIBLE
FILT_DTYPE = np.dtype([("loglik", "<f8"), ("n_used", "<i4"), ("flags", "<i4"), ("post", "<f8", (STATES,))])
NINF = -np.inf


class Session(HR.Session):
    def __init__(self, model, nslots):
        super().__init__(model, nslots)
        self.alpha = np.full((nslots, self.S), NINF)

    def reset(self, slots, cal2=None):
        super().reset(slots, cal2)
        self.alpha[np.asarray(slots, dtype=np.int64)] = NINF

    def push(self, slots, chunks, feed):
        """hmmstream_ref's push (its records are returned), and alpha over the same samples"""
        slots = np.asarray(slots, dtype=np.int64)
        m = slots.size
        lens = np.array([len(c) for c in chunks], dtype=np.int64)
        top = int(lens.max(initial=0))
        X = np.zeros((m, max(top, 1)))
        for i, ch in enumerate(chunks):
            x = np.asarray(ch).astype(np.float64)
            if feed == "i16":
                x = (x + self.cal[slots[i], 0]) * self.cal[slots[i], 1]
            X[i, :len(ch)] = x
        n0 = self.n[slots].copy()
        al = self.alpha[slots].copy()
        if top > 0:
            e, _ = PR.components(self.c, self.mu, self.h, X[:, :top])            # [m, top, S]
            for p in range(top):
                act = lens > p
                with np.errstate(invalid="ignore"):
                    first = self.linit[None, :] + e[:, p]
                    step = PR.lse(al[:, :, None] + self.ltrans[None], axis=1) + e[:, p]
                na = np.where((n0 + p == 0)[:, None], first, step)
                al[act] = na[act]
        rec = super().push(slots, chunks, feed)
        self.alpha[slots] = al
        return rec

    def filter(self, slots):
        slots = np.asarray(slots, dtype=np.int64)
        m, S = slots.size, self.S
        out = np.zeros(m, dtype=FILT_DTYPE)
        if m == 0:
            return out
        al, n = self.alpha[slots], self.n[slots]
        some = n > 0
        L = PR.lse(al, axis=1)
        live = some & (L != NINF)
        Ls = np.where(live, L, 0.0)[:, None]
        with np.errstate(invalid="ignore"):
            g = PR.sk_exp((al + 0.0) - Ls)
        out["n_used"] = n
        out["loglik"] = np.where(some, L, 0.0)
        out["flags"] = np.where(some & ~live, IMPOSSIBLE, 0)
        out["post"][:, :S] = np.where(live[:, None], g, 0.0)
        return out


def empty_filters(m):
    return np.zeros(m, dtype=FILT_DTYPE)


def dead_end_model():
    """three states in a row; nothing leaves the last one, not even to itself: a read is possible for three samples at
    the most (0 -> 0 .., 0 -> 1 -> 2, and then no state has a predecessor)"""
    return {"nstates": 3, "linit": np.array([0.0, NINF, NINF]),
            "ltrans": np.array([[NINF, -0.5, NINF], [NINF, NINF, -0.25], [NINF, NINF, NINF]]),
            "c": np.array([[0.0, NINF], [-1.0, -2.0], [-0.5, NINF]]), "mu": np.array([[1.0, 0.0], [2.0, 3.0], [0.0, 0.0]]),
            "h": np.array([[0.5, 0.0], [0.25, 1.0], [0.125, 0.0]])}


def loop_model():
    """three states in a loop 0 -> 1 -> 2 -> 0 with self transitions, one linit -inf: non-integer scores, every lse has
    two finite terms"""
    lt = np.full((3, 3), NINF)
    for i in range(3):
        lt[i, i], lt[i, (i + 1) % 3] = np.log(0.9), np.log(0.1)
    return {"nstates": 3, "linit": np.array([np.log(0.7), NINF, np.log(0.3)]), "ltrans": lt,
            "c": np.array([[-1.0, -2.5], [-1.5, NINF], [-0.75, -3.0]]), "mu": np.array([[0.0, 2.0], [1.0, 0.0], [3.0, 1.5]]),
            "h": np.array([[0.5, 0.125], [0.3, 0.0], [0.2, 0.7]])}


def run_session(model, sess):
    """what a filtered session must return for the script (hmmstream_ref.draw_session): per "push" op, in order, the pair
    (records hmmstream_ref.DTYPE [m], filters FILT_DTYPE [m] of the same slots after the push)"""
    ref = Session(model, sess["nslots"])
    want = []
    for op in sess["ops"]:
        if op[0] == "reset":
            ref.reset(op[1], op[2])
        else:
            rec = ref.push(op[1], op[2], op[3])
            want.append((rec, ref.filter(op[1])))
    return want


def assert_filters(got, want, slots, label):
    assert got.dtype == FILT_DTYPE and got.shape == want.shape, label
    assert not np.isnan(got["loglik"]).any() and not np.isnan(got["post"]).any(), label
    if got.tobytes() != want.tobytes():
        bad = [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()]
        raise AssertionError("%s: entry %d slot %d (%d entries differ)\n got  %r\n want %r" % (
            label, bad[0], int(slots[bad[0]]), len(bad), got[bad[0]], want[bad[0]]))


def play_session(api, model, sess, label="", want=None):
    """The script on a filtered api.HmmStream and on a plain one: after every push the records of both are
    hmmstream_ref's byte for byte and the filter is the statement's (want: run_session's, if the caller has it).  Returns
    the number of pushes."""
    want = run_session(model, sess) if want is None else want
    lm = HR.lib_model(model)
    j = 0
    with api.HmmStream(lm, sess["nslots"], filter=True) as hf, api.HmmStream(lm, sess["nslots"]) as hp:
        for step, op in enumerate(sess["ops"]):
            if op[0] == "reset":
                hf.reset(op[1], op[2])
                hp.reset(op[1], op[2])
                continue
            _, slots, chunks, feed = op
            tag = "%s op %d (%s)" % (label, step, feed)
            got = hf.push(slots, chunks) if feed == "i16" else hf.push_values(slots, chunks)
            plain = hp.push(slots, chunks) if feed == "i16" else hp.push_values(slots, chunks)
            HR.assert_records(got, want[j][0], slots, tag, sess)
            assert plain.tobytes() == got.tobytes(), tag
            assert_filters(hf.filter(slots), want[j][1], slots, tag)
            j += 1
    return j
