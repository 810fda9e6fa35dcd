"""The MotifSeq session contract in numpy (include/squigglekit_hip.h, "MotifSeq sessions"): what a slot's record must be
after any sequence of pushes, as a function of the samples pushed so far alone.

record()  the statement: numpy statistics + the oracle's dtw_subsequence on the whole prefix.
Resume    the same search continued column by column from the last column (D, S) and the running minimum -- the state a
          session keeps; tests/test_stream_host.py checks it against record() on random cuts.
"""
import numpy as np

EMPTY, DEGENERATE, CALIBRATING = 1, 2, 8
NAN = float("nan")
FIELDS = ("dist", "tail", "start", "end", "n", "seen", "flags")


def keep(raw, lo, hi):
    raw = np.asarray(raw, dtype=np.int16)
    return raw[(raw > lo) & (raw < hi)]


def statistics(x, mode):
    """(center, scale, degenerate) of the kept samples x (int16, at least one) as the one-shot path takes them."""
    x = np.asarray(x).astype(np.float64)
    if mode == "medmad":
        med = np.median(x)
        mad = np.median(np.abs(x - med))
        return float(med), float(mad * 1.4826), bool(mad == 0.0)
    sd = float(np.std(x))
    return float(np.mean(x)), (1.0 if sd == 0.0 else sd), False


def normalisation(raw, W, mode, lo, hi, flushed, given=None):
    """(center, scale, flags) the slot searches under after `raw`, or (None, None, flags) while / where it has none.
    flushed: False, True (flushed now, after all of raw) or the number of raw samples pushed when the flush came.
    A calibration that a flush ended on a MAD of 0 has flags DEGENERATE and center = +inf instead of None: record()
    then gives the one-shot call's distance for such a read, +inf, where a degenerate slot otherwise says NaN."""
    kept = keep(raw, lo, hi)
    n = kept.size
    at = len(raw) if flushed is True else (None if flushed is False else int(flushed))
    if given is not None:
        return float(given[0]), float(given[1]), (EMPTY if (at is not None and n == 0) else 0)
    if n >= W and (at is None or keep(raw[:at], lo, hi).size >= W):
        used = kept[:W]
    elif at is None:
        return None, None, CALIBRATING
    else:
        n_at = keep(raw[:at], lo, hi).size
        if n_at == 0:
            return None, None, EMPTY
        used = kept[:min(n_at, W)]
        if n_at < W and statistics(used, mode)[2]:
            return np.inf, None, DEGENERATE
    c, s, deg = statistics(used, mode)
    return (None, None, DEGENERATE) if deg else (c, s, 0)


def record(raw_prefix, motif, W, mode, lo, hi, flushed, given=None):
    """The record of one motif after the samples `raw_prefix`: (dist, tail, start, end, n, seen, flags)."""
    from oracle import oracle
    raw = np.asarray(raw_prefix, dtype=np.int16)
    kept = keep(raw, lo, hi)
    n, seen = int(kept.size), int(raw.size)
    c, s, flags = normalisation(raw, W, mode, lo, hi, flushed, given)
    if s is None or n == 0:
        return (np.inf if c is not None and s is None else NAN, NAN, -1, -1, n, seen, flags)
    y = (kept.astype(np.float64) - c) / s
    dist, start, end, cost = oracle.dtw_subsequence(np.asarray(motif, dtype=np.float64), y, want_cost=True)
    return (float(dist), float(cost[-1, -1]), int(start), int(end), n, seen, flags)


class Resume:
    """dtw_subsequence(x, y) continued: push() takes the next normalised samples, the state is the last column."""

    def __init__(self, x):
        self.x = np.asarray(x, dtype=np.float64)
        N = self.x.size
        self.D = np.full(N, np.inf)
        self.S = np.full(N, -1, dtype=np.int64)
        self.best, self.bestS, self.bestJ, self.ncols = np.inf, -1, -1, 0

    def push(self, y):
        x, N = self.x, self.x.size
        for yj in np.asarray(y, dtype=np.float64):
            j = self.ncols
            cost = np.abs(x - yj)
            pD, pS = self.D, self.S
            D, S = np.empty(N), np.empty(N, dtype=np.int64)
            D[0], S[0] = cost[0], j                          # free start: row -1 is (0, j)
            for i in range(1, N):
                if j == 0:
                    m, s = D[i - 1], S[i - 1]                # column 0 has only its "up" neighbour
                else:
                    m, s = pD[i - 1], pS[i - 1]              # diagonal first,
                    if pD[i] < m:
                        m, s = pD[i], pS[i]                  # then j - 1,
                    if D[i - 1] < m:
                        m, s = D[i - 1], S[i - 1]            # then i - 1
                D[i], S[i] = cost[i] + m, s
            self.D, self.S = D, S
            if D[-1] < self.best:
                self.best, self.bestS, self.bestJ = D[-1], int(S[-1]), j
            self.ncols += 1
        return self

    def record(self):
        """(dist, tail, start, end) -- NaN / -1 before the first column"""
        if self.ncols == 0:
            return (NAN, NAN, -1, -1)
        return (float(self.best), float(self.D[-1]), self.bestS, self.bestJ)


def same(a, b):
    """two records (or field tuples) equal, NaN == NaN, doubles bit for bit"""
    if len(a) != len(b):
        return False
    for u, v in zip(a, b):
        if isinstance(u, float) or isinstance(v, float):
            if not (np.float64(u).tobytes() == np.float64(v).tobytes() or (u != u and v != v)):
                return False
        elif int(u) != int(v):
            return False
    return True


def fields(rec):
    """a STREAM_DTYPE scalar as the tuple record() returns"""
    return (float(rec["dist"]), float(rec["tail"]), int(rec["start"]), int(rec["end"]), int(rec["n"]), int(rec["seen"]),
            int(rec["flags"]))
