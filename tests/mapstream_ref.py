"""The statement of a mapping session (include/squigglekit_hip.h, "Mapping sessions") in plain Python, and the helpers
the mapping-session tests share.  Nothing here calls the library.

chained_rows sweeps the rows of one chunk over a target and carries the LAST ROW -- (D, S) per target column -- from
chunk to chunk: a fresh sweep starts under the virtual row -1 (D = 0; the corner (-1, -1) is 0 as well), a continuing one
under the stored row (no corner: the diagonal of column 0 is +inf).  Every cell is c + min in the tie order of the
back-trace (diagonal, then left, then up: up only if strictly smaller, left only if strictly smaller than the diagonal).
The record is the first argmin of the current last row; nothing else is carried."""
import numpy as np

MAPREC = np.dtype([("dist", "<f8"), ("start", "<i4"), ("end", "<i4"), ("n", "<i4"), ("flags", "<i4"), ("rows", "<i4"),
                   ("pushes", "<i4")])
INF = float("inf")


def chained_rows(chunk, y, state=None):
    """(D, S) of the last row after the rows of `chunk`, continuing from `state` (None: fresh)"""
    y = [float(v) for v in y]
    M = len(y)
    if state is None:
        upD, upS, corner = [0.0] * M, [j + 1 for j in range(M)], (0.0, 0)
    else:
        upD, upS, corner = list(state[0]), list(state[1]), (INF, -1)
    for xi in chunk:
        xi = float(xi)
        nD, nS = [0.0] * M, [0] * M
        for j in range(M):
            c = abs(xi - y[j])
            lfD, lfS = (nD[j - 1], nS[j - 1]) if j else (INF, -1)
            dgD, dgS = (upD[j - 1], upS[j - 1]) if j else corner
            m, s = (lfD, lfS) if lfD < dgD else (dgD, dgS)
            if upD[j] < m:
                m, s = upD[j], upS[j]
            nD[j], nS[j] = c + m, s
        upD, upS, corner = nD, nS, (INF, -1)
    return upD, upS


def record_of(state):
    """(dist, start, end): the first argmin of the last row"""
    D, S = state
    j = min(range(len(D)), key=lambda k: (D[k], k))
    return D[j], S[j], j


def chained_record(chunks, y):
    """the record after the chunks, the last row carried between them"""
    state = None
    for ch in chunks:
        if len(ch):
            state = chained_rows(ch, y, state)
    return record_of(state)


def splits_of(N):
    """the cuts of a query of N points the tests use: 1 | N-1, N-1 | 1, thirds, all ones"""
    third = max(1, N // 3)
    return {"1|N-1": [1, N - 1], "N-1|1": [N - 1, 1], "thirds": [third, third, N - 2 * third], "ones": [1] * N}


def cut(x, lens):
    out, a = [], 0
    for n in lens:
        out.append(x[a:a + n])
        a += n
    assert a == len(x)
    return out


class Shadow:
    """What a session's slots have been given, and the oracle's record of it: the reference of every GPU test.  Oracle
    records are cached per (slot content, target), so a peek costs nothing."""

    def __init__(self, ora, targets, nslots):
        self.ora, self.targets = ora, [np.asarray(t, dtype=np.float64) for t in targets]
        self.pts = [np.zeros(0) for _ in range(nslots)]
        self.pushes = [0] * nslots
        self.cache = {}

    def reset(self, slots):
        for s in slots:
            self.pts[s], self.pushes[s] = np.zeros(0), 0
            self.cache = {k: v for k, v in self.cache.items() if k[0] != s}

    def push(self, slots, chunks):
        """append, and the records MAPREC [T, m] the session must return"""
        for s, ch in zip(slots, chunks):
            ch = np.asarray(ch, dtype=np.float64)
            if ch.size:
                self.pts[s] = np.concatenate([self.pts[s], ch])
                self.pushes[s] += 1
                self.cache = {k: v for k, v in self.cache.items() if k[0] != s}
        out = np.zeros((len(self.targets), len(slots)), dtype=MAPREC)
        for i, s in enumerate(slots):
            for t, y in enumerate(self.targets):
                if self.pts[s].size == 0:
                    out[t, i] = (np.nan, -1, -1, y.size, 0, 0, 0)
                    continue
                if (s, t) not in self.cache:
                    self.cache[(s, t)] = self.ora.dtw_subsequence(self.pts[s], y)
                d, a, e = self.cache[(s, t)]
                out[t, i] = (d, a, e, y.size, 0, self.pts[s].size, self.pushes[s])
        return out


def first_difference(got, want):
    """None, or a text naming the first record that differs (bits of dist; two NaNs agree)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "shape %s != %s" % (got.shape, want.shape)
    gd, wd = got["dist"], want["dist"]
    ok = (gd.view(np.uint64) == wd.view(np.uint64)) | (np.isnan(gd) & np.isnan(wd))
    for f in got.dtype.names:
        if f != "dist":
            ok &= got[f] == want[f]
    if ok.all():
        return None
    idx = tuple(int(v) for v in np.argwhere(~ok)[0])
    return "record %s: got %s, want %s" % (idx, got[idx], want[idx])


# ---- drawn sessions: the seeded random tests and tools/fuzz_gpu.py ---------------------------------------------------
CHUNKS = (0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 255, 256, 257, 700, 1023, 1024, 1025, 2100)
TARGETS = (1, 2, 3, 16, 17, 63, 64, 65, 200, 513, 1025, 1500, 3000)
CELLS = 60_000_000                   # oracle cells per drawn session (about 0.4 s of the oracle on one core)


def draw_session(rng):
    """a drawn session as plain data: targets, nslots and a script of ("push", slots, chunks) / ("reset", slots) steps
    (a chunk of length 0 is a peek); normal draws or tie-heavy integers per target and per slot"""
    T = int(rng.integers(1, 5))
    targets = [rng.integers(-3, 4, size=M).astype(np.float64) if rng.random() < 0.5 else rng.normal(size=M)
               for M in (int(rng.choice(TARGETS)) if rng.random() < 0.6 else int(rng.integers(1, 800)) for _ in range(T))]
    nslots = int(rng.choice([1, 2, 3, 4, 5, 9, 17, 40]))
    ties = rng.random(nslots) < 0.5
    sumM = sum(len(t) for t in targets)
    rows = np.zeros(nslots, dtype=np.int64)
    steps, cells = [], 0
    for _ in range(int(rng.integers(3, 12))):
        if rng.random() < 0.15 and steps:
            slots = [int(s) for s in rng.permutation(nslots)[:int(rng.integers(1, nslots + 1))]]
            steps.append(("reset", slots))
            rows[slots] = 0
            continue
        slots = [int(s) for s in rng.permutation(nslots)[:int(rng.integers(1, nslots + 1))]]
        small = rng.random() < 0.5                                       # one shape group, or every group at once
        chunks = []
        for s in slots:
            n = int(rng.choice(CHUNKS[:9])) if small else int(rng.choice(CHUNKS))
            if cells + (rows[s] + n) * sumM > CELLS:                     # (the oracle sweeps the whole concatenation)
                n = 0
            chunks.append(rng.integers(-3, 4, size=n).astype(np.float64) if ties[s] else rng.normal(size=n))
            if n:
                rows[s] += n
                cells += int(rows[s]) * sumM
        steps.append(("push", slots, chunks))
    return {"targets": targets, "nslots": nslots, "steps": steps}


def describe_session(case):
    return "targets %s, %d slots, steps %s" % (
        [len(t) for t in case["targets"]], case["nslots"],
        [(st[0], st[1]) + (([len(c) for c in st[2]],) if st[0] == "push" else ()) for st in case["steps"]])


def run_session(api, ora, case):
    """the drawn session through api.MapStream against the oracle on every slot's concatenation, after every push.
    None, or a text naming the step and the first record that differs"""
    sh = Shadow(ora, case["targets"], case["nslots"])
    with api.MapStream(case["targets"], case["nslots"]) as ms:
        for k, st in enumerate(case["steps"]):
            if st[0] == "reset":
                ms.reset(st[1])
                sh.reset(st[1])
                continue
            diff = first_difference(ms.push(st[1], st[2]), sh.push(st[1], st[2]))
            if diff is not None:
                return "step %d (slots %s, chunks %s): %s" % (k, st[1], [len(c) for c in st[2]], diff)
        every = list(range(case["nslots"]))
        diff = first_difference(ms.peek(every), sh.push(every, [np.zeros(0)] * len(every)))
        if diff is not None:
            return "closing peek: %s" % diff
    return None
