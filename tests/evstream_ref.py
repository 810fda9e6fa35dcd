"""The event-session contract in numpy and plain Python, on top of detect_ref (a helper, not a test).

A session has `nslots` slots and one parameter set.  A slot holds a read in progress: the samples it has been given since
its reset.  A push appends a chunk and walks the slot's positions i while i + w_long <= n: for those both t_short[i] and
t_long[i] are what they will be in the finished read.  Every mark closes the event [last boundary, pos) and emits its
record (start, length, sum, sumsq) in read coordinates.  END walks the rest under detect_ref's rule and emits the closing
event [last boundary, n).  So:

    emitted(x, params, ended=False)   the records a slot has emitted after the samples x: the events closed by the marks
                                      that detect_ref's walk makes at steps i < max(0, len(x) - w_long + 1);
    emitted(x, params, ended=True)    detect_ref.events(x).

Two facts carry the kernel (tests/test_evstream_host.py checks them): marks_with_steps() returns strictly rising positions
across both detectors together, so an event is final the moment its end is marked; and consecutive marks lie at least
w_short // 2 + 1 apart, which bounds what a push can emit.

run_session() plays a whole script with ONE walk per read (the marks of all its samples with the steps that made them;
a prefix's emission is a count of those) -- the same arrays as emitted() on every prefix, which the host test checks.
"""
import numpy as np

import detect_ref

DTYPE = detect_ref.DTYPE
KINDS = ("steps", "ties", "walk", "clean")


def marks_with_steps(x, params, steps=None):
    """[(pos, step)]: detect_ref.marks' walk over steps i < `steps` (default: all of them), with the step that made
    each mark.  The positions alone, for steps = len(x), are detect_ref.marks(x, params)."""
    w_short, w_long, th_short, th_long, h = params
    n = len(x)
    steps = n if steps is None else min(int(steps), n)
    ws = (int(w_short), int(w_long))
    th = (float(th_short), float(th_long))
    t = (detect_ref.tstat(x, ws[0]).tolist(), detect_ref.tstat(x, ws[1]).tolist())
    pos = [-1, -1]
    val = [np.inf, np.inf]
    valid = [False, False]
    masked_to = [-1, -1]
    out = []
    for i in range(steps):
        for k in (0, 1):
            if i <= masked_to[k]:
                continue
            cur = t[k][i]
            if pos[k] == -1:
                if cur < val[k]:
                    val[k] = cur
                elif cur - val[k] > h:
                    val[k] = cur
                    pos[k] = i
            else:
                if cur > val[k]:
                    val[k] = cur
                    pos[k] = i
                if k == 0 and val[0] > th[0]:
                    masked_to[1] = pos[0] + ws[0]
                    pos[1] = -1
                    val[1] = np.inf
                    valid[1] = False
                if val[k] - cur > h and val[k] > th[k]:
                    valid[k] = True
                if valid[k] and i - pos[k] > ws[k] // 2:
                    out.append((pos[k], i))
                    pos[k] = -1
                    val[k] = cur
                    valid[k] = False
    return out


def walked(n, params):
    """positions walked of a slot that holds n samples and has not ended"""
    return max(0, int(n) - int(params[1]) + 1)


def records_of(x, bounds):
    """the records of the events between consecutive boundaries"""
    x = np.asarray(x).astype(np.int64)
    c1 = np.concatenate(([0], np.cumsum(x)))
    c2 = np.concatenate(([0], np.cumsum(x * x)))
    rec = np.zeros(max(len(bounds) - 1, 0), dtype=DTYPE)
    for k in range(len(bounds) - 1):
        a, b = bounds[k], bounds[k + 1]
        rec[k] = (a, b - a, int(c1[b] - c1[a]), int(c2[b] - c2[a]))
    return rec


def emitted(x, params, ended=False):
    """The statement: everything a slot has emitted after the samples x."""
    x = np.asarray(x)
    if ended:
        return detect_ref.events(x, params)
    ms = marks_with_steps(x, params, walked(len(x), params))
    return records_of(x, [0] + [p for p, _ in ms])


# ---- random reads and sessions ----------------------------------------------------------------------------------------
def draw_read(rng, n, kind):
    """n int16 samples of one of the four kinds: level steps plus noise, tie-heavy small integers, a random walk,
    noise-free steps"""
    n = int(n)
    if n == 0:
        return np.zeros(0, dtype=np.int16)
    if kind == "ties":
        return rng.integers(-1, 2, size=n).astype(np.int16)
    if kind == "walk":
        return np.clip(np.cumsum(rng.integers(-40, 41, size=n)), -30000, 30000).astype(np.int16)
    dwell = rng.integers(2, 40, size=n // 2 + 1)
    level = rng.integers(-600, 600, size=dwell.size)
    x = np.repeat(level, dwell)[:n].astype(np.float64)
    if kind == "steps":
        x = x + rng.normal(0.0, float(rng.choice([2.0, 15.0, 60.0])), size=n)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def draw_params(rng):
    """dna, rna, or random parameters (w_short 1 .. 19, w_long up to 39, peak_height 0 .. 1), the corners now and then"""
    c = int(rng.integers(0, 8))
    if c == 0:
        return detect_ref.PRESETS["dna"]
    if c == 1:
        return detect_ref.PRESETS["rna"]
    if c == 2:
        return (1, int(rng.integers(1, 5)), 1.0, 4.0, 0.0)
    if c == 3:
        return (64, 64, 2.0, 3.0, 0.1)
    ws = int(rng.integers(1, 20))
    wl = int(rng.integers(ws, 40))
    return (ws, wl, float(np.round(rng.uniform(0.5, 4.0), 3)), float(np.round(rng.uniform(2.0, 10.0), 3)),
            float(np.round(rng.uniform(0.0, 1.0), 3)))


def draw_session(rng, nslots=None, budget=12000, maxlen=None):
    """{"params", "nslots", "ops"}: ops are ("push", slots, chunks, end) and ("reset", slots).  Pushes name shuffled
    subsets; a slot is fresh, continuing, ending or given an empty chunk; an ended slot gets empty chunks only until a
    reset revives it.  About `budget` samples in all."""
    params = draw_params(rng)
    nslots = int(rng.choice([1, 3, 64, 70, 130])) if nslots is None else int(nslots)
    kinds = [KINDS[int(rng.integers(0, 4))] for _ in range(nslots)]
    ended = [False] * nslots
    ops, used = [], 0
    if maxlen is None:
        maxlen = int(rng.choice([5, 70, 300, 700] if nslots <= 16 else [5, 40, 150, 300]))

    def subset():                                                    # most of the slots, or a few
        return int(rng.integers(1, nslots + 1)) if rng.random() < 0.5 else int(rng.integers(1, min(nslots, 8) + 1))

    while used < budget:
        if rng.random() < 0.12:
            slots = rng.permutation(nslots)[:subset()].astype(np.int32)
            ops.append(("reset", slots))
            for s in slots:
                ended[s] = False
                kinds[s] = KINDS[int(rng.integers(0, 4))]
            continue
        k = subset()
        slots = rng.permutation(nslots)[:k].astype(np.int32)
        chunks, end = [], []
        for s in slots:
            u = rng.random()
            n = 0 if (ended[s] or u < 0.15) else (1 if u < 0.25 else int(rng.integers(0, maxlen + 1)))
            n = min(n, max(budget - used, 0) + 1)
            chunks.append(draw_read(rng, n, kinds[s]))
            used += n
            e = bool(rng.random() < 0.15)
            end.append(e)
            if e:
                ended[s] = True
        ops.append(("push", slots, chunks, np.array(end, dtype=np.int32)))
        used += 1
    ops.append(("push", np.arange(nslots, dtype=np.int32), [np.zeros(0, dtype=np.int16)] * nslots,
                np.ones(nslots, dtype=np.int32)))
    return {"params": params, "nslots": nslots, "ops": ops}


def run_session(sess):
    """What every push of the script must return: a list with one (off int64 [m + 1], rec) per "push" op, in order.
    One walk per read: the marks of all the samples a slot gets between two resets, with their steps."""
    params, nslots, ops = sess["params"], sess["nslots"], sess["ops"]
    # pass 1: every read's samples (a read: what a slot is given between resets; samples stop counting at its END)
    reads = [[{"chunks": [], "ended": False}] for _ in range(nslots)]
    for op in ops:
        if op[0] == "reset":
            for s in op[1]:
                reads[s].append({"chunks": [], "ended": False})
            continue
        _, slots, chunks, end = op
        for s, c, e in zip(slots, chunks, end):
            r = reads[s][-1]
            if r["ended"]:
                assert len(c) == 0, "the script gives samples to an ended slot"
                continue
            r["chunks"].append(np.asarray(c, dtype=np.int16))
            if e:
                r["ended"] = True
    for per_slot in reads:
        for r in per_slot:
            x = np.concatenate(r["chunks"]) if r["chunks"] else np.zeros(0, dtype=np.int16)
            ms = marks_with_steps(x, params, None if r["ended"] else walked(len(x), params))
            r["x"], r["steps"] = x, [st for _, st in ms]
            r["rec"] = detect_ref.events(x, params) if r["ended"] else records_of(x, [0] + [p for p, _ in ms])
            r["n"], r["out"], r["done"] = 0, 0, False
    # pass 2: the counts after every push
    at = [0] * nslots
    want = []
    for op in ops:
        if op[0] == "reset":
            for s in op[1]:
                at[s] += 1
            continue
        _, slots, chunks, end = op
        parts = []
        for s, c, e in zip(slots, chunks, end):
            r = reads[s][at[s]]
            if r["done"]:
                parts.append(r["rec"][:0])
                continue
            r["n"] += len(c)
            if e:
                r["done"] = True
                cnt = len(r["rec"])
            else:
                lim = walked(r["n"], params)
                cnt = int(np.searchsorted(np.asarray(r["steps"], dtype=np.int64), lim, side="left"))
            parts.append(r["rec"][r["out"]:cnt])
            r["out"] = cnt
        off = np.zeros(len(slots) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(p) for p in parts])
        want.append((off, np.concatenate(parts) if parts else np.zeros(0, dtype=DTYPE)))
    return want


def play_session(api, sess, label=""):
    """Run the script on an api.EventStream: every push's (off, rec) equal run_session's byte for byte, every ended
    read's concatenation equal the one-shot api.detect_events on its samples, and no guard hit."""
    from squigglekit_amd import _lib
    params = _lib.DetParams(*sess["params"])
    want = run_session(sess)
    nslots = sess["nslots"]
    had = [[[], []] for _ in range(nslots)]                          # per slot: chunks, records since its reset
    closed = [False] * nslots
    finished = []
    j = 0
    with api.EventStream(params, nslots) as es:
        for step, op in enumerate(sess["ops"]):
            if op[0] == "reset":
                es.reset(op[1])
                for s in op[1]:
                    had[s], closed[s] = [[], []], False
                continue
            _, slots, chunks, end = op
            off, rec = es.push(slots, chunks, end=end)
            w_off, w_rec = want[j]
            j += 1
            assert rec.dtype == DTYPE
            assert np.array_equal(off, w_off) and rec.tobytes() == w_rec.tobytes(), \
                "%s op %d: off %s, want %s\n%s" % (label, step, off[:12], w_off[:12], describe_session(sess))
            for i, (s, c, e) in enumerate(zip(slots, chunks, end)):
                if closed[s]:
                    continue
                had[s][0].append(np.asarray(c, dtype=np.int16))
                had[s][1].append(rec[off[i]:off[i + 1]])
                if e:
                    closed[s] = True
                    finished.append((np.concatenate(had[s][0]), np.concatenate(had[s][1])))
        guard = api.last_event_plan()["guard_hits"]
    assert guard == 0, "%s: guard_hits = %d" % (label, guard)
    if finished:
        off, rec = api.detect_events([x for x, _ in finished], params)
        for k, (x, got) in enumerate(finished):
            assert got.tobytes() == rec[off[k]:off[k + 1]].tobytes(), \
                "%s: read %d of %d samples differs from the one-shot call\n%s" % (label, k, len(x), describe_session(sess))
    return len(finished)


def describe_session(sess):
    """one line per op: what to look at when a seed fails"""
    lines = ["params %r, %d slots, %d ops" % (tuple(sess["params"]), sess["nslots"], len(sess["ops"]))]
    for j, op in enumerate(sess["ops"]):
        if op[0] == "reset":
            lines.append("%3d reset %s" % (j, list(map(int, op[1]))[:12]))
        else:
            _, slots, chunks, end = op
            lines.append("%3d push  %s" % (j, " ".join("%d:%d%s" % (int(s), len(c), "E" if e else "")
                                                      for s, c, e in list(zip(slots, chunks, end))[:12])
                                          + (" ..." if len(slots) > 12 else "")))
    return "\n".join(lines[:60])
