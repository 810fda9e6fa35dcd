"""The fixed scripts of the session tests that reach past the Python wrapper's corner (a helper, not a test): pushes of
thousands of entries, rows as a C caller lays them out, and the device-form contracts of include/squigglekit_hip.h.
tests/test_session_cases.py asserts, from the statement modules alone, that the scripts hold what the GPU tests rely on;
tests/RANDOM_CASES_SESSIONS.md describes them.  Nothing here calls the library.

Scripts come in the families' own forms: evstream_ref's {"params", "nslots", "ops"}, hmmstream_ref's {"nslots", "ops"}
and mapstream_ref's {"targets", "nslots", "steps"}.  Every builder is seeded and cached: a script is drawn once per
process and never changed by its users."""
import numpy as np

import detect_ref
import evstream_ref as ER

DNA = detect_ref.PRESETS["dna"]
SEAM = 4096                          # SCAN_THREADS * SCAN_ITEMS of sk_pull.hip: entry 4 096 opens the scan's second block
MANY_SLOTS = 4200
BIG = (4095, 4096, 4097)
LONG_FROM = 4030                     # entries LONG_FROM .. m - 1 of a big push carry long chunks
LIVE_CALIB = 5
LIVE_RULE = (3, 1.5, 0.02, 12)       # (min_rows, max_dist_per_row, min_margin, give_up_rows): every decision occurs
_cache = {}


def cached(fn):
    def wrapper(*key):
        k = (fn.__name__,) + key
        if k not in _cache:
            _cache[k] = fn(*key)
        return _cache[k]
    wrapper.__name__, wrapper.__doc__ = fn.__name__, fn.__doc__
    return wrapper


class Pool:
    """int16 samples of evstream_ref's four kinds in turn, handed out in consecutive windows"""

    def __init__(self, rng, kinds=ER.KINDS, shift=0):
        parts = [ER.draw_read(rng, 6000, kinds[k % len(kinds)]) for k in range(24)]
        self.x = (np.concatenate(parts).astype(np.int32) + shift).clip(-32768, 32767).astype(np.int16)
        self.at = 0

    def take(self, n):
        if self.at + n > len(self.x):
            self.at = 0
        out = self.x[self.at:self.at + n].copy()
        self.at += n
        return out


def _i32(a):
    return np.asarray(a, dtype=np.int32)


# ---- part A: many entries in one push -----------------------------------------------------------------------------------
def many_lengths(rng, m, longs=230):
    """chunk lengths of one big push: 0 .. 20 samples, 60 .. 300 for `longs` entries anywhere and for every entry from
    LONG_FROM on (the last entry the longest), so both sides of entry SEAM emit"""
    n = rng.integers(0, 21, size=m)
    at = np.concatenate([rng.choice(LONG_FROM, size=longs, replace=False), np.arange(LONG_FROM, m)])
    n[at] = rng.integers(60, 301, size=at.size)
    n[m - 1] = 300
    n[min(m, SEAM) - 1] = 300
    return n


@cached
def event_many():
    """evstream_ref script, MANY_SLOTS slots: pushes of 4 095, 4 096 and 4 097 shuffled slots with a push of one entry
    between them, then 4 097 with END on every other entry"""
    rng = np.random.default_rng(20261021)
    pool = Pool(rng)
    ops = []
    for j, m in enumerate(BIG + (4097,)):
        slots = _i32(rng.permutation(MANY_SLOTS)[:m])
        chunks = [pool.take(int(n)) for n in many_lengths(rng, m)]
        end = np.zeros(m, dtype=np.int32)
        if j == 3:
            end[::2] = 1
        ops.append(("push", slots, chunks, end))
        if j < 3:
            ops.append(("push", _i32([int(rng.integers(0, MANY_SLOTS))]), [pool.take(150)], np.zeros(1, dtype=np.int32)))
    return {"params": DNA, "nslots": MANY_SLOTS, "ops": ops}


@cached
def live_targets():
    rng = np.random.default_rng(77)
    return [rng.normal(size=40), rng.normal(size=65)]


@cached
def live_many():
    """evstream_ref script for a live session of calibration length LIVE_CALIB on live_targets(): pushes of 4 095 and
    4 096 entries leave most slots CALIBRATING with held levels and a few hundred MAPPING; the push of 4 097 entries
    then holds slots that stay CALIBRATING, slots that become MAPPING with held levels in front of fresh ones, and
    slots already MAPPING -- with output on both sides of entry SEAM"""
    rng = np.random.default_rng(20261022)
    pool = Pool(rng, kinds=("steps", "walk", "clean"))
    ops = []
    for j, m in enumerate(BIG):
        slots = _i32(rng.permutation(MANY_SLOTS)[:m])
        chunks = [pool.take(int(n)) for n in many_lengths(rng, m, longs=150)]
        ops.append(("push", slots, chunks, np.zeros(m, dtype=np.int32)))
        if j < 2:
            ops.append(("push", _i32([int(rng.integers(0, MANY_SLOTS))]), [pool.take(150)], np.zeros(1, dtype=np.int32)))
    return {"params": DNA, "nslots": MANY_SLOTS, "ops": ops}


@cached
def hmm_many():
    """(model, hmmstream_ref script): a tie-heavy 3-state model, pushes of 4 095, 4 096, 4 097 and 4 097 shuffled slots
    in alternating feeds with a push of one entry between them and one reset with calibration pairs, chunks of 0 .. 40
    small integers"""
    import hmmstream_ref as HR
    rng = np.random.default_rng(20261023)
    model = HR.tie_model(rng, 3)
    d = np.arange(3)
    model["ltrans"][d, d] = np.where(np.isfinite(model["ltrans"][d, d]), model["ltrans"][d, d], -1.0)   # every state can stay
    ops = []
    for j, (m, feed) in enumerate(zip(BIG + (4097,), ("i16", "f64", "i16", "f64"))):
        slots = _i32(rng.permutation(MANY_SLOTS)[:m])
        chunks = [rng.integers(0, 4, int(n)).astype(np.int16 if feed == "i16" else np.float64) for n in rng.integers(0, 41, size=m)]
        ops.append(("push", slots, chunks, feed))
        one = "f64" if feed == "i16" else "i16"
        ops.append(("push", _i32([int(rng.integers(0, MANY_SLOTS))]),
                    [rng.integers(0, 4, 25).astype(np.int16 if one == "i16" else np.float64)], one))
        if j == 1:
            again = _i32(rng.permutation(MANY_SLOTS)[:100])
            ops.append(("reset", again, np.stack([rng.integers(-2, 3, 100).astype(np.float64), rng.choice([0.5, 1.0, 2.0], 100)], axis=1)))
    return model, {"nslots": MANY_SLOTS, "ops": ops}


MAP_SLOTS = 1100
MAP_LIVE = (1024, 1025, 1024)        # live slots of the three pushes: live * T = 2 048, 2 050, 2 048 with two targets


@cached
def map_many():
    """mapstream_ref case: targets of 40 and 65 points, three pushes that name slots 0 .. live - 1 in shuffled order with
    chunks of 32 .. 64 points -- three of 31 (always 16 lanes) and three of 257 (always 64 lanes) among them -- and two
    peeks at slots nobody else names"""
    rng = np.random.default_rng(20261024)
    targets = [rng.normal(size=40), rng.integers(-3, 4, size=65).astype(np.float64)]
    ties = rng.random(MAP_SLOTS) < 0.5
    steps = []
    for j, live in enumerate(MAP_LIVE):
        n = np.where(rng.random(live) < 0.8, rng.integers(32, 37, size=live), rng.integers(32, 65, size=live))
        odd = rng.choice(1024, size=6, replace=False)
        n[odd[:3]], n[odd[3:]] = 31, 257
        slots = [int(s) for s in rng.permutation(live)]
        chunks = [rng.integers(-3, 4, size=int(n[s])).astype(np.float64) if ties[s] else rng.normal(size=int(n[s])) for s in slots]
        for peek in (1090 + j, 1050 - j):
            at = int(rng.integers(0, len(slots) + 1))
            slots.insert(at, peek)
            chunks.insert(at, np.zeros(0))
        steps.append(("push", slots, chunks))
    return {"targets": targets, "nslots": MAP_SLOTS, "steps": steps}


def map_shapes(case, step):
    """(count, {N: (L, R)}) of a push of a mapping case: sk_map_session_push hands sk_exact_shape the live entries times
    the targets, restated by randcases.panel_shape; no chunk here passes one piece of 1 024 points"""
    import randcases as rc
    lens = [len(c) for c in case["steps"][step][2]]
    assert max(lens) <= 1024
    count = sum(n > 0 for n in lens) * len(case["targets"])
    return count, {n: rc.panel_shape(n, count, {}) for n in sorted(set(lens)) if n}


# ---- part B: rows as a C caller lays them out ------------------------------------------------------------------------------
LAYOUT_SLOTS = 70                    # two workgroups of k_evs_push, the second with 6 live lanes
LAYOUTS = ((304, 0), (303, 0), (304, 2), (304, 8), (301, 6))            # (stride in samples, byte shift of the base)
SEAM_LENS = (0, 1, 7, 8, 9, 127, 128, 129, 255, 256, 257, 300)           # the 128-sample tile and the 256-sample ring
PAD, PAD_ONE = -12345, 32767         # what stands behind a row's len; PAD_ONE under the layout (303, 0)
LAYOUT_TARGETS = live_targets


def pad_of(layout):
    return PAD_ONE if tuple(layout) == (303, 0) else PAD


@cached
def layout_script():
    """evstream_ref script of LAYOUT_SLOTS slots under the dna preset: a first push of odd lengths to every slot, two
    pushes whose lengths walk SEAM_LENS, a push to a subset with ENDs, and a closing END for all.  The samples sit around
    500 so that a MotifSeq session's filter (0, 1200) keeps most and drops some."""
    rng = np.random.default_rng(20261025)
    pool = Pool(rng, shift=500)
    S = LAYOUT_SLOTS
    ops = []
    zero = np.zeros(S, dtype=np.int32)
    ops.append(("push", _i32(rng.permutation(S)), [pool.take(int(n)) for n in 2 * rng.integers(0, 50, size=S) + 1], zero))
    for shift in (0, 5):
        lens = [SEAM_LENS[(i + shift) % len(SEAM_LENS)] for i in range(S)]
        ops.append(("push", _i32(rng.permutation(S)), [pool.take(n) for n in lens], zero))
    some = _i32(rng.permutation(S)[:41])
    ops.append(("push", some, [pool.take(int(n)) for n in rng.integers(0, 301, size=some.size)],
                _i32(rng.random(some.size) < 0.3)))
    ops.append(("push", _i32(np.arange(S)), [np.zeros(0, dtype=np.int16)] * S, np.ones(S, dtype=np.int32)))
    return {"params": DNA, "nslots": S, "ops": ops}


def rows_of(chunks, stride, pad):
    """(rows int16 [m, stride] with `pad` behind every chunk, lens int32 [m])"""
    rows = np.full((len(chunks), stride), pad, dtype=np.int16)
    for i, c in enumerate(chunks):
        rows[i, :len(c)] = c
    return rows, _i32([len(c) for c in chunks])


# ---- part C: what the header promises of device-form pushes ---------------------------------------------------------------
CONTRACT_SLOTS = 6
CONTRACT_STRIDE = 40


@cached
def contract_script(ends=True):
    """The pushes of the contract tests, as dicts of what the C caller hands over -- slots, len (as written, unclamped),
    end -- and `chunks`: what the header says each entry amounts to (None: the entry names no slot of the session and
    is skipped).  Rows hold CONTRACT_STRIDE samples each; a len of -5 is 0 samples and stride + 9 is the whole row.
    ends: the session knows END (event, live), so an ended slot takes nothing; False: the flags mean nothing to it."""
    rng = np.random.default_rng(20261026)
    pool = Pool(rng, shift=500)
    st = CONTRACT_STRIDE
    rows = [[pool.take(st) for _ in range(CONTRACT_SLOTS + 2)] for _ in range(5)]
    pushes = [
        # clamping: -5 is 0, stride + 9 is stride
        dict(slots=[0, 1, 2, 3, 4, 5], len=[st, -5, st + 9, 17, 0, st], end=[0, 0, 0, 0, 0, 0]),
        # entries that name no slot: -1 and nslots, in the middle and at the end; slot 5 ends
        dict(slots=[3, -1, 0, 1, 5, CONTRACT_SLOTS], len=[st, 30, 23, st + 9, 11, st], end=[0, 0, 0, 0, 1, 1]),
        # samples for the ended slot 5: ignored
        dict(slots=[5, 2, 4], len=[st, 9, st], end=[0, 0, 0]),
        # (a reset of slot 5 comes here)
        dict(slots=[5, 0, -1], len=[st, -5, 8], end=[0, 0, 0]),
        dict(slots=[0, 1, 2, 3, 4, 5], len=[0, 0, 0, 0, 0, 0], end=[1, 1, 1, 1, 1, 1]),
    ]
    ended = set()
    for j, p in enumerate(pushes):
        if j == 3:
            ended.discard(5)
        p["rows"] = np.stack(rows[j][:len(p["slots"])])
        p["chunks"] = []
        for i, (s, n, e) in enumerate(zip(p["slots"], p["len"], p["end"])):
            if not 0 <= s < CONTRACT_SLOTS:
                p["chunks"].append(None)
                continue
            n = 0 if s in ended else min(max(n, 0), st)
            p["chunks"].append(p["rows"][i, :n].copy())
            if e and ends:
                ended.add(s)
    return pushes


CONTRACT_RESET_BEFORE = 3            # slot 5 is reset before this push of contract_script()


def contract_ops(with_end=True):
    """contract_script() as the statement modules take it: the skipped entries left out, the reset in its place.
    Returns (ops, keep): keep[j] are the entry indices of push j that name a slot."""
    ops, keep = [], []
    for j, p in enumerate(contract_script(bool(with_end))):
        if j == CONTRACT_RESET_BEFORE:
            ops.append(("reset", _i32([5])))
        k = [i for i, c in enumerate(p["chunks"]) if c is not None]
        keep.append(k)
        ops.append(("push", _i32([p["slots"][i] for i in k]), [p["chunks"][i] for i in k],
                    _i32([p["end"][i] if with_end else 0 for i in k])))
    return ops, keep


# ---- part D: sessions between other calls --------------------------------------------------------------------------------
# the one-shot calls in the order they come: sizes go up and then down (pairs 130: 19 pairs, pairs 9: 202 pairs and
# 19.6 M cells; pairpaths 22: 5 pairs, 145: 204; hits 324: rows of 4 376 samples, hits 1: 122 601; detect 4: 28 000
# samples, 27: 55 000 in rows of 12 683; hmm 3: one read, 35: 130 reads of six states; panel 29: two motifs, 4: 256; drna
# 39: rows of 115 samples, 14: 74 677), so the context's grow-only buffers are reallocated between two pushes of a session
ONESHOT = [("pairs", 130), ("pairpaths", 22), ("hits", 324), ("detect", 4), ("hmm", 3), ("panel", 29), ("drna", 39),
           ("band", 0), ("pairhits", 0),
           ("pairs", 9), ("pairpaths", 145), ("hits", 1), ("detect", 27), ("hmm", 35), ("panel", 4), ("drna", 14),
           ("maphits", 0), ("pairhits", 1), ("maphits", 0),
           ("pairs", 130), ("hits", 324), ("detect", 4), ("hmm", 3), ("drna", 39), ("band", 0), ("pairhits", 0)]
SESSIONS = ("event", "hmm", "mapA", "mapB", "motif", "live")
MOTIF_PARAMS = dict(W=60, mode="medmad", lo=0, hi=1200)


@cached
def band_case():
    """a dtw_band list: drifting pairs and tie-heavy ones, inside and beyond band / 2"""
    import band_ref
    rng = np.random.default_rng(20261027)
    seqs = []
    for M in (40, 150, 300):
        seqs += list(band_ref.drift_pair(rng, M=M, stall=0))
    seqs += [band_ref.ties(rng, 90), band_ref.ties(rng, 120)]
    return {"seqs": seqs, "pairs": [(0, 1), (2, 3), (4, 5), (6, 7), (0, 1), (6, 1)], "band": 128, "end": "pinned"}


@cached
def pairhits_case(large):
    """a dtw_pairs_hits list: 3 pairs on a target of 300 points, or 40 pairs on targets of 300, 1 500 and 4 097 points
    (more rows than any session's hit list here names: c->rowhit grows)"""
    rng = np.random.default_rng(20261028 + int(large))
    nq = 4
    seqs = [rng.integers(-3, 4, size=n).astype(np.float64) if k % 2 else rng.normal(size=n) for k, n in enumerate((16, 17, 30, 24))]
    seqs += [rng.normal(size=M) for M in ((300, 1500, 4097) if large else (300,))]
    nt = len(seqs) - nq
    npairs = 40 if large else 3
    pairs = [(int(rng.integers(0, nq)), nq + int(rng.integers(0, nt))) for _ in range(npairs)]
    return {"seqs": seqs, "pairs": pairs, "K": 3}


def _map_steps(rng, nslots, pushes):
    steps = []
    for _ in range(pushes):
        slots = [int(s) for s in rng.permutation(nslots)[:int(rng.integers(max(1, nslots - 2), nslots + 1))]]
        steps.append(("push", slots, [rng.normal(size=int(rng.choice((0, 1, 17, 33, 64, 100, 257)))) for _ in slots]))
    return steps


@cached
def interleave_scripts():
    """the six sessions' scripts: {"event": evstream_ref script, "hmm": (model name, hmmstream_ref script), "mapA" / "mapB":
    mapstream_ref cases on different targets, "motif": {"motifs", "nslots", "ops"}, "live": evstream_ref script}"""
    import hmmstream_ref as HR
    rng = np.random.default_rng(20261029)
    out = {}
    out["event"] = ER.draw_session(rng, nslots=70, budget=9000, maxlen=300)
    out["hmm"] = ("synth_raw", HR.draw_session(rng, nslots=65, budget=12000, maxlen=200,
                                               draw_chunk=lambda r, n: r.integers(380, 620, n).astype(np.int16)))
    out["mapA"] = {"targets": [rng.normal(size=200), rng.normal(size=65)], "nslots": 9, "steps": _map_steps(rng, 9, 5)}
    out["mapB"] = {"targets": [rng.integers(-3, 4, size=513).astype(np.float64)], "nslots": 5, "steps": _map_steps(rng, 5, 4)}
    pool = Pool(rng, shift=500)
    motif_ops = []
    for _ in range(4):
        slots = _i32(rng.permutation(5)[:int(rng.integers(3, 6))])
        motif_ops.append(("push", slots, [pool.take(int(rng.choice((0, 1, 63, 64, 200, 256)))) for _ in slots]))
    out["motif"] = {"motifs": [np.sin(np.arange(17) * 0.9) * 1.3, rng.normal(size=40)], "nslots": 5, "ops": motif_ops}
    live = ER.draw_session(rng, nslots=65, budget=3000, maxlen=300)
    live["params"] = DNA
    out["live"] = live
    return out


def session_ops(scripts, name):
    s = scripts[name]
    return s[1]["ops"] if name == "hmm" else s["steps"] if name.startswith("map") else s["ops"]


@cached
def interleave_sequence():
    """The fixed walk: a list of ("session", name) -- the next op of that session -- and the ONESHOT entries in their
    order.  Every session's first op comes first; then a seeded shuffle that keeps each session's ops and the one-shot
    calls in order; the ops left over come last, so every session has a push after the largest calls."""
    rng = np.random.default_rng(20261030)
    scripts = interleave_scripts()
    left = {name: len(session_ops(scripts, name)) - 1 for name in SESSIONS}
    seq = [("session", name) for name in SESSIONS]
    keep_last = {name: min(1, left[name]) for name in SESSIONS}       # one op per session waits for the end
    for name in SESSIONS:
        left[name] -= keep_last[name]
    shots = list(ONESHOT)
    while shots or any(left.values()):
        names = [n for n in SESSIONS if left[n]]
        take_shot = shots and (not names or rng.random() < len(shots) / (len(shots) + sum(left.values())))
        if take_shot:
            seq.append(shots.pop(0))
            while shots and (shots[0][0] == "maphits" or seq[-1][0] == "maphits"):   # hits, the large list, hits: together
                seq.append(shots.pop(0))
        else:
            name = names[int(rng.integers(0, len(names)))]
            seq.append(("session", name))
            left[name] -= 1
    seq += [("session", name) for name in SESSIONS if keep_last[name]]
    return seq
