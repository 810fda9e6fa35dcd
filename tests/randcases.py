"""Seeded random cases for the four newest kernel files (csrc/sk_sweep.hip, sk_hits.hip, sk_path.hip, sk_pull.hip): per
family  draw_<family>(rng) -> case,  expect_<family>(ora, case) -> what the reference says,  call_<family>(api, case,
exp) -> what the GPU says,  diff_<family>(case, got, exp) -> None or the first difference as text.

A plain module: not collected, no conftest, pure numpy, no GPU import at module level (`api` is handed in).  The same
seed gives the same case on any machine: draw_* take a numpy.random.Generator and nothing else.  Used by
tests/test_random_cases.py (CPU: the committed seeds reach what they claim), tests/test_gpu_random.py (GPU: every seed
against its reference, plus one interleaved sequence) and tools/fuzz_gpu.py (open-ended).  tests/RANDOM_CASES.md says
what each family draws and which one-line kernel mutants the committed seeds catch.

The references are the statements that already exist: the oracle's scale_outliers + get_segs per (set, read) for the
sweep, reference_hits (test_hits_host.py), reference_paths (test_paths_host.py), numpy_pull_text (test_squigglepull.py).
Every comparison is exact: integers as integers, distances and text byte for byte.

Wall times (one run each, 16 oracle threads at most): `pytest tests -m "not gpu"` 70.6 s without tests/test_random_cases.py
and 69.2 s with it (the module alone: 14 s); `pytest tests -m gpu` on the MI355X 277.7 s with tests/test_gpu_random.py,
which alone takes 10.4 s -- about 267 s without it (not run separately).
"""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:                       # (tools/fuzz_gpu.py imports this module from outside tests/)
    sys.path.insert(0, _HERE)

# ---- the committed seeds (tests/test_random_cases.py asserts what they reach) -------------------------------------
SEEDS = {
    "sweep": [16, 22, 60, 97],
    "hits": [1, 20, 87, 95, 131, 214, 298, 324],
    "paths": [1, 12, 29, 50, 123, 135, 187, 272],
    "pull": [0, 3, 21, 40],
}

# every tuning switch a case may set; a runner clears the ones a case does not name
SWITCHES = ("SK_SEG_DELTA_SCALE", "SK_WALK_GENERAL", "SK_DTW_SMALL_MAX", "SK_HITS_ROW_BYTES", "SK_PATH_LDS_BYTES",
            "SK_PATH_SCRATCH_BYTES")


def rng_of(family, seed):
    """The generator of a committed case: the family is part of the seed, so the four lists do not share streams."""
    return np.random.default_rng([sorted(SEEDS).index(family), int(seed)])


def case_of(family, seed):
    case = DRAW[family](rng_of(family, seed))
    case["seed"] = int(seed)
    return case


def _pick(rng, values):
    return values[int(rng.integers(len(values)))]


def _plain(v):
    if isinstance(v, (np.integer,)):
        return int(v)
    if isinstance(v, (np.floating,)):
        return float(v)
    return v


def describe(case):
    """Everything needed to reproduce a case, on one line."""
    keys = [k for k in case if k not in ("reads", "rows", "sets", "motifs", "prefixes", "calib", "lens", "sig")]
    return "%s seed=%s %s env=%s" % (case["family"], case.get("seed"),
                                     " ".join("%s=%s" % (k, _plain(case[k])) for k in keys
                                              if k not in ("family", "seed", "env")), case["env"])


# ======================================================================================================================
# sweep
# ======================================================================================================================
# sk_launch_seg_sweep_walk: a launch of n sets gives each read setw = the power of two >= n lanes (at most 64, the
# wavefront), 64 / setw reads per wavefront, and slices of 64 sets on grid.y.  So the set counts to reach are the
# powers of two and their neighbours up to 64, and counts past 64 (two slices, the second one partly filled).
SWEEP_LANES = 64
SWEEP_COUNTS = (1, 2, 3, 7, 8, 9, 33, SWEEP_LANES - 1, SWEEP_LANES, SWEEP_LANES + 1, 2 * SWEEP_LANES + 2)
# squeeze_entry / the bit queue of k_seg_sweep_walk work on 64-sample entries and 32-sample words
SWEEP_LENS = (0, 1, 31, 32, 33, 63, 64, 65)
SWEEP_LONG = 70000                               # "ragged up to >= 70 000": many 128-byte lines of entries per read
# api._too_wide_for_i16: limits further apart than 38 000 values take the float64 route
SWEEP_WIDE = (-40000, 40000)
SWEEP_NARROW = ((0, 900), (0, 900), (200, 2500), (-50, 1200), (300, 800))
SWEEP_STD = (0.5, 0.75, 0.75, 1.0, 1.5, 3.0, 0.0)
# run_word32 serves error < corrector, corrector >= 1, window >= 1, first_len = ceil(window * stall_len) >= 1;
# gen_word32 the rest
SWEEP_ERROR = (5, 5, 3, 0, -1, 10, 60)
SWEEP_CORRECTOR = (50, 50, 3, 0, 20)
SWEEP_WINDOW = (150, 100, 20, 1, 0, 126, 127, 400)
SWEEP_SEG_DIST = (50, 0, 1, 10 ** 9)
SWEEP_STALL_LEN = (0.25, 0.0, 0.05, 0.9, 1.2)
F64_STREAM_MAX = 4096                            # sk_f64stat.hip: the streaming statistics kernel's longest read


def sweep_is_fast(s):
    """sk_sweep_plan's test for the run-hopping walk (without SK_WALK_GENERAL)."""
    fl = float(s["window"]) * float(s["stall_len"])
    return s["error"] < s["corrector"] and s["corrector"] >= 1 and s["window"] >= 1 and int(np.ceil(fl)) >= 1


def _sweep_one_set(rng):
    return dict(error=_pick(rng, SWEEP_ERROR), corrector=_pick(rng, SWEEP_CORRECTOR), window=_pick(rng, SWEEP_WINDOW),
                seg_dist=_pick(rng, SWEEP_SEG_DIST), stall_len=_pick(rng, SWEEP_STALL_LEN),
                stall_start=_pick(rng, (300, 50, 0)), gap_dist=_pick(rng, (3000, 10, 0)))


def _stall_read(rng, n, base=500.0, spread=60.0, f64=False):
    """Noise with a quiet stretch near the start and one in the middle, so that segments appear."""
    x = rng.normal(base, spread, n)
    if n >= 400:
        a = int(rng.integers(0, 60))
        x[a:a + int(rng.integers(120, 500))] = rng.normal(base + 5, spread / 8, 1)[0]
        m = n // 2
        w = int(rng.integers(160, 600))
        x[m:m + w] = rng.normal(base - 5, spread / 8, min(w, n - m))
        x += rng.normal(0, spread / 20, n)
    return x


def draw_sweep(rng):
    from squigglekit_amd import synth
    long_case = rng.random() < 0.25
    env = {}
    if rng.random() < 0.25:
        env["SK_SEG_DELTA_SCALE"] = "1e13"       # every read through the numpy-order redo
    if rng.random() < 0.2:
        env["SK_WALK_GENERAL"] = "1"             # every set through gen_word32
    form = _pick(rng, ("batch", "list", "list"))
    # ---- the sets: 2 .. 4 groups of (lim_low, lim_hi, std_scale), one of them too wide for the int16 kernels
    ngroups = int(rng.integers(2, 5))
    counts = [int(_pick(rng, SWEEP_COUNTS[:6] if long_case else SWEEP_COUNTS)) for _ in range(ngroups)]
    if not long_case and rng.random() < 0.5:
        counts[0] = int(_pick(rng, SWEEP_COUNTS[6:]))
    wide_at = int(rng.integers(ngroups))
    counts[wide_at] = min(counts[wide_at], 9)    # (the float64 route costs one launch per set kind all the same)
    sets, group_counts, used = [], [], set()
    for g in range(ngroups):
        while True:
            lim = SWEEP_WIDE if g == wide_at else _pick(rng, SWEEP_NARROW)
            key = (lim, _pick(rng, SWEEP_STD))
            if key not in used:
                used.add(key)
                break
        mix = _pick(rng, ("fast", "gen", "mixed", "mixed"))
        n = 0
        while n < counts[g]:
            s = _sweep_one_set(rng)
            if (mix == "fast" and not sweep_is_fast(s)) or (mix == "gen" and sweep_is_fast(s)):
                continue
            s.update(lim_low=key[0][0], lim_hi=key[0][1], std_scale=key[1])
            sets.append(s)
            n += 1
        group_counts.append((counts[g], mix))
    order = rng.permutation(len(sets))           # the groups interleaved: sk_sweep_plan has to find them
    sets = [sets[int(i)] for i in order]
    # ---- the reads
    reads = []
    budget = 36_000_000 // max(1, len(sets))     # samples the oracle walks per set
    M = int(_pick(rng, (512, 1000, 2047, 4000, 4001)))
    R = int(_pick(rng, (3, 9, 17, 40)))
    R = max(2, min(R, budget // (2 * M)))
    kind = int(rng.integers(3))
    if kind == 0 or M < 512:
        reads += [r for r in synth.squiggle_batch(R, M, int(rng.integers(1 << 30)))]
    elif kind == 1:
        reads += [r for r in synth.pattern_reads(rng, R, M)]
    else:
        reads += [r for r in synth.squiggle_batch(R - R // 2, M, int(rng.integers(1 << 30)))]
        reads += [r for r in synth.pattern_reads(rng, max(1, R // 2), M)]
    reads.append(np.full(int(rng.integers(1, 300)), 500, dtype=np.int16))                 # constant: std 0
    reads.append(np.full(int(rng.integers(1, 300)), 2000, dtype=np.int16))                # empty after most filters
    for n in rng.choice(SWEEP_LENS, size=4, replace=False):
        reads.append(rng.integers(300, 700, size=int(n)).astype(np.int16))
    if long_case:
        n = int(rng.integers(SWEEP_LONG, SWEEP_LONG + 20000))
        x = np.clip(np.rint(_stall_read(rng, n)), -32768, 32767).astype(np.int16)
        if rng.random() < 0.5:
            x[:4000] = synth.pattern_reads(rng, 1, 4000)[0]
        x[rng.integers(0, n, 30)] = rng.choice([0, 950, -7, 3000], 30)
        reads.append(x)
    nfloat = 0
    if form == "list":
        # float64 reads: the streaming statistics kernel up to F64_STREAM_MAX samples, the others beyond; ties on a
        # 0.01 grid, NaN / inf inside
        for n in (int(_pick(rng, (5, 64, 1000, F64_STREAM_MAX - 1, F64_STREAM_MAX))),
                  int(rng.integers(F64_STREAM_MAX + 1, 9000))):
            x = np.round(_stall_read(rng, n, 90.0, 15.0), 2)
            if rng.random() < 0.6 and n > 8:
                x[rng.integers(0, n, 3)] = rng.choice([np.nan, np.inf, -np.inf, 899.99, 0.01], 3)
            reads.append(x)
            nfloat += 1
    order = rng.permutation(len(reads))
    reads = [reads[int(i)] for i in order]
    case = dict(family="sweep", form=form, sets=sets, group_counts=group_counts, reads=reads, nreads=len(reads),
                rowkind=("squiggle", "pattern", "both")[kind] if M >= 512 else "squiggle", M=M,
                nsets=len(sets), nfloat=nfloat, longest=max(len(r) for r in reads), env=env)
    if form == "batch":
        stride = (case["longest"] + 8 + int(rng.integers(0, 40))) // 8 * 8               # stride > the longest row
        sig = rng.integers(-100, 1300, size=(len(reads), stride)).astype(np.int16)       # (padding is not zeros)
        for i, r in enumerate(reads):
            sig[i, :len(r)] = r
        case["sig"], case["lens"] = sig, np.array([len(r) for r in reads], dtype=np.int32)
        case["stride"] = stride
    return case


def _oracle_seg_params(ora, s):
    return ora.SegParams(s["error"], s["corrector"], s["window"], s["seg_dist"], s["std_scale"], s["stall_len"])


def expect_sweep(ora, case):
    """recs[set][read] as the 6 integers of a sweep record, sums recomputed from them; `nsegs_all`: segment counts
    before the two-segment cut (for the CPU leg's conditions)."""
    from concurrent.futures import ThreadPoolExecutor
    from squigglekit_amd import _lib, api
    from test_gpu_sweep import _expected_rec, _sums_from_recs
    sets, reads = case["sets"], case["reads"]
    filtered = {}
    for s in sets:
        key = (s["lim_low"], s["lim_hi"])
        if key not in filtered:
            filtered[key] = [ora.scale_outliers(np.asarray(r, dtype=np.float64), key[0], key[1]) for r in reads]

    def one(k):
        s = sets[k]
        p = _oracle_seg_params(ora, s)
        out = []
        for f in filtered[s["lim_low"], s["lim_hi"]]:
            segs = (ora.get_segs(f, p, max_segs=f.size // 2 + 8) or []) if f.size else []
            out.append((_expected_rec(segs, len(segs)), len(segs)))
        return out
    with ThreadPoolExecutor(16) as ex:
        rows = list(ex.map(one, range(len(sets))))
    recs = np.zeros((len(sets), len(reads)), dtype=_lib.SWEEP_REC_DTYPE)
    nall = np.zeros((len(sets), len(reads)), dtype=np.int64)
    for k, row in enumerate(rows):
        for r, (rec, n) in enumerate(row):
            recs[k, r] = rec
            nall[k, r] = n
    sweep_sets = [api.sweep_set(**s) for s in sets]
    return dict(recs=recs, sums=_sums_from_recs(sweep_sets, recs), nsegs_all=nall)


def call_sweep(api, case, exp=None):
    sets = [api.sweep_set(**s) for s in case["sets"]]
    if case["form"] == "batch":
        return api.segment_sweep(case["sig"], sets, case["lens"], records=True)
    return api.segment_sweep(case["reads"], sets, records=True)


def diff_sweep(case, got, exp):
    sums, recs = got
    if recs.shape != exp["recs"].shape:
        return "records shaped %s, want %s" % (recs.shape, exp["recs"].shape)
    bad = np.argwhere(recs != exp["recs"])
    if bad.size:
        k, r = (int(v) for v in bad[0])
        return "set %d %s read %d (%d samples): got %s want %s" % (k, case["sets"][k], r, len(case["reads"][r]),
                                                                   recs[k, r], exp["recs"][k, r])
    if not np.array_equal(sums, exp["sums"]):
        k = int(np.flatnonzero(sums != exp["sums"])[0])
        return "summary of set %d %s: got %s want %s" % (k, case["sets"][k], sums[k], exp["sums"][k])
    return None


# ======================================================================================================================
# hit lists and paths
# ======================================================================================================================
# N: lanes-per-read layouts of the exact pass change at 16 / 64 rows (k_sdtw), sk_path.hip sweeps the motif in stripes
# of 64 rows ((N + 63) >> 6: 64 | 65, 128 | 129), the chained pass starts beyond 1 024 points; 200 and 512 / 513 are
# the default model's size and the screening kernels' 16-lane limit.
HITS_N = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200, 512, 513, 1024, 1025)
HITS_K = (1, 2, 3, 8, 63, 64)                    # sk_hits.hip: lane h holds interval h, K <= 64
HIT_CACHE_COLS = 64 * 64                         # sk_hits.hip: 64 * HIT_CACHE columns are selected from registers
HITS_LONG = 100000
HITS_ROUTES = ("list", "batch", "pa", "centi", "wide")
HITS_CELLS = 14_000_000                          # cost-matrix cells the reference fills per case (CPU time)
# sk_path.hip
PATH_LDS_BYTES = 2 * 200 * 512 // 8
PATH_LDS_COLS = 1024
PATH_WORD_COLS = 16                              # direction words: 16 cells of a row, 2 bits each


def _np_medmad(f):
    med = np.median(f)
    return (f - med) / (np.median(np.abs(f - med)) * 1.4826)


def _hit_read(rng, n, motifs, kind):
    """One raw int16 read of n samples."""
    from squigglekit_amd import synth
    if kind == "ties":                                                       # tie-heavy small integers
        step = int(_pick(rng, (1, 10)))
        return (480 + step * rng.integers(0, int(_pick(rng, (3, 4))), size=n)).astype(np.int16)
    x = synth.squiggle_batch(1, max(n, 8), int(rng.integers(1 << 30)))[0][:n].copy()
    for m in motifs:                                                         # copies of the motifs, where they fit
        img = np.clip(np.rint(m * 93.4 + 511.0), -32768, 32767).astype(np.int16)
        for _ in range(int(rng.integers(0, 4))):
            if img.size < n:
                a = int(rng.integers(0, n - img.size))
                x[a:a + img.size] = img
    if kind == "dropped" and n:                                               # many samples the filter drops
        k = max(1, n // int(_pick(rng, (3, 7, 20))))
        x[rng.integers(0, n, k)] = rng.choice([-5, 0, 1200, 1500, 3000], k)
    return x


def draw_hits(rng, paths=False):
    from squigglekit_amd import synth
    env = {}
    nm = int(_pick(rng, (1, 1, 2, 3)))
    Ns = [int(_pick(rng, HITS_N)) if rng.random() < 0.75 else int(rng.integers(1, 600)) for _ in range(nm)]
    if paths and nm > 1 and len(set(Ns)) == 1:
        Ns[1] = Ns[0] + 1                                                    # motifs of different lengths in one call
    motifs = [synth.synthetic_motif(N, seed=int(rng.integers(1000))) for N in Ns]
    N0 = Ns[0]
    K = int(_pick(rng, HITS_K))
    route = _pick(rng, HITS_ROUTES)
    scale = _pick(rng, ("medmad", "medmad", "zscale"))
    lo, hi = (-10000, 30000) if route == "wide" else _pick(rng, ((0, 1200), (0, 1200), (0, 900), (-50, 2500)))
    special = None
    u = rng.random()
    if u < 0.12 and not paths:
        special = "long"                                                     # one read >= HITS_LONG samples
    elif u < 0.15 and paths:
        special = "plateau"                                                  # a best window wider than PATH_LDS_COLS
    elif u < 0.3:
        special = "over"                                                     # a read beyond HIT_CACHE_COLS columns
    if special == "long":
        Ns = [int(_pick(rng, (15, 30, 64)))]
        motifs, N0, route = [synth.synthetic_motif(Ns[0], seed=int(rng.integers(1000)))], Ns[0], "list"
    if special == "plateau":
        route, scale, lo, hi = _pick(rng, ("list", "batch")), "medmad", 0, 32768
    # ---- read lengths: around the first motif's length, then at random
    # (a read of one sample has MAD = std = 0 and is only checked for its flag: not in every case)
    lens = list(dict.fromkeys(([1] if rng.random() < 0.4 else []) + [max(2, N0 - 1), max(2, N0), N0 + 1, 2 * N0]))
    lens += [int(rng.integers(16, 6001)) for _ in range(int(rng.integers(5, 9)))]
    if special == "over":
        lens.append(int(rng.integers(HIT_CACHE_COLS + 1, 6001)))
    cells = sum(Ns)
    keep, total = [], 0
    for n in lens:                                                           # (the reference's CPU time)
        if (total + n) * cells <= HITS_CELLS or len(keep) < 5:
            keep.append(n)
            total += n
    lens = keep
    kinds = ["squiggle"] * len(lens)
    for i in range(len(lens)):
        if lens[i] >= 16:                                                    # (shorter ones: distinct values, MAD > 0)
            kinds[i] = _pick(rng, ("squiggle", "squiggle", "ties", "dropped"))
    reads = [_hit_read(rng, n, motifs, k) for n, k in zip(lens, kinds)]
    nbad = 0
    u = rng.random()
    if u < 0.25:
        reads.append(np.full(int(rng.integers(1, 80)), 2000 if route != "wide" else 31000, dtype=np.int16))
        nbad += 1                                                            # nothing survives the filter
    elif u < 0.4:
        reads.append(np.full(int(rng.integers(2, 80)), 500, dtype=np.int16))  # MAD = 0, std = 0
        nbad += 1
    if special == "long":
        reads.append(_hit_read(rng, int(rng.integers(HITS_LONG, HITS_LONG + 30000)), motifs, "squiggle"))
    if special == "plateau":
        # test_gpu_paths.plateau_read: one high sample, a two-value plateau, one distinct last sample; the motif is
        # (first, plateau, last) in normalised units, so its best window spans the whole plateau
        npl = int(rng.integers(PATH_LDS_COLS + 40, PATH_LDS_COLS + 700))
        raw = np.concatenate([[32767], np.where(np.arange(npl) % 2 == 0, 600, 601), [12000]]).astype(np.int16)
        y = _np_medmad(raw.astype(np.float64))
        motifs = [np.array([y[0], y[1], y[-1]])] + motifs[1:]
        Ns[0] = 3
        reads.append(raw)
    order = rng.permutation(len(reads))
    reads = [reads[int(i)] for i in order]
    if route in ("pa", "centi"):
        dig, ofs, rg = _pick(rng, ((8192.0, 16.0, 1493.94), (2048.0, -3.0, 748.58), (8192.0, 7.25, 1467.61)))
        reads = [np.round((r.astype(np.int64) + ofs) * (rg / dig), 2) for r in reads]
        lo, hi = _pick(rng, ((0, 1200), (0, 900), (40, 160)))
    longest = max(len(r) for r in reads)
    case = dict(family="paths" if paths else "hits", route=route, Ns=Ns, K=K, scale=scale, lo=lo, hi=hi, special=special,
                cut=_pick(rng, ("inf", "inf", "median2", "below")), motifs=motifs, reads=reads, nreads=len(reads),
                nbad=nbad, longest=longest, kinds="".join(k[0] for k in kinds), env=env)
    if route == "batch":
        stride = (longest + 8 + int(rng.integers(0, 64))) // 8 * 8           # stride > the longest row
        sig = rng.integers(300, 700, size=(len(reads), stride)).astype(np.int16)
        for i, r in enumerate(reads):
            sig[i, :len(r)] = r
        case["sig"], case["lens"], case["stride"] = sig, np.array([len(r) for r in reads], dtype=np.int32), stride
    # ---- switches
    if rng.random() < 0.3:
        env["SK_DTW_SMALL_MAX"] = "0"                                        # four reads per wavefront, as big batches
    if rng.random() < 0.3 and len(reads) >= 3 and special != "long":
        # run_hits (sk_api.hip): per read sizeof(sk_hit) + row_stride * 12 bytes of last row; row_stride is the stride
        # of the int16 batch or the longest float64 read.  A third of the reads per chunk: three chunks or more.
        row = case.get("stride", (longest + 7) // 8 * 8 if route in ("list",) else longest)
        row = max(row, 8) if route == "list" else row
        case["row_stride"] = int(row)
        env["SK_HITS_ROW_BYTES"] = str((24 + 12 * int(row)) * max(1, len(reads) // 3))
    if paths:
        u = rng.random()
        if u < 0.25:
            env["SK_PATH_LDS_BYTES"] = "0"                                   # every hit takes the scratch tier
        elif u < 0.6:
            # k_path_lds keeps a hit when N * ceil(W / 16) words fit: a budget for windows of about the motif's length
            N = Ns[0]
            wsplit = max(1, int(N * rng.uniform(0.9, 1.4)))
            env["SK_PATH_LDS_BYTES"] = str(min(PATH_LDS_BYTES - 4, 4 * N * ((wsplit + PATH_WORD_COLS - 1) // PATH_WORD_COLS)))
        if rng.random() < 0.3:
            env["SK_PATH_SCRATCH_BYTES"] = "1000"                            # less than one slab: a single wavefront
    return case


def draw_paths(rng):
    return draw_hits(rng, paths=True)


def hits_chunks(case):
    """Chunks run_hits makes of the case's reads under its SK_HITS_ROW_BYTES (1 when unset)."""
    if "SK_HITS_ROW_BYTES" not in case["env"]:
        return 1
    per = 24 + 12 * case["row_stride"]
    chunk = max(1, min(case["nreads"], int(case["env"]["SK_HITS_ROW_BYTES"]) // per))
    return -(-case["nreads"] // chunk)


def path_lds_words(case):
    """sk_launch_paths: the LDS tier's budget in words under the case's SK_PATH_LDS_BYTES."""
    words = PATH_LDS_BYTES // 4
    if "SK_PATH_LDS_BYTES" in case["env"]:
        v = int(case["env"]["SK_PATH_LDS_BYTES"])
        if v >= 0 and v // 4 < words:
            words = v // 4
    return words


def path_tier(case, N, W):
    words = N * ((W + PATH_WORD_COLS - 1) // PATH_WORD_COLS)
    return "lds" if words <= path_lds_words(case) and W <= PATH_LDS_COLS else "scratch"


def _cut_of(case, full):
    """max_dist from the reference's full lists of the first motif."""
    if case["cut"] == "inf":
        return float("inf")
    if case["cut"] == "median2":
        second = [h[1][0] for h in full if h and len(h) > 1]
        return float(np.median(second)) if second else float("inf")
    best = [h[0][0] for h in full if h]
    return float(np.nextafter(np.median(best), 0.0)) if best else 0.0        # below the best distance of half the reads


def _first(h):
    return h[0] if isinstance(h[0], tuple) else h


def expect_hits(ora, case):
    """dict(max_dist, want): want[m][r] = reference_hits' list (None: not compared) for motif m."""
    from concurrent.futures import ThreadPoolExecutor
    from test_hits_host import reference_hits
    from test_paths_host import reference_paths
    reads, kw = case["reads"], dict(scale=case["scale"], lo=case["lo"], hi=case["hi"])
    paths = case["family"] == "paths"
    with ThreadPoolExecutor(16) as ex:
        cut = float("inf")
        if case["cut"] != "inf":
            full = list(ex.map(lambda r: reference_hits(ora, [r], case["motifs"][0], 64, **kw)[0], reads))
            cut = _cut_of(case, full)
        fn = reference_paths if paths else reference_hits
        jobs = [(m, r) for m in case["motifs"] for r in reads]
        flat = list(ex.map(lambda mr: fn(ora, [mr[1]], mr[0], case["K"], cut, **kw)[0], jobs))
    R = len(reads)
    return dict(max_dist=cut, want=[flat[k * R:(k + 1) * R] for k in range(len(case["motifs"]))])


expect_paths = expect_hits


def call_hits(api, case, exp):
    paths = case["family"] == "paths"
    args = (case["motifs"], case["K"], exp["max_dist"], case["scale"], case["lo"], case["hi"])
    if case["route"] == "batch":
        fn = api.motifseq_paths_batch if paths else api.motifseq_hits_batch
        return fn(case["sig"], case["lens"], *args)
    if case["route"] == "centi":
        flat, off = api.pack_f64(case["reads"])
        fn = api.motifseq_paths_ragged_f64 if paths else api.motifseq_hits_ragged_f64
        return fn(np.round(flat * 100).astype(np.int32), off, *args)
    return (api.motifseq_paths if paths else api.motifseq_hits)(case["reads"], *args)


call_paths = call_hits


def diff_hits(case, got, exp):
    """What test_gpu_hits.same / test_gpu_paths.same assert, as text: counts, (start, end), the distance's bytes, the
    spans as integers, unused slots NaN / -1, reads without a result flagged."""
    paths = case["family"] == "paths"
    for m, (res, want) in enumerate(zip(got, exp["want"])):
        hits, count = res[0], res[1]
        spans = res[2] if paths else None
        for r, w in enumerate(want):
            tag = "motif %d (N=%d) read %d (%d samples)" % (m, len(case["motifs"][m]), r, len(case["reads"][r]))
            if w is None:
                if count[r] != 0 or not hits[r, 0]["flags"] & 3:
                    return "%s: the reference has no result, got count %d flags %d" % (tag, count[r], hits[r, 0]["flags"])
                if paths and not np.all(spans[r] == -1):
                    return "%s: spans without a path" % tag
                continue
            if count[r] != len(w):
                return "%s: %d hits, want %d (first wanted %s)" % (tag, count[r], len(w), [_first(h) for h in w[:3]])
            for k, h in enumerate(w):
                dist, start, end = _first(h)
                g = hits[r, k]
                if (int(g["start"]), int(g["end"])) != (start, end) or \
                        np.float64(g["dist"]).tobytes() != np.float64(dist).tobytes():
                    return "%s hit %d: got (%r, %d, %d) want (%r, %d, %d)" % (tag, k, float(g["dist"]), g["start"],
                                                                              g["end"], dist, start, end)
                if paths and not (spans[r, k].dtype == np.int32 and np.array_equal(spans[r, k], h[1])):
                    i = int(np.argwhere(spans[r, k] != h[1])[0][0])
                    return "%s hit %d (%d, %d): spans differ from motif point %d: got %s want %s" % (
                        tag, k, start, end, i, spans[r, k][i:i + 3].tolist(), h[1][i:i + 3].tolist())
            rest = hits[r, count[r]:]
            if not (np.all(np.isnan(rest["dist"])) and np.all(rest["start"] == -1) and np.all(rest["end"] == -1)):
                return "%s: unused slots are not (NaN, -1, -1)" % tag
            if paths and not np.all(spans[r, count[r]:] == -1):
                return "%s: spans in unused slots" % tag
    return None


diff_paths = diff_hits


# ======================================================================================================================
# pull
# ======================================================================================================================
PULL_T = 64 * 4                                  # sk_pull.hip: PULL_T = SK_WAVE * PULL_S samples per tile
PULL_TOK_MAX = 18                                # "-" + 13 digits + "." + 2 decimals + separator
PULL_K_LIMIT = 1e15                              # |k| = |rint((d + offset) * unit * 100)| at or past this: refused
PULL_ALIGN = 16                                  # k_pull_write: LDS image at dst & 15, 16-byte body stores
PULL_LENS = (0, 1, 3, 4, 5, PULL_T - 1, PULL_T, PULL_T + 1, 2 * PULL_T - 1, 2 * PULL_T, 2 * PULL_T + 1)
PULL_PREFIX_MAX = 40


def draw_pull(rng):
    R = int(_pick(rng, (1, 5, 17, 40, 90)))
    lens = np.array([int(_pick(rng, PULL_LENS)) if rng.random() < 0.6 else int(rng.integers(0, 1400)) for _ in range(R)],
                    dtype=np.int32)
    stride = max(8, int(lens.max()) + int(rng.integers(0, 30)))
    rows = rng.integers(-2000, 3000, size=(R, stride)).astype(np.int16)
    raw = bool(rng.random() < 0.3)
    calib = np.empty((R, 3))
    kinds = []
    for r in range(R):
        kind = _pick(rng, ("normal", "normal", "tiny", "huge", "full"))
        n = int(lens[r])
        dig = float(_pick(rng, (8192.0, 2048.0, 4096.0)))
        ofs = float(_pick(rng, (16.0, -16.0, 0.0, 7.25, -250.5, np.round(rng.uniform(-40, 40), 1))))
        rg = float(rng.uniform(20, 2000))
        if kind == "full":                                           # the whole int16 range
            rows[r] = rng.integers(-32768, 32768, size=stride).astype(np.int16)
        elif kind == "tiny":                                         # "%.2f" % range is 0.00 .. 0.02: 0.0 and -0.0
            rg = float(rng.uniform(0.0, 0.024))
        elif kind == "huge" and n:
            # tokens of PULL_TOK_MAX - 1 characters: |k| just under PULL_K_LIMIT at the row's largest |d + offset|,
            # with samples whose d + offset is 0 ("0.0") beside them; integer offsets so that the zero is exact
            ofs = float(_pick(rng, (16.0, -16.0, 250.0, -250.0)))
            rows[r] = rng.integers(-32768, 32768, size=stride).astype(np.int16)
            at = rng.integers(0, n, max(1, n // 3))
            rows[r, at] = int(-ofs)
            rows[r, at[: max(1, len(at) // 2)] - (1 if n > 1 else 0)] = int(_pick(rng, (-32768, -32000, 32767)))
            top = float(np.max(np.abs(rows[r, :n].astype(np.float64) + ofs)))
            rg = float("%.2f" % rng.uniform(20, 2000))
            unit = 0.99 * PULL_K_LIMIT / 100.0 / max(top, 1.0)       # 1 % under the limit: no rounding reaches it
            dig = rg / unit
        calib[r] = (dig, ofs, rg)
        kinds.append(kind)
    alphabet = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789_-./\t", dtype=np.uint8)
    prefixes = [bytes(rng.choice(alphabet, size=int(rng.integers(0, PULL_PREFIX_MAX + 1))).astype(np.uint8))
                for _ in range(R)]
    return dict(family="pull", R=R, raw=raw, entry=_pick(rng, ("host", "host", "dev")), stride=stride, rows=rows, lens=lens,
                calib=calib, prefixes=prefixes, kinds="".join(k[0] for k in kinds), env={})


def expect_pull(ora, case):
    from test_squigglepull import numpy_pull_text
    with np.errstate(all="ignore"):
        return dict(text=numpy_pull_text(case["rows"], case["lens"], case["prefixes"], calib=case["calib"], raw=case["raw"]))


def call_pull(api, case, exp=None):
    if case["entry"] == "host":
        return api.pull_text(case["rows"], case["lens"], case["prefixes"], calib=case["calib"], raw=case["raw"])
    # the device entry point, as test_squigglepull.test_host_and_dev_entry_points_and_overflow drives it
    import ctypes as C
    from squigglekit_amd import _lib
    L = _lib.ensure_init()
    ptr = _lib.ptr
    rows, lens, R = np.ascontiguousarray(case["rows"]), case["lens"], case["R"]
    blob, poff = api.pack_prefixes(case["prefixes"])
    pbuf = np.frombuffer(blob, dtype=np.uint8) if len(blob) else np.zeros(1, dtype=np.uint8)
    cap = len(blob) + PULL_TOK_MAX * int(lens.sum()) + R + 1
    mode = _lib.SK_PULL_RAW if case["raw"] else _lib.SK_PULL_PA
    cal2 = np.zeros((R, 2))
    _lib.check(L.sk_pa_calib(ptr(np.ascontiguousarray(case["calib"])), R, ptr(cal2)))
    line_off = np.zeros(R + 1, dtype=np.int64)
    arrays = dict(rows=rows, lens=lens, cal=cal2, pre=pbuf, poff=poff, off=line_off)
    d = {k: L.sk_dev_alloc(max(a.nbytes, 8)) for k, a in arrays.items()}
    d_text = L.sk_dev_alloc(cap + 64)
    try:
        for k in ("rows", "lens", "cal", "pre", "poff"):
            _lib.check(L.sk_dev_upload(d[k], ptr(arrays[k]), arrays[k].nbytes))
        fill = np.full(cap + 64, 0x5A, dtype=np.uint8)
        _lib.check(L.sk_dev_upload(d_text, ptr(fill), fill.nbytes))
        total = C.c_int64(-1)
        _lib.check(L.sk_pull_text_dev(d["rows"], case["stride"], d["lens"], R, None if case["raw"] else d["cal"], mode,
                                      d["pre"], d["poff"], d_text, cap, C.byref(total), d["off"]))
        _lib.check(L.sk_sync())
        back = np.zeros(cap + 64, dtype=np.uint8)
        _lib.check(L.sk_dev_download(ptr(back), d_text, back.nbytes))
        if not 0 <= total.value <= cap or not np.all(back[total.value:] == 0x5A):
            return b"<bytes written past the reported total %d>" % total.value
        return back[:total.value].tobytes()
    finally:
        for p in list(d.values()) + [d_text]:
            L.sk_dev_free(C.c_void_p(p) if isinstance(p, int) else p)


def diff_pull(case, got, exp):
    want = exp["text"]
    if bytes(got) == want:
        return None
    g, w = bytes(got).split(b"\n"), want.split(b"\n")
    for i in range(min(len(g), len(w))):
        if g[i] != w[i]:
            at = next((k for k in range(min(len(g[i]), len(w[i]))) if g[i][k] != w[i][k]), min(len(g[i]), len(w[i])))
            return "%d vs %d bytes, line %d (prefix %d bytes, %d samples, calib %s) differs at byte %d: got %r want %r" % (
                len(got), len(want), i, len(case["prefixes"][i]) if i < case["R"] else -1,
                int(case["lens"][i]) if i < case["R"] else -1, case["calib"][i].tolist() if i < case["R"] else None, at,
                g[i][max(0, at - 12):at + 24], w[i][max(0, at - 12):at + 24])
    return "%d vs %d lines" % (len(g), len(w))


# ======================================================================================================================
# the older single-set calls, for the interleaved sequence only
# ======================================================================================================================
def draw_plain(rng, kind):
    """kind: 'segment' (api.segment_batch), 'motifseq' (api.motifseq_batch), 'pa' (api.segment_batch_pa)."""
    from squigglekit_amd import synth
    R = int(_pick(rng, (3, 40, 300)))
    M = int(_pick(rng, (512, 2047, 4000, 6000)))
    motif = synth.synthetic_motif(int(_pick(rng, (17, 100, 200))), seed=int(rng.integers(1000)))
    sig = synth.squiggle_batch(R, M, int(rng.integers(1 << 30)), motif=motif if kind == "motifseq" else None)
    lens = rng.integers(0, M + 1, R).astype(np.int32)
    lens[int(rng.integers(R))] = M
    case = dict(family=kind, R=R, M=M, sig=sig, lens=lens, env={})
    if kind == "motifseq":
        case.update(motifs=[motif], scale=_pick(rng, ("medmad", "zscale")))
    elif kind == "pa":
        cal = np.empty((R, 3))
        cal[:, 0] = rng.choice([8192.0, 2048.0], R)
        cal[:, 1] = np.round(rng.uniform(-40, 40, R), 1)
        cal[:, 2] = rng.uniform(600, 1600, R)
        case["calib"] = cal
    return case


def expect_plain(ora, case):
    sig, lens = case["sig"], case["lens"]
    if case["family"] == "segment":
        return dict(zip(("segs", "nsegs"), ora.segment_batch_i16(sig, lens, max_segs=64)))
    if case["family"] == "motifseq":
        return dict(hits=ora.motifseq_batch_i16(sig, lens, case["motifs"][0], scale_mode=0 if case["scale"] == "medmad" else 1))
    out = []
    for r in range(case["R"]):
        dig, ofs, rg = case["calib"][r]
        pa = np.round((sig[r, :lens[r]].astype(np.int64) + ofs) * (float("{0:.2f}".format(rg)) / dig), 2)
        f = ora.scale_outliers(pa, 0, 900)
        out.append((ora.get_segs(f) or []) if f.size else [])
    return dict(segs=out)


def call_plain(api, case, exp=None):
    if case["family"] == "segment":
        return api.segment_batch(case["sig"], case["lens"], max_segs=64)
    if case["family"] == "motifseq":
        return api.motifseq_batch(case["sig"], case["lens"], case["motifs"][0], scale=case["scale"])
    return api.segment_batch_pa(case["sig"], case["lens"], case["calib"])


def diff_plain(case, got, exp):
    if case["family"] == "motifseq":
        want = exp["hits"]
        ok = ((got["flags"] & 2) == 0) & np.isfinite(want["dist"]) | (want["n"] == 0)      # MAD == 0 / std == 0 rows aside
        same = (got["start"] == want["start"]) & (got["end"] == want["end"]) & (got["n"] == want["n"]) & \
               ((got["dist"] == want["dist"]) | (np.isnan(got["dist"]) & np.isnan(want["dist"])))
        bad = np.flatnonzero(~same & ok)
        return None if not bad.size else "read %d: got %s want %s" % (bad[0], got[bad[0]], want[bad[0]])
    segs, nsegs = got
    for r in range(case["R"]):
        w = exp["segs"][r][:exp["nsegs"][r]].tolist() if case["family"] == "segment" else exp["segs"][r]
        if segs[r, :nsegs[r]].tolist() != w:
            return "read %d (%d samples): got %s want %s" % (r, case["lens"][r], segs[r, :nsegs[r]].tolist()[:3], w[:3])
    return None


def result_bytes(got):
    """A call's whole result as bytes (two calls with the same arguments must give the same ones)."""
    if isinstance(got, (bytes, bytearray, memoryview)):
        return bytes(got)
    if isinstance(got, np.ndarray):
        return got.tobytes()
    if got is None:
        return b""
    return b"|".join(result_bytes(g) for g in got)


DRAW = dict(sweep=draw_sweep, hits=draw_hits, paths=draw_paths, pull=draw_pull)
EXPECT = dict(sweep=expect_sweep, hits=expect_hits, paths=expect_paths, pull=expect_pull, segment=expect_plain,
              motifseq=expect_plain, pa=expect_plain)
CALL = dict(sweep=call_sweep, hits=call_hits, paths=call_paths, pull=call_pull, segment=call_plain, motifseq=call_plain,
            pa=call_plain)
DIFF = dict(sweep=diff_sweep, hits=diff_hits, paths=diff_paths, pull=diff_pull, segment=diff_plain, motifseq=diff_plain,
            pa=diff_plain)

# ---- the interleaved sequence (tests/test_gpu_random.py::test_interleaved_calls_share_the_context_buffers) --------
# (family, seed): committed cases by their seeds, the older calls by draw_plain seeds.  Filled beside SEEDS.
INTERLEAVE = [("paths", 50), ("sweep", 97), ("pull", 0), ("hits", 1), ("paths", 50), ("segment", 3), ("sweep", 22),
              ("motifseq", 2), ("pull", 21), ("paths", 12), ("pa", 3), ("hits", 324), ("sweep", 16), ("pull", 0),
              ("motifseq", 0), ("paths", 187), ("hits", 1), ("segment", 0), ("sweep", 97), ("paths", 29), ("pull", 3),
              ("pa", 2), ("hits", 214), ("sweep", 60), ("paths", 12), ("motifseq", 2)]


def interleave_case(family, seed):
    if family in SEEDS:
        return case_of(family, seed)
    case = draw_plain(np.random.default_rng([99, ["segment", "motifseq", "pa"].index(family), int(seed)]), family)
    case["seed"] = int(seed)
    return case
