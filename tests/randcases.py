"""Seeded random cases for the kernel files that have no other randomised test in the suite -- csrc/sk_sweep.hip,
sk_hits.hip, sk_path.hip, sk_pull.hip, sk_panel.hip, sk_detect.hip, sk_hmm.hip, sk_seglev.hip, through the twins of the
hit family sk_bg.hip and sk_events.hip, for the switches of the screening scheme sk_sdtwq.hip, and for both branches of the
dRNA segmenter (sk_drna_walk.hip and the dRNA kernels of sk_prep.hip), for DTW over a pair list with its warping paths
(sk_pairs.hip, sk_pairpath.hip), for the adaptive-band DTW (sk_band.hip), and for the signal HMM's posteriors
(sk_hmm_post.hip; their cases also feed filtered HMM sessions, sk_hmmstream.hip): per family
draw_<family>(rng) -> case,  expect_<family>(ora, case) ->
what the reference says,  call_<family>(api, case, exp) -> what the GPU says,  diff_<family>(case, got, exp) -> None or
the first difference as text.

A plain module: not collected, no conftest, pure numpy, no GPU import at module level (`api` is handed in).  The same
seed gives the same case on any machine: draw_* take a numpy.random.Generator and nothing else.  Used by
tests/test_random_cases.py (CPU: the committed seeds reach what they claim), tests/test_gpu_random.py (GPU: every seed
against its reference, plus six interleaved sequences) and tools/fuzz_gpu.py (open-ended: every draw it makes of these
families is DRAW[family] with its running generator).  tests/RANDOM_CASES.md says what each family draws, the
references, the budgets, the wall times, and which one-line kernel mutants the committed seeds catch
(tests/RANDOM_CASES_BAND.md for the band family, tests/RANDOM_CASES_HMMPOST.md for the posteriors).

The references are the statements that already exist: the oracle's scale_outliers + get_segs per (set, read) for the
sweep, reference_hits (test_hits_host.py), reference_paths (test_paths_host.py), numpy_pull_text (test_squigglepull.py),
reference_panel (test_panel_host.py), detect_ref.py, hmm_ref.py, hmm_path_ref.py, plain numpy on the oracle's segments
for the levels, reference_background_reads (test_background_host.py), reference_batch / reference_pool
(test_events_host.py), the oracle's scale_outliers + drna_segs / drna_roll per read for the dRNA branches,
pairs_ref.records and pair_paths_ref.list_spans for the pair lists, band_ref.records for the band,
hmm_post_ref.posterior_batch / posterior_reads for the posteriors.  Every comparison
is exact: integers as integers, doubles and text byte for byte.
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
    "panel": [4, 6, 8, 25, 29, 36, 66, 93, 94],
    "detect": [4, 6, 8, 10, 27, 44],
    "hmm": [3, 10, 11, 15, 21, 35, 39, 54],
    "levels": [13, 18, 22, 26, 42, 59],
    "screen": [67, 106, 119, 157, 238, 268, 281, 333, 337, 383, 387],
    "drna": [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 14, 15, 17, 18, 20, 22, 24, 27, 28, 29, 30, 31, 34, 35, 36, 37, 38, 39, 40,
             54, 56, 65, 66, 74, 116, 117, 140, 170, 210],
    "roll": [0, 1, 2, 3, 4, 10, 11, 13, 16, 21, 23, 24, 29, 31, 59],
    "pairs": [4, 5, 7, 9, 23, 54, 119, 130, 133],
    "pairpaths": [1, 5, 6, 7, 13, 17, 21, 22, 23, 36, 50, 145],
    "band": [27, 29, 44, 54, 61, 70, 75, 112, 138, 195, 238, 240, 297, 299, 331, 351, 423, 458],
    "hmmpost": [2, 8, 21, 22, 31, 34, 37, 48, 68, 77, 124, 137, 148, 162, 185, 215, 217, 239, 305, 339, 427, 465],
}

# every tuning switch a case may set; a runner clears the ones a case does not name
SWITCHES = ("SK_SEG_DELTA_SCALE", "SK_WALK_GENERAL", "SK_DTW_SMALL_MAX", "SK_HITS_ROW_BYTES", "SK_PATH_LDS_BYTES",
            "SK_PATH_SCRATCH_BYTES", "SK_DTW_NO_SMALL", "SK_PANEL_EXACT", "SK_HMM_SCRATCH_MB", "SK_INGEST_MB",
            "SK_DTW_QL", "SK_DTW_HINT_MIN", "SK_DTW_NOHINT", "SK_DTW_CK", "SK_DTW_SORT_MIN", "SK_DTW_SCRATCH_MB",
            "SK_DTW_NOFUSE", "SK_DTW_NO_SIBLINGS", "SK_DTW_NO_EARLY", "SK_DRNA_STEP", "SK_ROLL_ONE_LOOK",
            "SK_ROLL_DELTA_SCALE", "SK_ROLL_TWO_KERNELS", "SK_HMM_POST_BLOCK", "SK_BAND_WAVES")


# the family's number in the seed of its generator.  Frozen: the first four are what sorted(SEEDS).index(family) gave when
# the table held four keys, so those cases stay what they were (tests/test_random_cases.py pins their digests); a new
# family takes the next free number, whatever its name.
FAMILY_INDEX = dict(hits=0, paths=1, pull=2, sweep=3, panel=4, detect=5, hmm=6, levels=7, screen=8, drna=9, roll=10,
                    pairs=11, pairpaths=12, band=13, hmmpost=14)


def rng_of(family, seed):
    """The generator of a committed case: the family is part of the seed, so the lists do not share streams."""
    return np.random.default_rng([FAMILY_INDEX[family], int(seed)])


def case_of(family, seed):
    case = DRAW[family](rng_of(family, seed))
    case["seed"] = int(seed)
    return case


def _pick(rng, values):
    return values[int(rng.integers(len(values)))]


# what a case holds besides its drawn parameters: the arrays (describe leaves them out, case_digest hashes them)
ARRAY_KEYS = ("reads", "rows", "sets", "motifs", "prefixes", "calib", "lens", "sig", "win", "means", "sds", "model", "cal",
              "use", "seqs", "pairs")


def _plain(v):
    if isinstance(v, (np.integer,)):
        return int(v)
    if isinstance(v, (np.floating,)):
        return float(v)
    return v


def describe(case):
    """Everything needed to reproduce a case, on one line."""
    keys = [k for k in case if k not in ARRAY_KEYS]
    return "%s seed=%s %s env=%s" % (case["family"], case.get("seed"),
                                     " ".join("%s=%s" % (k, _plain(case[k])) for k in keys
                                              if k not in ("family", "seed", "env")), case["env"])


def _digest_into(h, v):
    if isinstance(v, np.ndarray):
        h.update(("%s%s" % (v.dtype.str, v.shape)).encode())
        h.update(np.ascontiguousarray(v).tobytes())
    elif isinstance(v, (bytes, bytearray)):
        h.update(b"b%d:" % len(v) + bytes(v))
    elif isinstance(v, dict):
        for k in sorted(v):
            h.update(("{%s}" % k).encode())
            _digest_into(h, v[k])
    elif isinstance(v, (list, tuple)):
        h.update(b"[%d]" % len(v))
        for x in v:
            _digest_into(h, x)
    else:
        h.update(repr(_plain(v)).encode())


def case_digest(case):
    """sha256 over describe(case) and every array the case holds (dtype, shape, bytes): two cases with the same digest
    are the same input on any machine."""
    import hashlib
    h = hashlib.sha256(describe(case).encode())
    for k in sorted(k for k in case if k in ARRAY_KEYS):
        h.update(("<%s>" % k).encode())
        _digest_into(h, case[k])
    return h.hexdigest()


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
# panel
# ======================================================================================================================
# sk_panel_plan gives a motif of N points L lanes and R rows per lane: beyond 1 024 points the chained launcher; up to 256
# points L = 16, R = ceil(N / 16) -- unless the call is "small" (reads * motifs <= SK_DTW_SMALL_MAX = 2 048, and no
# SK_DTW_NO_SMALL) and N >= 32; everything else L = 64, R = ceil(N / 64).  P = L * R - N lanes hold one row fewer.
PANEL_N = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
PANEL_K = (1, 2, 3, 12, 64, 256)                 # 256: the ABI's limit
PANEL_CELLS = 120_000_000                        # cost-matrix cells the oracle fills per case (about 1 s, see RANDOM_CASES.md)
PANEL_LIMITS = (0, 1200)                         # test_panel_host.oracle_records' limits
INT32_MAX = 2 ** 31 - 1


def panel_shape(N, pairs, env):
    """(L, R) as sk_panel_plan picks them for a motif of N points in a call of `pairs` (read, motif) pairs; None: the
    chained launcher."""
    if N > 64 * 16:
        return None
    small_max = 2048
    if "SK_DTW_SMALL_MAX" in env and int(env["SK_DTW_SMALL_MAX"]) >= 0:
        small_max = int(env["SK_DTW_SMALL_MAX"])
    spread = pairs <= small_max and "SK_DTW_NO_SMALL" not in env
    if N <= 256 and not (spread and N >= 32):
        return 16, (N + 15) // 16
    return 64, (N + 63) // 64


def _is_int_read(r):
    r = np.asarray(r)
    return r.dtype.kind in "iu" or r.size == 0 or bool(np.all(np.isfinite(r)) and np.all(r == np.rint(r)))


def panel_calls(case):
    """Reads per C call: the list form splits into the integer-valued reads and the rest."""
    if case["route"] != "list":
        return [case["nreads"]]
    n = sum(_is_int_read(r) for r in case["reads"])
    return [v for v in (n, case["nreads"] - n) if v]


def panel_groups(case):
    """[{(L, R) or None: [motif indices]}] per C call of the case."""
    out = []
    for R in panel_calls(case):
        g = {}
        for k, m in enumerate(case["motifs"]):
            g.setdefault(panel_shape(len(m), R * len(case["motifs"]), case["env"]), []).append(k)
        out.append(g)
    return out


def panel_windows(case):
    """(begin, length) of every read's window, as Python slices it."""
    out = []
    for r, raw in enumerate(case["reads"]):
        a, b = (int(case["win"][r][0]), int(case["win"][r][1])) if case["win"] is not None else case["region"]
        lo, hi, _ = slice(a, b).indices(len(raw))
        out.append((lo, max(0, hi - lo)))
    return out


def panel_screened(case):
    """sk_launch_panel_dtw hands a group to the screening path: 256 reads or more and a longest window of at least
    4 * (N0 + N0 / 8 + 136) samples, N0 the group's first motif."""
    if "SK_PANEL_EXACT" in case["env"] or min(panel_calls(case)) < 256:
        return False
    longest = max(w for _, w in panel_windows(case))
    return any(shape is not None and longest >= 4 * (len(case["motifs"][ks[0]]) + len(case["motifs"][ks[0]]) // 8 + 136)
               for g in panel_groups(case) for shape, ks in g.items())


def _panel_len_for(kind, a, c, E, w):
    """A read length whose window under the region kind has w samples (w <= E)."""
    return {"head": w, "tail": w, "mid": a + w, "negend": a + c + w}[kind]


def _panel_region(kind, a, c, E):
    return {"head": (0, E), "tail": (-E, None), "mid": (a, a + E), "negend": (a, -c), "empty": (a + E, a + E - c),
            "beyond": (20000, 20000 + E)}[kind]


def draw_panel(rng):
    from squigglekit_amd import synth
    env = {}
    screen = rng.random() < 0.12                  # 256 reads and windows long enough for the screening path
    batchlay = rng.random() < 0.5
    if batchlay:                                  # the layout big batches get: every motif of up to 256 points on L = 16
        env["SK_DTW_SMALL_MAX"] = "0"
        env["SK_DTW_NO_SMALL"] = "1"
    K = int(_pick(rng, PANEL_K[:3])) if screen else int(_pick(rng, PANEL_K if batchlay else PANEL_K[:4]))
    # ---- motif lengths: the listed ones, (L, R, P) triples made on purpose, random ones; for big panels mostly short
    def one_n(short):
        u = rng.random()
        if short:
            return int(rng.integers(1, 49))
        if u < 0.4:
            return int(_pick(rng, PANEL_N))
        if u < 0.8:
            L = int(_pick(rng, (16, 64)))
            return max(1, L * int(rng.integers(1, 17)) - int(_pick(rng, (0, 1, L - 1, int(rng.integers(0, L))))))
        return int(rng.integers(1, 300))
    if screen:
        Ns = [16] + [int(rng.integers(1, 25)) for _ in range(K - 1)]
    else:
        Ns = [one_n(k >= 6) for k in range(K)]
        if K >= 12 and rng.random() < 0.6:       # a ladder: up to 16 different R of one L in one call
            L = 16 if batchlay and rng.random() < 0.6 else 64
            for k, r in enumerate(rng.permutation(16)[:min(K, 16)] + 1):
                Ns[k] = max(1, L * int(r) - int(_pick(rng, (0, 1, L - 1, int(rng.integers(0, L))))))
        elif K >= 3 and rng.random() < 0.6:      # three groups or more with several members each, and a long motif
            base = [int(_pick(rng, (5, 16, 20, 40, 48)))]
            base += [base[0] + 16, base[0] + 40]
            for k in range(K):
                if k >= 1 and rng.random() < 0.7:
                    Ns[k] = base[k % 3] - int(rng.integers(0, 3))
            Ns[int(rng.integers(1, K))] = int(rng.integers(1025, 1101))
    motifs = [synth.synthetic_motif(N, seed=int(rng.integers(1000))) for N in Ns]
    twins = None
    if K >= 2 and rng.random() < 0.6:            # two identical motifs (same length: same mean and sd): score ties
        i, j = (int(v) for v in rng.choice(K, 2, replace=False))
        if screen and j == 0:                     # (the screening case keeps its 16-point first motif)
            i, j = j, i
        if Ns[i] <= 1024:
            motifs[j], Ns[j], twins = motifs[i].copy(), Ns[i], (min(i, j), max(i, j))
    order = np.arange(K) if screen else rng.permutation(K)       # groups interleaved in motif order
    motifs, Ns = [motifs[int(i)] for i in order], [Ns[int(i)] for i in order]
    if twins:
        inv = np.argsort(order)
        twins = tuple(sorted(int(inv[t]) for t in twins))
    N0 = Ns[0]
    route = "batch" if screen else _pick(rng, ("batch", "batch", "f64", "list"))
    scale = _pick(rng, ("medmad", "medmad", "zscale"))
    # ---- a tie between `left` and `diag` that moves `start`: a motif that begins with z points of exactly 0.0, and (below)
    # a three-level read with a run of more than z samples at its median -- medmad makes them exactly 0.0, so the first z
    # rows cost nothing along the run, every cell there ties, and the tie order decides where the hit starts
    plateau = None
    if not screen and scale == "medmad" and rng.random() < 0.5:
        free = [k for k in range(K) if not twins or k not in twins]
        if free:
            z = int(_pick(rng, (2, 3, 5)))
            plateau = (int(_pick(rng, free)), z)
            motifs[plateau[0]] = np.array([0.0] * z + [1.0 / 1.4826] * 2)
            Ns[plateau[0]] = z + 2
            N0 = Ns[0]
    # ---- the region
    E = int(_pick(rng, (700, 760))) if screen else int(_pick(rng, (120, 300, 700, 2000)))
    a, c = int(_pick(rng, (5, 100, 333))), int(_pick(rng, (1, 50)))
    kind = _pick(rng, ("head", "tail")) if screen else _pick(rng, ("head", "tail", "mid", "negend", "win", "win", "rare"))
    if kind == "rare":
        kind = _pick(rng, ("empty", "beyond"))
    # ---- window sizes: the listed ones around the first motif's N and L, then random
    sumN = sum(Ns)
    room = max(1, PANEL_CELLS // max(1, sumN) - (121 if plateau else 0))     # window samples the reference can afford
    L0 = (panel_shape(N0, 10 ** 9 if batchlay else 1, env) or (64, 16))[0]
    if screen:
        wins = [int(rng.integers(640, E + 1)) for _ in range(256 + int(rng.integers(0, 9)))]
        wins[:3] = [0, 9, 40]
    else:
        wins = [w for w in (0, 7, 8, 9, N0 - 1, N0, N0 + 1, L0 - 1, L0, L0 + 1, 2 * L0 + 1) if 0 <= w <= E]
        if rng.random() < 0.4:
            wins.append(1)                        # (one sample: MAD 0, only its flag is compared)
        wins = list(dict.fromkeys(wins))
        cap = max(12, 2048 // K if not batchlay else 400)
        more = int(_pick(rng, (8, 30, 60)))
        for _ in range(more):
            w = int(rng.integers(16, E + E // 2))
            if len(wins) < cap and sum(wins) + w <= room:
                wins.append(w)
        while sum(wins) > room and len(wins) > 1:    # (many long motifs: the listed windows alone are too much)
            wins.remove(max(wins))
    if plateau:
        wins.append(int(rng.integers(100, 121)))
    nspecial = sum(w == 1 for w in wins)
    # ---- the reads
    plant = [m for m in motifs if len(m) <= 300][:3]
    reads, kinds, rows_kind = [], [], []
    for w in wins:
        rk = kind if kind != "win" else _pick(rng, ("head", "tail", "mid", "negend"))
        if rk in ("empty", "beyond"):
            n = w + int(rng.integers(0, 200))
        else:
            n = _panel_len_for(rk, a, c, E, w) if w <= E else w + a + c
        k = "squiggle" if w < 16 else _pick(rng, ("squiggle", "squiggle", "ties", "dropped"))
        if plateau and len(reads) == len(wins) - 1:                        # the read with the run at its median
            step = int(_pick(rng, (1, 10)))
            x = (480 + step * rng.integers(0, 3, size=n)).astype(np.int16)
            b, e = _panel_region(rk, a, c, E)
            lo, hi, _ = slice(b, e).indices(n)
            run = [480 + step] * (plateau[1] + int(rng.integers(3, 8))) + [480 + 2 * step] * 2
            if hi - lo > len(run):                                         # (an empty region: nothing to plant in)
                at = lo + int(rng.integers(0, hi - lo - len(run)))
                x[at:at + len(run)] = run
            reads.append(x)
            kinds.append("z")
            rows_kind.append(rk)
            continue
        reads.append(_hit_read(rng, n, plant, k))
        kinds.append(k[0])
        rows_kind.append(rk)
    def add(read, tag):
        reads.append(read)
        kinds.append(tag)
        rows_kind.append(kind if kind != "win" else "head")
    if len(reads) >= 10 * (nspecial + 1) + 1 and rng.random() < 0.6:
        add(np.full(a + c + int(rng.integers(40, E + 40)), 500, dtype=np.int16), "m")           # MAD 0 in any window
        nspecial += 1
    if rng.random() < 0.5:
        add(np.full(a + c + int(rng.integers(2, 300)), 2000, dtype=np.int16), "e")              # nothing inside the limits
    while len(reads) <= 10 * nspecial:            # (the reads whose distance is not compared stay under a tenth)
        w = int(rng.integers(16, 40))
        add(_hit_read(rng, w + (a + c if kind in ("mid", "negend") else 0), plant, "squiggle"), "s")
    order = rng.permutation(len(reads))
    reads, rows_kind = [reads[int(i)] for i in order], [rows_kind[int(i)] for i in order]
    kinds = "".join(kinds[int(i)] for i in order)
    R = len(reads)
    win = None
    region = _panel_region(kind, a, c, E) if kind != "win" else (0, None)
    if kind == "win":
        win = np.zeros((R, 2), dtype=np.int32)
        for r in range(R):
            b, e = _panel_region(rows_kind[r], a, c, E)
            win[r] = (b, INT32_MAX if e is None else e)
            if rows_kind[r] == "negend" and len(reads[r]) < a + c:       # (begin behind end, one side cut: refused)
                win[r] = (0, E)
        win[int(rng.integers(R))] = (10 ** 6, -10 ** 6)                   # both ends cut to the read: an empty window
    # ---- the routes
    nfloat = 0
    if route in ("f64", "list"):
        dig, ofs, rg = _pick(rng, ((8192.0, 16.0, 1493.94), (2048.0, -3.0, 748.58), (8192.0, 7.25, 1467.61)))
        for r in range(R):
            if route == "f64" or (rng.random() < 0.5 and len(reads[r])):
                x = np.round((reads[r].astype(np.int64) + ofs) * (rg / dig), 2)
                if kinds[r] == "e":
                    x[:] = 1500.25
                if x.size:
                    x[0] += 0.005                                         # (never integer-valued as a whole)
                reads[r] = x
                nfloat += 1
    longest = max(len(r) for r in reads)
    case = dict(family="panel", route=route, scale=scale, K=K, Ns=Ns, twins=twins, plateau=plateau, kind=kind, region=region, E=E,
                screen=screen, motifs=motifs, reads=reads, nreads=R, nfloat=nfloat, nspecial=nspecial, longest=longest,
                kinds=kinds, win=win, env=env)
    if route == "batch":
        stride = (longest + 8 + int(rng.integers(0, 64))) // 8 * 8       # stride > the longest row
        sig = rng.integers(300, 700, size=(R, stride)).astype(np.int16)  # (padding is not zeros)
        for i, r in enumerate(reads):
            sig[i, :len(r)] = r
        case["sig"], case["lens"], case["stride"] = sig, np.array([len(r) for r in reads], dtype=np.int32), stride
    return case


def expect_panel(ora, case):
    from test_panel_host import model_terms, reference_panel
    mean, sd = model_terms(case["motifs"])
    ref = reference_panel(ora, case["reads"], case["motifs"], case["region"], case["win"], case["scale"])
    return dict(ref=ref, means=mean, sds=sd)


def call_panel(api, case, exp):
    kw = dict(region=case["region"], win=case["win"], scale=case["scale"], records=True)
    if case["route"] == "batch":
        return api.motifseq_panel_batch(case["sig"], case["lens"], case["motifs"], exp["means"], exp["sds"], **kw)
    if case["route"] == "f64":
        return api.motifseq_panel_ragged_f64(*api.pack_f64(case["reads"]), case["motifs"], exp["means"], exp["sds"], **kw)
    return api.motifseq_panel(case["reads"], case["motifs"], exp["means"], exp["sds"], **kw)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def diff_panel(case, got, exp):
    """What test_gpu_panel.same asserts, as text with the first differing (motif, read)."""
    panel, frm, allrec = got
    recs, flags, rfrm, best, second, sb, ss = exp["ref"]

    def first(bad):
        return int(np.flatnonzero(bad)[0])
    if not np.array_equal(frm, rfrm):
        r = first(frm != rfrm)
        return "read %d (%d samples): window from %d, want %d" % (r, len(case["reads"][r]), frm[r], rfrm[r])
    cmp = flags != 2
    for k, g in enumerate(allrec):
        w = recs[k]
        bad = (g["n"] != w["n"]) | ((g["flags"] & 3) != flags) | \
              (cmp & ((_bits(g["dist"]) != _bits(w["dist"])) | (g["start"] != w["start"]) | (g["end"] != w["end"])))
        if bad.any():
            r = first(bad)
            return "motif %d (N=%d, shape %s) read %d (%d samples, window %s): got %s want %s flags %d" % (
                k, len(case["motifs"][k]), panel_shape(len(case["motifs"][k]), case["nreads"] * case["K"], case["env"]), r,
                len(case["reads"][r]), panel_windows(case)[r], g[r], w[r], flags[r])
    bad = (panel["best"] != best) | (panel["second"] != second) | (_bits(panel["score_best"]) != _bits(sb)) | \
          (_bits(panel["score_second"]) != _bits(ss))
    if bad.any():
        r = first(bad)
        return "read %d: ranked (%d, %d) scores (%r, %r), want (%d, %d) (%r, %r)" % (
            r, panel["best"][r], panel["second"][r], float(panel["score_best"][r]), float(panel["score_second"][r]),
            best[r], second[r], float(sb[r]), float(ss[r]))
    for r in range(len(frm)):
        h = panel["hit"][r]
        if best[r] >= 0:
            if h.tobytes() != allrec[best[r]][r].tobytes():
                return "read %d: the panel's hit is not the best motif's record" % r
        elif not (np.isnan(h["dist"]) and h["start"] == -1 and h["end"] == -1 and h["n"] == recs[0]["n"][r]
                  and h["flags"] & 3 == flags[r]):
            return "read %d: unranked, but its hit is %s" % (r, h)
    return None


# ======================================================================================================================
# event detection
# ======================================================================================================================
# sk_detect.hip: k_detect_mark takes 64 reads a workgroup and gathers marks in 64-sample words; k_detect_fill walks a
# read in rounds of 4 096 samples, a lane per word; rows are loaded with 16-byte loads where the stride allows it.
DET_WORD = 64
DET_ROUND = 4096
DET_COUNTS = (1, 63, 64, 65, 130)
DET_LENS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097)
DET_LONG = 8192
DET_SAMPLES = 600_000                            # samples per case (the numpy reference: about 2 us each)
DET_PRESETS = {"dna": (3, 6, 1.4, 9.0, 0.2), "rna": (7, 14, 2.5, 9.0, 1.0)}


def _det_read(rng, n):
    """tools/fuzz_gpu.py's reads: levels with noise, anything an int16 holds, flat or two values."""
    kind = rng.random()
    if kind < 0.6:
        lv = np.repeat(rng.normal(500, 80, n // 3 + 1), rng.integers(1, 20, n // 3 + 1))[:n]
        x = lv + rng.normal(0, float(rng.choice([0, 2, 8, 30])), lv.size)
    elif kind < 0.8:
        x = rng.integers(-32768, 32768, n).astype(np.float64)
    else:
        x = np.where(rng.random(n) < float(rng.choice([0.0, 0.5])), 32767.0, float(rng.integers(-32768, 32767)))
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16), "lrf"[0 if kind < 0.6 else 1 if kind < 0.8 else 2]


def _ragged_lens(rng, R, seams, dmax, budget):
    lens = [int(_pick(rng, seams)) if rng.random() < 0.5 else int(rng.integers(0, dmax + 1)) for _ in range(R)]
    total = 0
    for i, n in enumerate(lens):                 # (the reference's CPU time)
        if total + n > budget:
            lens[i] = n = int(rng.integers(0, 70))
        total += n
    return lens


def _i16_rows(rng, reads, aligned, pad=-7):
    """(rows [R, stride], lens int32, stride): stride a multiple of 8 or not, padding not zeros."""
    longest = max([len(r) for r in reads] + [1])
    stride = (longest + 7 + 8 * int(rng.integers(0, 2))) // 8 * 8 if aligned else (longest + int(rng.integers(0, 9))) | 1
    buf = np.full((len(reads), stride), pad, dtype=np.int16)
    for r, x in enumerate(reads):
        buf[r, :len(x)] = x
    return buf, np.array([len(x) for x in reads], dtype=np.int32), stride


def draw_detect(rng):
    R = int(_pick(rng, DET_COUNTS))
    u = rng.random()
    if u < 0.25:
        params, pk = DET_PRESETS["dna"], "dna"
    elif u < 0.4:
        params, pk = DET_PRESETS["rna"], "rna"
    else:
        v = rng.random()
        ws = 1 if v < 0.2 else int(rng.integers(1, 65))
        wl = 64 if v < 0.35 else ws if v < 0.5 else int(rng.integers(ws, 65))
        params = (ws, wl, float(_pick(rng, (0.0, 1.4, 2.5, 20.0))), float(_pick(rng, (0.0, 4.0, 9.0))),
                  float(_pick(rng, (0.0, 0.2, 1.0, 5.0))))
        pk = "drawn"
    ws, wl = params[0], params[1]
    seams = DET_LENS + (2 * ws - 1, 2 * ws, 2 * ws + 1, 2 * wl - 1, 2 * wl, 2 * wl + 1)
    dmax = int(_pick(rng, (8, 70, 130, 300, 1500, 5000)))
    lens = _ragged_lens(rng, R, seams, dmax, DET_SAMPLES - 3 * DET_ROUND - 2 * DET_LONG)
    reads, kinds = [], ""
    for n in lens:
        x, k = _det_read(rng, n)
        reads.append(x)
        kinds += k
    long_read = flat_round = False
    if rng.random() < 0.5:                        # one read above DET_LONG samples
        at = int(rng.integers(R))
        reads[at], _ = _det_read(rng, int(rng.integers(DET_LONG + 1, DET_LONG + 3000)))
        long_read = True
    if rng.random() < 0.5:                        # a whole round of k_detect_fill without a mark, events on both sides
        at = int(rng.integers(R))
        n = 3 * DET_ROUND + int(rng.integers(0, 500))
        lv = np.repeat(rng.normal(500, 80, n // 3 + 1), rng.integers(3, 20, n // 3 + 1))[:n] + rng.normal(0, 2, n)
        lv[DET_ROUND - 130:2 * DET_ROUND + 130] = float(rng.integers(300, 700))
        reads[at] = np.rint(lv).astype(np.int16)
        kinds = kinds[:at] + "p" + kinds[at + 1:]
        flat_round = True
    aligned = bool(rng.random() < 0.5)
    buf, lens, stride = _i16_rows(rng, reads, aligned)
    return dict(family="detect", R=R, params=params, preset=pk, dmax=dmax, stride=stride, aligned=aligned,
                long_read=long_read, flat_round=flat_round, total=int(lens.sum()), kinds=kinds, sig=buf, lens=lens,
                reads=reads, env={})


def expect_detect(ora, case):
    import detect_ref
    off, rec = detect_ref.detect(case["reads"], case["params"])
    return dict(off=off, rec=rec)


def call_detect(api, case, exp=None):
    p = case["params"]
    return api.detect_events_batch(case["sig"], case["lens"], api.det_params(
        w_short=p[0], w_long=p[1], th_short=p[2], th_long=p[3], peak_height=p[4]))


def diff_detect(case, got, exp):
    off, rec = got
    if off.shape != exp["off"].shape:
        return "offsets shaped %s, want %s" % (off.shape, exp["off"].shape)
    if not np.array_equal(off, exp["off"]):
        r = int(np.flatnonzero(np.diff(off) != np.diff(exp["off"]))[0])
        return "read %d (%d samples): %d events, want %d" % (r, case["lens"][r], off[r + 1] - off[r],
                                                              exp["off"][r + 1] - exp["off"][r])
    if rec.tobytes() != exp["rec"].tobytes():
        q = int(np.flatnonzero(rec != exp["rec"])[0])
        r = int(np.searchsorted(off, q, side="right") - 1)
        return "read %d (%d samples) event %d: got %s want %s" % (r, case["lens"][r], q - off[r], rec[q], exp["rec"][q])
    return None


# ======================================================================================================================
# signal HMM: the record call and the segments call on the same case
# ======================================================================================================================
# sk_hmm.hip: 64 reads a wavefront; the segments call keeps back pointers, 256 bytes a sample and group of 64 reads, in
# slices of SK_HMM_SCRATCH_MB (1 MiB: a single group per slice once a read has more than 2 048 samples).
HMM_COUNTS = (1, 63, 64, 65, 130, 200)
HMM_LENS = (0, 1, 2, 31, 32, 33, 127, 128, 129, 255)
HMM_LIMITS = (0, 0, 1, 33, 129, 100000)
HMM_SAMPLES = 600_000


def hmm_slices(case):
    """Slices sk_launch_hmm_paths makes of the case's reads (per C call; the list form's larger call)."""
    budget = (int(case["env"]["SK_HMM_SCRATCH_MB"]) << 20) if "SK_HMM_SCRATCH_MB" in case["env"] else 16 << 30
    n = max([len(r) for r in case["reads"]] + [1])
    if case["limit"] > 0:
        n = min(n, case["limit"])
    nreads = case["R"] if case["feed"] != "list" else max(case["nfloat"], case["R"] - case["nfloat"])
    groups = (nreads + 63) // 64
    g = min(max(1, budget // (max(n, 1) * 256)), groups)
    return -(-groups // g) if groups else 0


def _draw_hmm_model(rng):
    """(model, S, integer): tools/fuzz_gpu.py's model -- S = 1 .. 6, integer scores (ties) in 30 % of the draws and logs of
    uniform draws otherwise, 30 % of linit and 40 % of ltrans -inf, half the states without a second component, 20 % of
    h zero.  draw_hmm and draw_hmmpost begin with it: the order of its draws is part of the pinned cases."""
    S = int(rng.integers(1, 7))
    integer = bool(rng.random() < 0.3)
    if integer:                                   # integer scores: ties
        hl, ht = rng.integers(-3, 1, S).astype(np.float64), rng.integers(-2, 1, (S, S)).astype(np.float64)
        hc = rng.integers(-2, 1, (S, 2)).astype(np.float64)
        hmu = rng.integers(-3, 4, (S, 2)).astype(np.float64) * 100 + 500
        hh = rng.integers(0, 2, (S, 2)).astype(np.float64)
    else:
        hl, ht = np.log(rng.uniform(0.01, 1, S)), np.log(rng.uniform(0.001, 1, (S, S)))
        hc = np.log(rng.uniform(0.01, 1, (S, 2)) / rng.uniform(2, 90, (S, 2)))
        hmu = rng.uniform(-200, 1200, (S, 2))
        hh = np.where(rng.random((S, 2)) < 0.2, 0.0, 1.0 / (2.0 * rng.uniform(2, 90, (S, 2)) ** 2))
    hl[rng.random(S) < 0.3] = -np.inf
    if not np.isfinite(hl).any():
        hl[int(rng.integers(S))] = 0.0
    ht[rng.random((S, S)) < 0.4] = -np.inf
    hc[rng.random(S) < 0.5, 1] = -np.inf
    return dict(nstates=S, linit=hl, ltrans=ht, c=hc, mu=hmu, h=hh), S, integer


def draw_hmm(rng):
    model, S, integer = _draw_hmm_model(rng)
    # ---- the reads
    env = {}
    R = int(_pick(rng, HMM_COUNTS))
    dmax = int(_pick(rng, (70, 300, 1500, 5000)))
    if rng.random() < 0.35:
        env["SK_HMM_SCRATCH_MB"] = "1"
    if rng.random() < 0.3:
        env["SK_INGEST_MB"] = "1"
    lens = _ragged_lens(rng, R, HMM_LENS, dmax, HMM_SAMPLES - 3000)
    limit = int(_pick(rng, HMM_LIMITS))
    if "SK_HMM_SCRATCH_MB" in env and R >= 130 and rng.random() < 0.7:
        lens[int(rng.integers(R))] = int(rng.integers(2100, 3000))        # 1 MiB then holds one group of 64 reads: a slice each
        limit = int(_pick(rng, (0, 100000)))
    reads = [_det_read(rng, n)[0] for n in lens]
    feed = _pick(rng, ("batch", "batch", "f64", "list"))
    cal, nfloat, aligned = None, 0, None
    case = dict(family="hmm", R=R, S=S, integer=integer, feed=feed, limit=limit, dmax=dmax)
    if feed == "batch":
        aligned = bool(rng.random() < 0.5)
        case["sig"], case["lens"], case["stride"] = _i16_rows(rng, reads, aligned)
        if rng.random() < 0.5:
            cal = np.stack([rng.uniform(-50, 50, R), rng.uniform(0.1, 0.3, R)], axis=1)
    else:
        for r in range(R):
            if len(reads[r]) and (feed == "f64" or rng.random() < 0.5):
                reads[r] = reads[r].astype(np.float64) * float(_pick(rng, (1.0, 0.25, 0.1))) + 0.37    # not integers
                nfloat += 1
    case.update(aligned=aligned, calibrated=cal is not None, nfloat=nfloat, total=int(sum(len(r) for r in reads)),
                model=model, cal=cal, reads=reads, env=env)
    return case


def hmm_model_of(api, case):
    m = case["model"]
    return api.HmmModel.from_arrays(m["nstates"], m["linit"], m["ltrans"], m["c"], m["mu"], m["h"])


def expect_hmm(ora, case):
    """rec: the records; parts: [(read indices, rec, off, seg)] per C call of the segments call."""
    import hmm_path_ref
    import hmm_ref
    model, limit, reads = case["model"], case["limit"], case["reads"]        # (the references take the plain arrays)
    if case["feed"] == "batch":
        rec = hmm_ref.viterbi_batch(model, case["sig"], case["lens"], case["cal"], limit)
        return dict(rec=rec, parts=[(list(range(case["R"])),) +
                                    hmm_path_ref.segments_batch(model, case["sig"], case["lens"], case["cal"], limit)])
    rec = hmm_ref.viterbi_reads(model, reads, limit)
    ints = [i for i, r in enumerate(reads) if _is_int_read(r)] if case["feed"] == "list" else []
    flts = [i for i in range(len(reads)) if i not in set(ints)]
    parts = []
    if ints:
        parts.append((ints,) + hmm_path_ref.segments_reads(model, [reads[i] for i in ints], limit, raw=True))
    if flts:
        parts.append((flts,) + hmm_path_ref.segments_reads(model, [reads[i] for i in flts], limit))
    return dict(rec=rec, parts=parts)


def call_hmm(api, case, exp=None):
    """(records of the record call, records of the segments call, [segments of read r])"""
    model, limit, reads = hmm_model_of(api, case), case["limit"], case["reads"]
    if case["feed"] == "batch":
        rec = api.hmm_viterbi_batch(case["sig"], case["lens"], model, case["cal"], limit)
        prec, off, seg = api.hmm_segments_batch(case["sig"], case["lens"], model, case["cal"], limit)
    elif case["feed"] == "f64":
        rec = api.hmm_viterbi_ragged_f64(*api.pack_f64(reads), model, limit)
        prec, off, seg = api.hmm_segments_ragged_f64(*api.pack_f64(reads), model, limit)
    else:
        rec = api.hmm_viterbi(reads, model, limit)
        prec, segs = api.hmm_segments(reads, model, limit)
        return rec, prec, segs
    return rec, prec, [seg[int(off[r]):int(off[r + 1])] for r in range(len(reads))]


def diff_hmm(case, got, exp):
    return diff_hmm_records(case, got, exp) or diff_hmm_paths(case, got, exp)


def diff_hmm_records(case, got, exp):
    """the record call against hmm_ref"""
    rec = got[0]
    if rec.tobytes() != exp["rec"].tobytes():
        r = int(np.flatnonzero(rec != exp["rec"])[0])
        return "record of read %d (%d samples): got %s want %s" % (r, len(case["reads"][r]), rec[r], exp["rec"][r])
    return None


def diff_hmm_paths(case, got, exp):
    """the segments call against hmm_path_ref, its records against the record call's"""
    rec, prec, segs = got
    if prec.tobytes() != rec.tobytes():
        r = int(np.flatnonzero(prec != rec)[0])
        return "read %d: the segments call's record %s is not the record call's %s" % (r, prec[r], rec[r])
    for idx, wrec, woff, wseg in exp["parts"]:
        for k, r in enumerate(idx):
            want = wseg[int(woff[k]):int(woff[k + 1])]
            g = segs[r]
            if g.dtype["sum"] == want.dtype["sum"] and g.tobytes() == want.tobytes():
                continue
            n = min(len(g), len(want))
            bad = np.flatnonzero(np.frombuffer(g[:n].tobytes(), dtype=np.uint8).reshape(n, -1) !=
                                 np.frombuffer(want[:n].tobytes(), dtype=np.uint8).reshape(n, -1)) if n and \
                g.dtype.itemsize == want.dtype.itemsize else np.zeros(0, dtype=np.int64)
            q = int(bad[0]) // g.dtype.itemsize if bad.size else n
            return "read %d (%d samples): %d segments (sums %s), want %d (%s); segment %d: got %s want %s" % (
                r, len(case["reads"][r]), len(g), g.dtype["sum"].base, len(want), want.dtype["sum"].base, q,
                g[q] if q < len(g) else None, want[q] if q < len(want) else None)
    return None


# ======================================================================================================================
# signal HMM posteriors (sk_hmm_post.hip: k_hmm_fwd<FEED>, k_hmm_bwd<FEED, COUNTS>; tests/RANDOM_CASES_HMMPOST.md)
# ======================================================================================================================
# lengths: 0, 1, 2; the float64 tile's seams (32 values), the int16 tile's (128 samples); the block seams at B = 128, 256
# and 1 024 with their neighbours
POST_LENS = (0, 1, 2, 31, 32, 33, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513, 1023, 1024, 1025)
POST_LIMITS = (0, 0, 1, 33, 129, 1000, 100000)
POST_DMAX = (70, 300, 1500, 2600)
POST_BLOCKS = (None, "256", "1024", "4096", "100")          # SK_HMM_POST_BLOCK; 100 is refused by post_block(): 128
POST_SAMPLES = 200_000                           # samples per case (the statement's CPU time, RANDOM_CASES_HMMPOST.md)
POST_LONGEST = 2600                              # ... and of its longest read: 21 blocks at B = 128
# sub_batches() of sk_api.hip never cuts a call of fewer than 8 192 rows, so in a fifth of the batch cases under
# SK_INGEST_MB=1 the read count is this one: short reads and one of POST_MANY_LONG samples, whose stride of 130 or more
# brings the sub-batch down to its floor of 4 096 rows -- three sub-batches of 2 800
POST_MANY = 8400
POST_MANY_SHORT = 12
POST_MANY_LONG = 130
POST_GUARD = 256                                 # bytes behind each output of the device form


def post_block_of(env):
    """post_block() of sk_hmm_post.hip"""
    v = int(env.get("SK_HMM_POST_BLOCK", "0"))
    return v if 128 <= v <= 4096 and v % 128 == 0 else 128


def hmmpost_calls(case):
    """[(reads, npad, stride or None)] per C call of the case's api call: sk_hmm_npad over the stride of an int16 batch
    (api.pack_i16's for the integer reads of a list), over the longest read of a float64 call"""
    lens = [len(r) for r in case["reads"]]
    limit = case["limit"]

    def npad(n):
        return max(1, min(n, limit) if limit > 0 else n)
    if case["feed"] == "batch":
        return [(case["R"], npad(case["stride"]), case["stride"])]
    if case["feed"] == "f64":
        return [(case["R"], npad(max(lens + [0])), None)]
    ints = [n for n, r in zip(lens, case["reads"]) if _is_int_read(r)]
    flts = [n for n, r in zip(lens, case["reads"]) if not _is_int_read(r)]
    calls = []
    if ints:
        stride = max(8, (max(ints) + 7) // 8 * 8)
        calls.append((len(ints), npad(stride), stride))
    if flts:
        calls.append((len(flts), npad(max(flts)), None))
    return calls


def hmmpost_sub_batches(case):
    """Sub-batches sub_batches() of sk_api.hip makes of the case's largest int16 host call (1 for a float64 call)"""
    most = 1
    target = (int(case["env"]["SK_INGEST_MB"]) << 20) if "SK_INGEST_MB" in case["env"] else 256 << 20
    for nreads, _, stride in hmmpost_calls(case):
        if stride is None:
            continue
        per = max(4096, target // (stride * 2))
        if per * 2 <= nreads:
            most = max(most, -(-nreads // per))
    return most


def hmmpost_slices(case):
    """Slices sk_launch_hmm_post makes of the case's reads -- post_group_bytes / post_slice_groups of sk_hmm_post.hip -- per
    launch (a sub-batch of the largest C call), the most of the case's calls"""
    budget = (int(case["env"]["SK_HMM_SCRATCH_MB"]) << 20) if "SK_HMM_SCRATCH_MB" in case["env"] else 16 << 30
    B = post_block_of(case["env"])
    most = 0
    for nreads, npad, stride in hmmpost_calls(case):
        if stride is not None:
            nsub = hmmpost_sub_batches(dict(case, feed="batch", R=nreads, stride=stride))
            nreads = -(-nreads // nsub)
        group_bytes = 64 * 8 + (-(-npad // B) + B) * (6 * 64 * 8)
        groups = (nreads + 63) // 64
        g = min(max(1, budget // group_bytes), groups)
        most = max(most, -(-groups // g))
    return most


def draw_hmmpost(rng):
    """One posterior call: draw_hmm's model; R of HMM_COUNTS (or POST_MANY, see there) reads, each with a length of POST_LENS
    or a uniform one up to a drawn maximum, inside POST_SAMPLES samples and POST_LONGEST a read, drawn as draw_hmm draws
    them; the feed (an int16 batch with an aligned or an unaligned stride, with or without calibration pairs; float64
    values; a list of integer and float reads), the limit, which outputs are asked for, and the switches
    SK_HMM_POST_BLOCK, SK_HMM_SCRATCH_MB and SK_INGEST_MB."""
    model, S, integer = _draw_hmm_model(rng)
    env = {}
    R = int(_pick(rng, HMM_COUNTS))
    dmax = int(_pick(rng, POST_DMAX))
    block = _pick(rng, POST_BLOCKS)
    if block is not None:
        env["SK_HMM_POST_BLOCK"] = block
    if rng.random() < 0.35:
        env["SK_HMM_SCRATCH_MB"] = "1"
    if rng.random() < 0.3:
        env["SK_INGEST_MB"] = "1"
    feed = _pick(rng, ("batch", "batch", "f64", "list"))
    limit = int(_pick(rng, POST_LIMITS))
    counts, dense = bool(rng.random() < 0.8), bool(rng.random() < 0.8)
    many = bool("SK_INGEST_MB" in env and feed == "batch" and rng.random() < 0.2)
    if many:
        R, dmax = POST_MANY, POST_MANY_SHORT
        lens = [int(n) for n in rng.integers(0, POST_MANY_SHORT + 1, R)]
        lens[int(rng.integers(R))] = POST_MANY_LONG
    else:
        lens = _ragged_lens(rng, R, POST_LENS, dmax, POST_SAMPLES)
    reads = [_det_read(rng, n)[0] for n in lens]
    cal, nfloat, aligned = None, 0, None
    case = dict(family="hmmpost", R=R, S=S, integer=integer, feed=feed, limit=limit, dmax=dmax, counts=counts, dense=dense)
    if feed == "batch":
        aligned = bool(rng.random() < 0.5)
        case["sig"], case["lens"], case["stride"] = _i16_rows(rng, reads, aligned)
        if rng.random() < 0.5:
            cal = np.stack([rng.uniform(-50, 50, R), rng.uniform(0.1, 0.3, R)], axis=1)
    else:
        for r in range(R):
            if len(reads[r]) and (feed == "f64" or rng.random() < 0.5):
                reads[r] = reads[r].astype(np.float64) * float(_pick(rng, (1.0, 0.25, 0.1))) + 0.37    # not integers
                nfloat += 1
    case.update(aligned=aligned, calibrated=cal is not None, nfloat=nfloat, total=int(sum(len(r) for r in reads)),
                longest=max(len(r) for r in reads), model=model, cal=cal, reads=reads, env=env)
    return case


def hmmpost_rows(case):
    """(x float64 [R, N] in the model's units, n_used int64 [R]): what the statement runs on"""
    lens = np.array([len(r) for r in case["reads"]], dtype=np.int64)
    x = np.zeros((case["R"], max(1, int(lens.max(initial=0)))))
    for i, r in enumerate(case["reads"]):
        x[i, :len(r)] = np.asarray(r, dtype=np.float64)
    if case["cal"] is not None:
        x = (x + case["cal"][:, :1]) * case["cal"][:, 1:]
    return x, (np.minimum(lens, case["limit"]) if case["limit"] > 0 else lens)


POST_CLASS_CUTS = (32, 128, 512)                 # where expect_hmmpost may part the reads by the samples they use
POST_STEP_READS = 140                            # a time step of the statement costs what 140 padded samples cost


def hmmpost_classes(used):
    """The reads parted by the samples they use, for the statement's CPU time alone: hmm_post_ref advances the reads of a
    call together over the rectangle [reads, longest], and every read's arithmetic is the statement's whatever its
    neighbours are, so a few short rectangles give the bytes of the one wide one.  Of the partitions at subsets of
    POST_CLASS_CUTS, the one with the smallest sum of longest * (POST_STEP_READS + reads)."""
    used = np.asarray(used, dtype=np.int64)
    best = None
    for pick in range(1 << len(POST_CLASS_CUTS)):
        cuts = [c for k, c in enumerate(POST_CLASS_CUTS) if pick >> k & 1]
        cls = np.searchsorted(cuts, used, side="left") if cuts else np.zeros(used.size, dtype=np.int64)
        parts = [np.flatnonzero(cls == k) for k in range(len(cuts) + 1)]
        parts = [p for p in parts if p.size]
        cost = sum(int(used[p].max()) * (POST_STEP_READS + p.size) for p in parts)
        if best is None or cost < best[0]:
            best = (cost, parts)
    return best[1]


def expect_hmmpost(ora, case, whole=False):
    """dict(post, counts, goff, gamma) by hmm_post_ref.posterior_batch / posterior_reads, always with counts and dense rows:
    one call per class of hmmpost_classes (whole: one call over all reads -- the same bytes, asserted on the CPU)"""
    import hmm_post_ref
    used = hmmpost_rows(case)[1]
    parts = [np.arange(case["R"])] if whole else hmmpost_classes(used)
    post = np.zeros(case["R"], dtype=hmm_post_ref.POST_DTYPE)
    counts = np.zeros(case["R"], dtype=hmm_post_ref.COUNTS_DTYPE)
    goff = np.concatenate([[0], np.cumsum(used)]).astype(np.int64)
    gamma = np.zeros((int(goff[-1]), hmm_post_ref.STATES))
    for idx in parts:
        if case["feed"] == "batch":
            p, c, off, g = hmm_post_ref.posterior_batch(case["model"], case["sig"][idx], case["lens"][idx],
                                                        None if case["cal"] is None else case["cal"][idx], case["limit"])
        else:
            p, c, off, g = hmm_post_ref.posterior_reads(case["model"], [case["reads"][i] for i in idx], case["limit"])
        post[idx], counts[idx] = p, c
        for k, r in enumerate(idx):
            gamma[goff[r]:goff[r + 1]] = g[off[k]:off[k + 1]]
    assert np.array_equal(post["n_used"], used)
    return dict(post=post, counts=counts, goff=goff, gamma=gamma)


def call_hmmpost(api, case, exp=None):
    """(post, counts or None, goff or None, gamma [goff[R], 6] or None) of the case's call with the outputs it asks for"""
    model, limit, reads, counts, dense = hmm_model_of(api, case), case["limit"], case["reads"], case["counts"], case["dense"]
    if case["feed"] == "batch":
        return api.hmm_posterior_batch(case["sig"], case["lens"], model, case["cal"], limit, counts, dense)
    if case["feed"] == "f64":
        return api.hmm_posterior_ragged_f64(*api.pack_f64(reads), model, limit, counts, dense)
    post, cnt, gammas = api.hmm_posterior(reads, model, limit, counts, dense)
    if not dense:
        return post, cnt, None, None
    goff = np.concatenate([[0], np.cumsum([len(g) for g in gammas])]).astype(np.int64)
    return post, cnt, goff, np.concatenate(gammas + [np.zeros((0, 6))])


def hmmpost_device_call(api, case, counts, dense, shift=0):
    """sk_hmm_posterior_dev_i16 on device buffers, the rows `shift` bytes behind a 16-byte boundary, POST_GUARD bytes of
    0x5A behind post, counts and the dense rows: (post, counts or None, goff or None, gamma or None, clean) -- clean:
    nothing written behind an output, and nothing at all to one that was not asked for"""
    import ctypes as C
    from squigglekit_amd import _lib
    L = _lib.ensure_init()
    sig, lens = np.ascontiguousarray(case["sig"]), np.ascontiguousarray(case["lens"])
    R, stride = sig.shape
    n = np.clip(lens.astype(np.int64), 0, stride)
    goff = np.concatenate([[0], np.cumsum(np.minimum(n, case["limit"]) if case["limit"] > 0 else n)]).astype(np.int64)
    sizes = (R * 112, R * 624, int(goff[R]) * 48)
    outs = [np.full(s + POST_GUARD, 0x5A, dtype=np.uint8) for s in sizes]
    ins = [sig, lens, goff] + ([np.ascontiguousarray(case["cal"])] if case["cal"] is not None else [])
    model = hmm_model_of(api, case)
    ptrs = []
    try:
        for a in ins + outs:
            ptrs.append(L.sk_dev_alloc(a.nbytes + 16))
            _lib.check(L.sk_dev_upload(ptrs[-1] + (shift if a is sig else 0), _lib.ptr(a), a.nbytes))
        d_out = ptrs[len(ins):]
        _lib.check(L.sk_hmm_posterior_dev_i16(ptrs[0] + shift, stride, ptrs[1], R, ptrs[3] if case["cal"] is not None else None,
                                              C.byref(model), case["limit"], d_out[0], d_out[1] if counts else None,
                                              ptrs[2] if dense else None, d_out[2] if dense else None))
        _lib.check(L.sk_sync())
        for a, d in zip(outs, d_out):
            _lib.check(L.sk_dev_download(_lib.ptr(a), d, a.nbytes))
    finally:
        for d in ptrs:
            L.sk_dev_free(d)
    clean = all(bool(np.all(a[-POST_GUARD:] == 0x5A)) for a in outs)
    if not counts:
        clean = clean and bool(np.all(outs[1] == 0x5A))
    if not dense:
        clean = clean and bool(np.all(outs[2] == 0x5A))
    post = outs[0][:-POST_GUARD].view(api.HMM_POST_DTYPE).copy()
    cnt = outs[1][:-POST_GUARD].view(api.HMM_COUNTS_DTYPE).copy() if counts else None
    gamma = outs[2][:-POST_GUARD].view(np.float64).reshape(-1, 6).copy() if dense else None
    return post, cnt, goff if dense else None, gamma, clean


POST_BOTH_SEED, POST_BOTH_READS = 22, 65


def hmmpost_both_kinds(case, exp, R=POST_BOTH_READS):
    """A hand-made case out of a drawn batch case with impossible reads: R of its reads, a possible one with samples and an
    impossible one in turn, so that lane by lane a wavefront holds both kinds (emissions are finite, so where a drawn
    model has impossible reads its possible ones have at most S samples, and a drawn wavefront holds few of them).
    `exp` is the statement's answer to `case`: it only says which reads are which."""
    post = exp["post"]
    live = np.flatnonzero((post["flags"] == 0) & (post["n_used"] > 0))
    live = np.concatenate([live[post["n_used"][live] >= 2], live[post["n_used"][live] < 2]])     # two samples and more first
    dead = np.flatnonzero(post["flags"] != 0)
    assert case["feed"] == "batch" and len(live) >= (R + 1) // 2 and len(dead) >= R // 2
    idx = np.empty(R, dtype=np.int64)
    idx[0::2], idx[1::2] = live[:(R + 1) // 2], dead[:R // 2]
    reads = [case["reads"][int(i)] for i in idx]
    return dict(case, made="both kinds", R=R, sig=np.ascontiguousarray(case["sig"][idx]), lens=case["lens"][idx].copy(),
                cal=None if case["cal"] is None else case["cal"][idx].copy(), reads=reads,
                total=int(sum(len(r) for r in reads)), longest=max(len(r) for r in reads))


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def diff_hmmpost(case, got, exp):
    """What a posterior call returned against the statement, every double by its bit pattern: no tolerance anywhere"""
    post, cnt, goff, gamma = got[:4]
    want = exp["post"]
    if post.shape != want.shape:
        return "records shaped %s, want %s" % (post.shape, want.shape)
    for f in ("n_used", "flags"):
        if not np.array_equal(post[f], want[f]):
            r = int(np.flatnonzero(post[f] != want[f])[0])
            return "read %d: %s %d, want %d" % (r, f, post[f][r], want[f][r])
    checks = [("post", post, want, ("loglik", "final_post", "occ"))]
    if cnt is not None:
        checks.append(("counts", cnt, exp["counts"], ("n", "sx", "sxx", "xi", "init")))
    for name, g, w, fields in checks:
        if g.shape != w.shape:
            return "%s shaped %s, want %s" % (name, g.shape, w.shape)
        for f in fields:
            bad = np.flatnonzero((_u64(g[f]) != _u64(w[f])).reshape(len(w), -1).any(axis=1))
            if bad.size:
                r = int(bad[0])
                return "read %d (%d samples used): %s.%s got %r want %r" % (r, want["n_used"][r], name, f, g[f][r], w[f][r])
    if post.tobytes() != want.tobytes():
        return "the records' bytes differ where no field does"
    if len(got) > 4 and not got[4]:                             # (before the return below: the call without dense rows too)
        return "bytes written behind an output of the device form, or to one that was not asked for"
    if gamma is None:
        return None
    if not np.array_equal(np.asarray(goff, dtype=np.int64), exp["goff"]):
        return "goff %s want %s" % (np.asarray(goff).tolist()[:8], exp["goff"].tolist()[:8])
    if gamma.shape != exp["gamma"].shape:
        return "dense rows shaped %s, want %s" % (gamma.shape, exp["gamma"].shape)
    if np.isnan(gamma).any():
        return "a NaN among the dense rows, first at row %d" % int(np.flatnonzero(np.isnan(gamma).any(axis=1))[0])
    bad = np.flatnonzero((_u64(gamma) != _u64(exp["gamma"])).any(axis=1))
    if bad.size:
        q = int(bad[0])
        r = int(np.searchsorted(exp["goff"], q, side="right") - 1)
        return "read %d (%d samples used): gamma differs first at sample %d: got %r want %r" % (
            r, want["n_used"][r], q - int(exp["goff"][r]), gamma[q], exp["gamma"][q])
    return None


# ======================================================================================================================
# segment levels
# ======================================================================================================================
# sk_seglev.hip: the kept mask in entries of 64 raw samples; k_seglev_stats stages a work item (a segment, or the whole
# read) of up to SEGLEV_LDS_COLS samples in LDS and takes the scratch tier beyond.
SEGLEV_LDS_COLS = 4096
LEVELS_LENS = (0, 1, 63, 64, 65, 127, 128, 129, SEGLEV_LDS_COLS - 1, SEGLEV_LDS_COLS, SEGLEV_LDS_COLS + 1)
LEVELS_ROUTES = ("batch", "batch_pa", "ragged", "list")
LEVELS_MAX_SEGS = (1, 2, 64)
LEVELS_LIMITS = ((0, 900), (0, 900), (-50, 1200), (-50, 1200), (200, 2500))


def draw_levels(rng):
    from squigglekit_amd import synth
    route = _pick(rng, LEVELS_ROUTES)
    lo, hi = _pick(rng, LEVELS_LIMITS)
    seg = dict(error=_pick(rng, (5, 5, 3, 0, 10)), corrector=_pick(rng, (50, 50, 3, 20)),
               window=_pick(rng, (150, 100, 20, 126, 127, 400)), seg_dist=_pick(rng, (50, 0, 1, 10 ** 9)),
               std_scale=_pick(rng, SWEEP_STD[:6]), stall_len=_pick(rng, (0.25, 0.05, 0.9, 1.2)), lim_low=lo, lim_hi=hi)
    base = 20.0 if lo < 0 and rng.random() < 0.7 else 500.0               # lim_low < 0: kept samples of both signs
    spread = float(_pick(rng, (60.0, 60.0, 20.0, 3.0)))                   # 3: a handful of distinct values, ties
    if base == 20.0:
        spread = min(spread, 20.0)
    reads = []
    for n in rng.choice(LEVELS_LENS, size=5, replace=False):
        reads.append(_stall_read(rng, int(n), base, spread))
    for _ in range(int(_pick(rng, (3, 9, 20)))):
        reads.append(_stall_read(rng, int(rng.integers(400, 4000)), base, spread))
    if base == 500.0:
        M = int(_pick(rng, (512, 2047, 4000)))
        reads += [r.astype(np.float64) for r in synth.pattern_reads(rng, int(_pick(rng, (2, 5))), M)]
    # one read above SEGLEV_LDS_COLS samples with a quiet stretch longer than that (a segment for the scratch tier)
    n = int(rng.integers(2 * SEGLEV_LDS_COLS + 500, 3 * SEGLEV_LDS_COLS))
    x = rng.normal(base, spread, n)
    a = int(rng.integers(100, 400))
    x[a:a + SEGLEV_LDS_COLS + int(rng.integers(50, 400))] = rng.normal(base + spread / 10, spread / 8, 1)[0]
    x += rng.normal(0, spread / 20, n)
    reads.append(x)
    for i in range(len(reads)):                                           # many dropped samples in some reads
        n = len(reads[i])
        if n >= 64 and rng.random() < 0.4:
            k = max(1, n // int(_pick(rng, (5, 20, 60))))
            reads[i][rng.integers(0, n, k)] = rng.choice([-500, 3000, 2999, hi, lo], k)
    reads = [np.clip(np.rint(r), -32768, 32767).astype(np.int16) for r in reads]
    order = rng.permutation(len(reads))
    reads = [reads[int(i)] for i in order]
    R = len(reads)
    case = dict(family="levels", route=route, seg=seg, lo=lo, hi=hi, base=base, spread=spread, R=R,
                longest=max(len(r) for r in reads))
    if route != "list":                           # (api.segment_levels takes no max_segs: the list form starts at 64)
        case["max_segs"] = int(_pick(rng, LEVELS_MAX_SEGS))
    if route in ("batch", "batch_pa"):
        case["sig"], case["lens"], case["stride"] = _i16_rows(rng, reads, True, pad=int(base))
    if route == "batch_pa":
        cal = np.empty((R, 3))
        cal[:, 0] = rng.choice([8192.0, 2048.0], R)
        cal[:, 1] = np.round(rng.uniform(-40, 40, R), 1)
        cal[:, 2] = rng.uniform(600, 1600, R)
        if base == 20.0:
            cal[:, 1] = np.round(rng.uniform(-4, 4, R), 1)
            cal[:, 2] = cal[:, 0] * rng.uniform(0.8, 1.2, R)              # unit about 1: both signs stay
        case["calib"] = cal
        reads = [np.round((r.astype(np.int64) + cal[i, 1]) * (float("{0:.2f}".format(cal[i, 2])) / cal[i, 0]), 2)
                 for i, r in enumerate(reads)]                            # (segmenter.py's pA values: the reference's input)
        if base == 500.0:
            case["lo"], case["hi"] = lo, hi = (0, 900) if lo >= 0 else (-10, 250)
            seg.update(lim_low=lo, lim_hi=hi)
    elif route == "ragged":
        reads = [np.round(r * 0.25 + 0.01 * rng.integers(0, 3, len(r)), 2) for r in reads]    # a 0.01 grid: ties
        case["lo"], case["hi"] = lo, hi = (lo // 4, hi // 4)
        seg.update(lim_low=lo, lim_hi=hi)
    elif route == "list":
        for i in range(R):
            if len(reads[i]) and rng.random() < 0.5:
                reads[i] = reads[i].astype(np.float64) + 0.5
    case.update(nfloat=sum(r.dtype == np.float64 for r in reads), reads=reads, env={})
    return case


def _no_levels(shape, dtype):
    """records of slots that hold no span: six NaNs, raw_start = raw_end = -1, n = 0"""
    a = np.zeros(shape, dtype=dtype)
    for f in ("mean", "std", "median", "mad", "min", "max"):
        a[f] = np.nan
    a["raw_start"] = a["raw_end"] = -1
    return a


def levels_expected(dtype, reads, segs, shape, lo, hi):
    """(levels [shape], read_level [R]) of the record type `dtype` as plain numpy makes them on the given segments
    (segs[r]: [[s, e], ..] in filtered coordinates): every record over w = y[s:e], y = the kept samples of the read --
    int64 for an integer read."""
    want_l, want_r = _no_levels(shape, dtype), _no_levels(len(reads), dtype)

    def one(w, kept, s):
        m = np.median(w)
        return (np.mean(w), np.std(w), m, np.median(np.abs(w - m)), w.min(), w.max(), kept[s], kept[s + len(w) - 1] + 1, len(w), 0)
    for r, a in enumerate(reads):
        a = np.asarray(a)
        if a.dtype.kind in "iu":
            a = a.astype(np.int64)
        kept = np.flatnonzero((a > lo) & (a < hi))
        y = a[kept]
        if y.size:
            want_r[r] = one(y, kept, 0)
        for k in range(min(len(segs[r]), shape[1])):
            s, e = segs[r][k]
            if len(y[s:e]):
                want_l[r, k] = one(y[s:e], kept, s)
    return want_l, want_r


def levels_mismatch(levels, read_level, want_l, want_r):
    """None, or where the records differ (doubles by bit pattern)"""
    for got, want, what in ((levels, want_l, "levels"), (read_level, want_r, "read_level")):
        for f in got.dtype.names:
            g, w = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
            if g.dtype.kind == "f":
                g, w = g.view(np.uint64), w.view(np.uint64)
            d = np.argwhere(g != w)
            if d.size:
                return "%s.%s at %s: got %r want %r" % (what, f, d[0].tolist(), got[f][tuple(d[0])], want[f][tuple(d[0])])
    return None


def expect_levels(ora, case):
    """segs[r]: the oracle's segments of read r (all of them: the call grows max_segs until none is cut)."""
    s = case["seg"]
    p = ora.SegParams(s["error"], s["corrector"], s["window"], s["seg_dist"], s["std_scale"], s["stall_len"])
    segs = []
    for r in case["reads"]:
        f = ora.scale_outliers(np.asarray(r, dtype=np.float64), case["lo"], case["hi"])
        segs.append([list(x) for x in ((ora.get_segs(f, p, max_segs=f.size // 2 + 8) or []) if f.size else [])])
    return dict(segs=segs)


def call_levels(api, case, exp=None):
    from squigglekit_amd._lib import SegParams
    p = SegParams(**case["seg"])
    if case["route"] == "batch":
        return api.segment_levels_batch(case["sig"], case["lens"], p, max_segs=case["max_segs"])
    if case["route"] == "batch_pa":
        return api.segment_levels_batch_pa(case["sig"], case["lens"], case["calib"], p, max_segs=case["max_segs"])
    if case["route"] == "ragged":
        return api.segment_levels_ragged_f64(*api.pack_f64(case["reads"]), None, p, max_segs=case["max_segs"])
    return api.segment_levels(case["reads"], p)


def diff_levels(case, got, exp):
    segs, nsegs, levels, read_level = got
    for r, want in enumerate(exp["segs"]):
        if int(nsegs[r]) != len(want) or segs[r, :nsegs[r]].tolist() != want:
            return "read %d (%d samples): segments %s, want %s" % (r, len(case["reads"][r]), segs[r, :nsegs[r]].tolist()[:3],
                                                                    want[:3])
    want_l, want_r = levels_expected(levels.dtype, case["reads"], exp["segs"], levels.shape, case["lo"], case["hi"])
    return levels_mismatch(levels, read_level, want_l, want_r)


# ======================================================================================================================
# screen: one int16 first-match call through the fixed-point screening scheme (sk_sdtwq.hip)
# ======================================================================================================================
# sk_launch_sdtw takes the screening scheme for 256 reads and more whose rows (the stride of an int16 batch) hold at
# least 4 * (N + N / 8 + 8 + ck) samples; screen_layout gives a motif L lanes per read and R = ceil(N / L) rows per lane,
# one compiled kernel per (L, R) and pass; the tagged sweep (the start hint) runs for L = 8 and 16 up to HINT_MAX_R rows.
SCREEN_MIN_READS = 256
SCREEN_N = (1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 199, 200, 201, 256, 257, 399, 400, 401, 512, 513, 1024)
SCREEN_CK = (64, 128, 256)                       # SK_DTW_CK: steps between checkpoints; a window spans 4 * ck columns
SCREEN_LIMITS = ((0, 1200), (0, 900), (-50, 2500), (400, 650))
SCREEN_CELLS = 1_500_000_000                     # cost-matrix cells the oracle fills per case (see RANDOM_CASES.md)
SCREEN_HOSTILE = 21                              # the last rows of a screen_batch
HINT_MAX_R, HINT_MAX_PLEN, HINT_MIN_READS, HINT_MIN_N = 25, 8192, 500000, 16      # sk_sdtwq.hip
SCREEN_GRID = [(L, R) for L in (8, 16) for R in range(1, 33)] + [(64, R) for R in range(1, 17)]


def screen_min_len(N, ck=128):
    """The shortest row, a multiple of 8, with which a motif of N points takes the screening scheme (sk_sdtw.hip: screens)."""
    return (4 * (N + N // 8 + 8 + ck) + 7) // 8 * 8


def screen_grid_lengths(L, R):
    """The two motif lengths of a grid test: L * R (no short lanes) and L * R - p, p from 1, L / 2, L - 1 in turn."""
    p = (1, L // 2, L - 1)[(R - 1) % 3]
    return [N for N in (L * R, L * R - p) if N > 0]


def screen_shape(N, nreads, maxlen, ql=None):
    """(L, R) as screen_layout (sk_sdtwq.hip) picks them; ql: SK_DTW_QL."""
    L = 8 if (N <= 256 and nreads >= (65536 if maxlen > 8192 else 49152)) else 16 if N <= 512 else 64
    if ql is not None:
        v = int(ql)
        if (v == 8 and N <= 256) or (v == 16 and N <= 512) or v == 64:
            L = v
    return L, (N + L - 1) // L


def screen_hint_gate(N, L, R, nreads, maxlen, env):
    """Whether sk_launch_sdtw_screen takes the tagged sweep for an int16 call."""
    hint_min = HINT_MIN_READS
    if int(env.get("SK_DTW_HINT_MIN", "0")) > 0:
        hint_min = int(env["SK_DTW_HINT_MIN"])
    return L in (8, 16) and N + maxlen + 2 <= HINT_MAX_PLEN and R <= HINT_MAX_R and N >= HINT_MIN_N and \
        nreads >= hint_min and "SK_DTW_NOHINT" not in env


def screen_chunks(L, R, nreads, maxlen, ck, scratch_mb):
    """(chunks sk_launch_sdtw_screen makes of a call under SK_DTW_SCRATCH_MB = scratch_mb -- None: one --, the scratch
    bytes it counts per read)."""
    nck = (maxlen + L - 1) // ck
    lq_stride = (maxlen + 3 * L + 7) & ~3
    per_read = max(nck, 1) * L * ((R + 3) // 2) * 4 + lq_stride * 4 + L * (R + 2) * 4 + (nck + 1) * L * 4 + 64
    if scratch_mb is None:
        return 1, per_read
    chunk = min(nreads, max(64, (int(scratch_mb) << 20) // per_read))
    return -(-nreads // chunk), per_read


def motif_image(v):
    """A motif in raw units, as synth.squiggle_batch plants it (kept inside the default limits)."""
    return np.clip(np.rint(np.asarray(v, dtype=np.float64) * 93.4 + 511.0), 1, 1199).astype(np.int16)


def screen_motif(N, seed=11):
    """synthetic_motif(N, seed'), seed' the first from `seed` on whose raw image is not constant (a short motif can be one
    level: its copies tiled end to end would be a constant row)."""
    from squigglekit_amd import synth
    for s in range(seed, seed + 64):
        motif = synth.synthetic_motif(N, seed=s)
        if N < 2 or np.unique(motif_image(motif)).size > 1:
            break
    return motif


def screen_batch(R, M, N, seed, ck=128, motif=None):
    """(sig [R, M] int16, lens, motif): synth.squiggle_batch rows with the motif planted, all of full length, and behind
    them SCREEN_HOSTILE rows picked to mislead the screening scheme -- the batch of tests/test_gpu_hint.py with its
    positions scaled to M and N.  M >= screen_min_len(N, ck)."""
    from squigglekit_amd import synth
    assert R > SCREEN_HOSTILE and M >= screen_min_len(N, ck)
    if motif is None:
        motif = screen_motif(N)
    sig = synth.squiggle_batch(R, M, seed, motif=motif)
    lens = np.full(R, M, dtype=np.int32)
    copy = motif_image(motif)
    h, wmax = R - SCREEN_HOSTILE, 4 * ck
    # two copies further apart than one window takes (4 checkpoint intervals): a second window (sibling)
    sig[h, 4:4 + N] = copy
    sig[h, M - N - 4:M - 4] = copy
    a = M // 8
    if a + 2 * N + wmax + 8 <= M:                                           # (where M allows)
        sig[h + 1, a:a + N] = copy
        sig[h + 1, a + N + wmax + 8:a + 2 * N + wmax + 8] = copy
    # copies stretched 3x and 4x: paths wider than every look-back; one of them ends on the last sample
    s3, s4 = motif_image(np.repeat(motif, 3)), motif_image(np.repeat(motif, 4))
    sig[h + 2, 50:50 + s3.size] = s3
    sig[h + 3, 50:50 + s4.size] = s4
    sig[h + 4, M - s3.size:] = s3
    # copies that start in the read's first granule, and one that ends on its last sample
    for r, off in ((h + 5, 0), (h + 6, 5), (h + 7, 15), (h + 8, M - N)):
        sig[r, off:off + N] = copy
    sig[h + 9, :] = 500                                                     # constant: MAD = 0
    sig[h + 10, :] = 500 + (np.arange(M) % 2)                               # two levels: every cost ties with many others
    sig[h + 11, :] = np.tile(copy, M // N + 1)[:M]                          # the motif end to end: near-minima everywhere
    if _np_mad_is_zero(sig[h + 11], 0, 1200):                               # (a short motif: more than half of it one level)
        sig[h + 11, :] += ((np.arange(M) // N) % 3).astype(np.int16)        # every tile 0, 1 or 2 raw units up: MAD = 1 unit
    rng = np.random.default_rng([97, int(seed), N])
    lens[h + 12:h + 18] = (0, 1, max(N - 1, 0), N, N + 1, M - 1)            # ragged: around the motif's length
    lens[h + 18:h + 21] = rng.integers(2, M, 3)
    return sig, lens, motif


def _np_mad_is_zero(x, lo, hi):
    f = x[(x > lo) & (x < hi)].astype(np.float64)
    return f.size > 0 and float(np.median(np.abs(f - np.median(f)))) == 0.0


def screen_mad0_rows(sig, lens, lo=0, hi=1200):
    """Rows with samples inside the limits whose MAD is 0 (the reference divides by zero there: flag 2, not compared)."""
    return [r for r in range(sig.shape[0]) if _np_mad_is_zero(sig[r, :lens[r]], lo, hi)]


def draw_screen(rng):
    env = {}
    nm = int(_pick(rng, (1, 1, 1, 2, 3)))
    ql = _pick(rng, (None, "8", "16", "64"))
    if nm > 1 and ql == "64":
        ql = _pick(rng, (None, "8", "16"))       # (a motif list is there to change L between motifs)

    def one_n(lo, hi):
        listed = [n for n in SCREEN_N if lo <= n <= hi]
        return int(_pick(rng, listed)) if rng.random() < 0.5 else int(rng.integers(lo, hi + 1))
    if nm == 1 and rng.random() < 0.5:           # a length made for the layout: every R under the L asked for, P = 0 and P > 0
        L = int(ql) if ql else 16
        N = L * int(rng.integers(1, (32 if L < 64 else 16) + 1)) - int(_pick(rng, (0, 0, 1, L // 2, L - 1, int(rng.integers(L)))))
        Ns = [max(1, N)]
    elif nm == 1:
        Ns = [one_n(1, 1024)]
    else:
        # consecutive motifs on different L: the resident quantised motif is keyed on L alone (motifq_L), and the later
        # motifs read the samples the first motif's prologue compacted
        classes = ((1, 256), (257, 512), (513, 640)) if ql == "8" else ((1, 512), (513, 640))
        k0 = int(rng.integers(len(classes)))
        Ns = [one_n(*classes[(k0 + k) % len(classes)]) for k in range(nm)]
    from squigglekit_amd import synth
    motifs = [screen_motif(Ns[0], seed=int(rng.integers(1000)))]
    motifs += [synth.synthetic_motif(N, seed=int(rng.integers(1000))) for N in Ns[1:]]
    ck = int(_pick(rng, (128, 128, 64, 256)))
    if ck != 128:
        env["SK_DTW_CK"] = str(ck)
    if ql is not None:
        env["SK_DTW_QL"] = ql
    hint = _pick(rng, ("on", "on", "on", "off", "default"))
    if hint == "on":
        env["SK_DTW_HINT_MIN"] = "1"
    elif hint == "off":
        env["SK_DTW_NOHINT"] = "1"
    if rng.random() < 0.5:
        env["SK_DTW_SORT_MIN"] = "1"             # the window passes take every chunk in sorted order
    for key, p in (("SK_DTW_NOFUSE", 0.3), ("SK_DTW_NO_EARLY", 0.3), ("SK_DTW_NO_SIBLINGS", 0.2)):
        if rng.random() < p:
            env[key] = "1"
    scale = _pick(rng, ("medmad", "medmad", "zscale"))
    lo, hi = _pick(rng, SCREEN_LIMITS)
    # ---- rows at the screening threshold of the longest motif and a little above it; 256 to about 700 reads
    M = screen_min_len(max(Ns), ck) + int(_pick(rng, (0, 0, 8, 24, 200)))
    R = int(rng.integers(SCREEN_MIN_READS, 701))
    R = max(SCREEN_MIN_READS, min(R, SCREEN_CELLS // (M * sum(Ns))))
    sig, lens, _ = screen_batch(R, M, Ns[0], int(rng.integers(1 << 30)), ck=ck, motif=motifs[0])
    h = R - SCREEN_HOSTILE
    for m in motifs[1:]:                          # copies of the other motifs in some of the plain rows
        for r in rng.integers(0, h, 12):
            at = int(rng.integers(0, M - len(m)))
            sig[r, at:at + len(m)] = motif_image(m)
    k = int(rng.integers(0, 40))                  # samples on and beyond the limits
    sig[rng.integers(0, h, k), rng.integers(0, M, k)] = rng.choice([-9, 0, 899, 900, 1199, 1200, 3000], k)
    stride = M
    if rng.random() < 0.4:                        # a stride longer than the longest row, padding that is not zeros
        stride = M + 8 * int(rng.integers(1, 6))
        wide = rng.integers(300, 700, size=(R, stride)).astype(np.int16)
        wide[:, :M] = sig
        sig = wide
    case = dict(family="screen", Ns=Ns, R=R, M=M, stride=stride, ck=ck, ql=ql, hint=hint, scale=scale, lo=lo, hi=hi,
                motifs=motifs, sig=sig, lens=lens, env=env)
    # ---- SK_DTW_SCRATCH_MB small enough for three chunks or more, where a whole number of MB is
    if rng.random() < 0.5:
        L, Rr = screen_shape(Ns[0], R, stride, ql)
        per_read = screen_chunks(L, Rr, R, stride, ck, 1)[1]
        mb = per_read * (R // 3) >> 20
        if mb >= 1:
            env["SK_DTW_SCRATCH_MB"] = str(mb)
    return case


def screen_plan(case):
    """Per motif: dict(N, L, R, P, hinted, chunks) as the library lays the call out."""
    out = []
    mb = case["env"].get("SK_DTW_SCRATCH_MB")
    for N in case["Ns"]:
        L, R = screen_shape(N, case["R"], case["stride"], case["ql"])
        out.append(dict(N=N, L=L, R=R, P=L * R - N,
                        hinted=screen_hint_gate(N, L, R, case["R"], case["stride"], case["env"]),
                        chunks=screen_chunks(L, R, case["R"], case["stride"], case["ck"], mb)[0]))
    return out


def expect_screen(ora, case):
    """want[m]: the oracle's records of motif m, the reads split over host threads."""
    from concurrent.futures import ThreadPoolExecutor
    sig, lens, R = case["sig"], case["lens"], case["R"]
    per = (R + 15) // 16
    jobs = [(m, a, min(R, a + per)) for m in range(len(case["motifs"])) for a in range(0, R, per)]
    mode = 0 if case["scale"] == "medmad" else 1
    with ThreadPoolExecutor(16) as ex:
        parts = list(ex.map(lambda j: ora.motifseq_batch_i16(sig[j[1]:j[2]], lens[j[1]:j[2]], case["motifs"][j[0]],
                                                             scale_mode=mode, lo=case["lo"], hi=case["hi"]), jobs))
    return dict(want=[np.concatenate([p for j, p in zip(jobs, parts) if j[0] == m]) for m in range(len(case["motifs"]))])


def call_screen(api, case, exp=None):
    args = (case["scale"], case["lo"], case["hi"])
    if len(case["motifs"]) == 1:
        return [api.motifseq_batch(case["sig"], case["lens"], case["motifs"][0], *args)]
    return api.motifseq_multi_batch(case["sig"], case["lens"], case["motifs"], *args)


def screen_compared(got, want):
    """The reads whose records are compared: all but the ones flagged MAD = 0 / std = 0, where the reference divides by
    zero (a read with nothing inside the limits is compared: n = 0)."""
    return ((got["flags"] & 2) == 0) & np.isfinite(want["dist"]) | (want["n"] == 0)


def diff_screen(case, got, exp):
    for m, (g, want) in enumerate(zip(got, exp["want"])):
        ok = screen_compared(g, want)
        same = (g["start"] == want["start"]) & (g["end"] == want["end"]) & (g["n"] == want["n"]) & \
               ((_bits(g["dist"]) == _bits(want["dist"])) | (np.isnan(g["dist"]) & np.isnan(want["dist"])))
        bad = np.flatnonzero(~same & ok)
        if bad.size:
            return "motif %d (N=%d) read %d (%d samples): got %s want %s" % (m, case["Ns"][m], bad[0], case["lens"][bad[0]],
                                                                            g[bad[0]], want[bad[0]])
    return None


# ======================================================================================================================
# the twins of the hit family: the read background on the hits cases, events and pooling on the paths cases
# ======================================================================================================================
def twin_case(family, case, use_seed=None):
    """A hits / paths case as its twin's: the same reads, motifs, K, scaling and switches (max_dist is inf, the reads go in
    as the list); `use_seed` seeds the pooling mask of the events twin."""
    return dict(case, family=family, of=case["family"], use_seed=int(case["seed"] if use_seed is None else use_seed))


def _twin_args(case):
    return (case["motifs"], case["K"], float("inf"), case["scale"], case["lo"], case["hi"])


def events_use(case, m, n):
    return np.random.default_rng([98, case["use_seed"], m]).random(n) < 0.7


def expect_background(ora, case):
    from test_background_host import reference_background_reads
    return dict(want=[reference_background_reads(ora, case["reads"], m, case["scale"], case["lo"], case["hi"])
                      for m in case["motifs"]])


def call_background(api, case, exp=None):
    return api.motifseq_background(case["reads"], *_twin_args(case)), api.motifseq_hits(case["reads"], *_twin_args(case))


def diff_background(case, got, exp):
    got, twin = got
    for m, want in enumerate(exp["want"]):
        if got[m][0].tobytes() != twin[m][0].tobytes() or not np.array_equal(got[m][1], twin[m][1]):
            return "motif %d: hit lists differ from the hit-list call's" % m
        for r, w in enumerate(want):
            g = got[m][2][r]
            if w is None:
                ok = g["below"] == -1 and all(np.isnan(g[f]) for f in ("mean", "std", "median", "mad"))
            else:
                ok = (int(g["below"]), int(g["n"])) == w[4:] and all(
                    np.float64(g[f]).tobytes() == np.float64(v).tobytes()
                    for f, v in zip(("mean", "std", "median", "mad"), w))
            if not ok:
                return "motif %d read %d (%d samples): got %s want %s" % (m, r, len(case["reads"][r]), g, w)
    return None


def expect_events(ora, case):
    from test_events_host import reference_batch, reference_pool
    want = [reference_batch(ora, case["reads"], m, case["K"], case["scale"], case["lo"], case["hi"])[1]
            for m in case["motifs"]]
    use = [events_use(case, m, w.shape[0] * w.shape[1]) for m, w in enumerate(want)]
    return dict(want=want, use=use, pool=[reference_pool(w, u) for w, u in zip(want, use)])


def call_events(api, case, exp):
    got = api.motifseq_events(case["reads"], *_twin_args(case))
    bad = api.last_path_mismatches()
    twin = api.motifseq_hits(case["reads"], *_twin_args(case))
    pools = [api.pool_events(got[m][2], exp["use"][m]) if got[m][2].shape == exp["want"][m].shape else None
             for m in range(len(case["motifs"]))]
    return got, twin, bad, pools


def diff_events(case, got, exp):
    got, twin, bad, pools = got
    for m, want in enumerate(exp["want"]):
        if got[m][0].tobytes() != twin[m][0].tobytes() or not np.array_equal(got[m][1], twin[m][1]):
            return "motif %d: hit lists differ from the hit-list call's" % m
        if bad != 0:
            return "%d hits failed the path kernel's self-check" % bad
        if got[m][2].shape != want.shape:
            return "motif %d: events shaped %s, want %s" % (m, got[m][2].shape, want.shape)
        if got[m][2].tobytes() != want.tobytes():
            r, k, i = (int(v[0]) for v in np.nonzero(got[m][2] != want))
            return "motif %d read %d hit %d point %d: got %s want %s" % (m, r, k, i, got[m][2][r, k, i], want[r, k, i])
        if any(pools[m][f].tobytes() != exp["pool"][m][f].tobytes() for f in exp["pool"][m].dtype.names):
            return "motif %d: the pooled model differs from numpy's" % m
    return None


# ======================================================================================================================
# dRNA segmenter, slow5 branch: k_drna_stats / k_prep_i16<.., WINDOWED, ..> (sk_prep.hip), k_drna_walk(_runs)
# ======================================================================================================================
DRNA_SAMPLES = 4_000_000                         # samples the oracle walks per case (about 32 ns each, filter included)
DRNA_COUNTS = (1, 63, 64, 65, 130, 257)          # one read per lane: a lone lane, a full wave and its neighbours, 5 waves
DRNA_TILE = 8 * 256                              # k_drna_stats / k_prep_i16: 8 samples per thread, 256 threads
DRNA_LENS = (0, 1, 63, 64, 65, 127, 128, 129, DRNA_TILE - 1, DRNA_TILE, DRNA_TILE + 1, 2 * DRNA_TILE)
DRNA_LONG = 70000
DRNA_W = (1, 2, 63, 64, 65, 100, 128, 1200, 1 << 24, (1 << 24) + 1)       # the scan by runs takes 64 <= w <= 2^24
DRNA_ERROR = (0, 1, 5, 63, 64, 65, 100, -1)
DRNA_SEG_DIST = (0, 1, 50, 10 ** 9)
DRNA_NO_ERR = (0, -7, 2500, 2560, 10 ** 7, INT32_MAX)                     # 2500: mid-word; 2560 = 40 * 64
DRNA_LIMITS = ((0, 1200), (300, 700), (0, 2049), (0, 2050), (-50, 2500))  # hi - lo - 1 = 2048 | 2049: the one-look gate
DRNA_STD = (0.8, 0.0, -0.5, 1e6, -1e6, 0.2, 1.5)                          # 1e6: top > 32767; -1e6: nothing in band
DRNA_WINDOWS = ((1000, 5000), (0, 2000), (0, 16384), (0, 16385), (700, 700), (1000, DRNA_TILE), (0, INT32_MAX))
DRNA_STRIDES = (8, 64, 128, 136, 320, 384)       # ceil(stride / 64) against the blocks of 256 of finish_stats
DRNA_ROUTES = ("list", "equal", "padded", "odd")
DRNA_OUT = 30000                                 # a sample outside every pair of limits above
DRNA_IN, DRNA_FAR = 400, 700                     # the two levels of a crafted read: in band, out of band
DRNA_PREFIX = 64                                 # crafted reads: 8 samples of DRNA_FAR, 56 of DRNA_IN; t_start = 0, t_end = 64
# sk_launch_prep_i16, restated: sizeof(Scratch) = 2 * 4 * 4 + 4 * 8 + 4 * 4 + 256 * 8 + 2 * 8 + 256 * 4 + 128 * 2 + 4 * 4
PREP_SCRATCH_BYTES = 3440
DRNA_LDS_GATE = 60 * 1024
PREP_LDSCOMP_GATE = 40 * 1024
DRNA_ONE_LOOK_STD = (0.0, 1e6, -1e6)             # signal variants 10 .. 12: these on the script's own parameters (k_drna_stats)
# the variants of a case: (kind, argument); the first draw of draw_drna picks one
DRNA_VARIANTS = ([("signal", i) for i in range(13)] + [("mask", i) for i in range(10)] +
                 [("crafted", s) for s in ("bits", "rearm", "thresh", "prev_err", "merge", "overflow", "exact", "budget")] +
                 [("stride", s) for s in DRNA_STRIDES] + [("long", s) for s in ("list", "lds-over", "lds-under")])


def drna_lds_bytes(stride, nbins, t_end):
    """Dynamic LDS of k_drna_stats as sk_launch_prep_i16 computes it."""
    nb4 = (nbins + 3) & ~3
    return PREP_SCRATCH_BYTES + 4 * nb4 + 4 * (2 * ((stride + 63) // 64) + 2) + 2 * (t_end + DRNA_TILE + 8)


def drna_route(case, env=None):
    """The statistics kernel a case takes: 'one-look' (k_drna_stats) or 'prep<lds|mem,win|all>' (k_prep_i16)."""
    env = case["env"] if env is None else env
    p, stride = case["params"], case["stride"]
    lo, hi = max(p["lim_low"], -32769), min(p["lim_hi"], 32768)
    nbins = max(0, hi - lo - 1)
    t0, t1 = p["t_start"], p["t_end"]
    if "SK_DRNA_STEP" not in env and 1 <= nbins <= 2048 and 0 <= t0 < t1 <= 16384 and stride < (1 << 19) and \
            drna_lds_bytes(stride, nbins, t1) <= DRNA_LDS_GATE:
        return "one-look"
    ldscomp = PREP_SCRATCH_BYTES + 4 * ((nbins + 3) & ~3) + 2 * stride <= PREP_LDSCOMP_GATE
    return "prep<%s,%s>" % ("lds" if ldscomp else "mem", "win" if t0 > 0 or t1 < INT32_MAX else "all")


def drna_walk(case, env=None):
    """sk_launch_drna_walk: 'runs' (k_drna_walk_runs) or 'step' (k_drna_walk)."""
    env = case["env"] if env is None else env
    p = case["params"]
    runs = 64 <= p["w"] <= (1 << 24) and 0 <= p["window"] <= (1 << 24) and "SK_DRNA_STEP" not in env
    return "runs" if runs else "step"


def _mask_runs(*runs):
    """(bit, count) pairs -> bool mask."""
    return np.concatenate([np.full(int(n), bool(b)) for b, n in runs] + [np.zeros(0, dtype=bool)])


def _pad_bits(mask, mod, bit=0):
    """The mask lengthened by `bit` until its length is `mod` modulo 64."""
    return np.concatenate([mask, np.full((mod - len(mask)) % 64, bool(bit))])


def _two_level(mask):
    return np.where(mask, DRNA_IN, DRNA_FAR).astype(np.int16)


def _drna_prefix():
    return _mask_runs((0, 8), (1, DRNA_PREFIX - 8))


def _random_mask(rng, n):
    """Runs of in-band and out-of-band samples with lengths around the seams of the scan: 1 .. 3, a word, the windows."""
    out, total = [], 0
    while total < n:
        kind = int(rng.integers(6))
        if kind == 0:                                # a long run with a few holes
            b = rng.random(int(rng.integers(40, 400))) > float(_pick(rng, (0.0, 0.01, 0.05)))
        elif kind == 1:                              # a run and a gap of exactly k
            b = _mask_runs((1, _pick(rng, (1, 2, 62, 63, 64, 65, 127, 128, 129, 200))),
                           (0, _pick(rng, (1, 2, 3, 5, 6, 7, 50, 51, 52, 64, 65))))
        elif kind == 2:                              # alternating
            per = int(rng.integers(2, 6))
            b = (np.arange(int(rng.integers(20, 300))) % per != 0) ^ bool(rng.integers(2))
        elif kind == 3:                              # a hole
            b = np.zeros(int(rng.integers(1, 200)), dtype=bool)
        elif kind == 4:                              # noise
            b = rng.random(int(rng.integers(10, 300))) < rng.uniform(0.3, 0.95)
        else:                                        # trains
            on, off = int(rng.integers(30, 140)), int(rng.integers(1, 12))
            b = (np.arange(int(rng.integers(100, 600))) % (on + off)) < on
        out.append(np.asarray(b, dtype=bool))
        total += len(b)
    return np.concatenate(out)[:n] if out else np.zeros(0, dtype=bool)


def _mask_read(rng, n):
    """A two-level read of n samples: the clean prefix, then a random mask (n < DRNA_PREFIX: the prefix cut short)."""
    return _two_level(np.concatenate([_drna_prefix(), _random_mask(rng, max(0, n - DRNA_PREFIX))])[:n])


def _drna_crafted(rng, which):
    """(params, masks, max_segs): reads whose band mask is the bit pattern given (see RANDOM_CASES.md), each behind the clean
    prefix -- a run that opens at sample 8.  tests/test_random_cases.py finds every seam in a sample-level trace."""
    pre = _drna_prefix()
    P = dict(t_start=0, t_end=DRNA_PREFIX, std_scale=float(_pick(rng, (0.2, 0.8, 1.5))), lim_low=0, lim_hi=1200,
             no_err_thresh=0)
    max_segs = 32
    if which == "bits":
        # error 0: the first out-of-band sample closes.  A run of 63 from the sample behind a close: closed at bit 63 of the
        # lane's window; a run of 64: the window is swallowed whole, the next one closes at its bit 0; a run of one sample
        P.update(error=0, w=128, window=2, seg_dist=0)
        masks = [np.concatenate([pre, _mask_runs((0, 1), (1, 63), (0, 1), (1, 64), (0, 1), (1, 1), (0, 1), (1, 30), (0, 9))]),
                 np.concatenate([pre, _mask_runs((0, 1), (1, 64), (0, 1), (1, 63), (0, 3), (1, 1), (0, 2))])]
    elif which == "rearm":
        # w = 64, window = 0: c is a multiple of w at start + 63, + 127, ...: a run that opens on a word's first sample
        # re-arms on its last one, a run that opens on the second sample re-arms on the next word's first one; 130 samples
        # in band re-arm twice (err = -2), then error + 2 = 3 out-of-band samples are taken and the fourth closes
        P.update(error=1, w=64, window=0, seg_dist=10 ** 9)
        m = _pad_bits(np.concatenate([pre, _mask_runs((0, 10))]), 0)
        m = np.concatenate([m, _mask_runs((1, 130), (0, 4))])
        m = _pad_bits(m, 1)
        m = np.concatenate([m, _mask_runs((1, 70), (0, 5), (1, 12), (0, 3))])
        m2 = _pad_bits(np.concatenate([pre, _mask_runs((0, 3))]), 1)
        m2 = np.concatenate([m2, _mask_runs((1, 200), (0, 1), (1, 5), (0, 1), (1, 5), (0, 1), (1, 5), (0, 1), (1, 5), (0, 9))])
        masks = [m, m2]
    elif which == "thresh":
        # no_err_thresh = 200 (bit 8 of its word): three out-of-band samples before it are taken and not counted, the run goes
        # on past it, takes error = 2 counted ones and closes at the third
        P.update(error=2, no_err_thresh=200, w=1200, window=10, seg_dist=5)
        masks = [np.concatenate([pre, _mask_runs((1, 100), (0, 3), (1, 40), (0, 2), (1, 5), (0, 1), (1, 20), (0, 40))]),
                 np.concatenate([pre, _mask_runs((1, 130), (0, 1), (1, 5), (0, 1), (1, 5), (0, 2), (1, 9), (0, 30))])]
    elif which == "prev_err":
        # end = i - prev_err with the out-of-band tail inside one piece, and with it split over two pieces (a run that opens
        # at sample 100 has its first piece end at sample 153: three of the tail before it, two and the closing one behind)
        P.update(error=5, w=1200, window=10, seg_dist=0)
        masks = [np.concatenate([pre, _mask_runs((1, 20), (0, 6), (0, 10), (1, 51), (0, 6), (1, 30), (0, 2), (1, 3), (0, 8))])]
    elif which == "merge":
        # gaps counted from the closing sample (error 0: end = the closing sample): a run 19 behind it merges, one 20 behind
        # does not; 21 idle samples (i - last_end = 20) do not stop the scan, 22 do, with a run of 30 behind them
        P.update(error=0, w=1200, window=5, seg_dist=20)
        masks = [np.concatenate([pre, _mask_runs((0, 25), (1, 30), (0, 19), (1, 30), (0, 20), (1, 30), (0, 21), (1, 30), (0, 22),
                                             (1, 30), (0, 5))]),
                 np.concatenate([pre, _mask_runs((0, 19), (1, 3), (0, 1), (1, 40), (0, 30), (1, 40), (0, 5))])]
    elif which == "overflow":
        # more segments than the 32 columns the call begins with: SK_ERR_OVERFLOW, the call grows max_segs
        P.update(error=0, w=64, window=2, seg_dist=1)
        masks = [np.concatenate([pre] + [_mask_runs((0, 1 + k % 2), (1, 3 + k % 5)) for k in range(45)] + [_mask_runs((0, 4))])]
    elif which == "exact":
        # exactly max_segs = 4 segments, then a run that merges into the last one (the store at column nseg - 1 = max_segs - 1)
        P.update(error=0, w=100, window=3, seg_dist=3)
        max_segs = 4
        masks = [np.concatenate([pre, _mask_runs((0, 3), (1, 5), (0, 3), (1, 5), (0, 4), (1, 5), (0, 2), (1, 7), (0, 3))])]
    else:
        # a budget of more than 64: whole windows of out-of-band samples are swallowed
        P.update(error=int(_pick(rng, (65, 100))), w=int(_pick(rng, (64, 1200))), window=10, seg_dist=50)
        masks = [np.concatenate([pre, rng.random(400) < 0.5, _mask_runs((0, 130), (1, 40), (0, 200))]),
                 np.concatenate([pre, _mask_runs((1, 10), (0, 64), (1, 1), (0, 70), (1, 30), (0, 120))])]
    return P, masks, max_segs


def _drop(rng, x, frac):
    if frac and len(x):
        x = x.copy()
        x[rng.random(len(x)) < frac] = DRNA_OUT
    return x


def _fill_reads(rng, count, budget, lo_len=300, hi_len=40000):
    """`count` dRNA-like reads of about budget / count samples each."""
    from squigglekit_amd import synth
    if count <= 0:
        return []
    avg = max(lo_len + 1, min(hi_len, budget // count))
    a, b = max(lo_len, avg // 2), max(lo_len + 2, min(hi_len, avg + avg // 2))
    reads = synth.drna_reads(count, int(rng.integers(1 << 30)), min_len=a, max_len=b)
    over, k = sum(len(r) for r in reads) - budget, 0
    while over > 0:                                  # (the reference's CPU time: never more than the budget)
        cut = min(over, len(reads[k]) // 2)
        reads[k] = reads[k][:len(reads[k]) - cut]
        over, k = over - cut, (k + 1) % count
    return reads


def _batch_rows(rng, reads, route, stride=None):
    """(sig [R, stride] int16, lens, stride) for a batch route: 'equal' -- the longest row; 'padded' -- beyond it, a
    multiple of 8, padding that is not zeros; 'odd' -- an odd stride (no vector loads)."""
    longest = max([len(r) for r in reads] + [1])
    if stride is None:
        stride = {"equal": longest, "padded": (longest + 8 + int(rng.integers(0, 40))) // 8 * 8,
                  "odd": (longest + int(rng.integers(0, 9))) | 1}[route]
    sig = rng.integers(300, 700, size=(len(reads), stride)).astype(np.int16) if route != "equal" else \
        np.zeros((len(reads), stride), dtype=np.int16)
    for i, r in enumerate(reads):
        sig[i, :len(r)] = r
        if route == "equal":
            sig[i, len(r):] = 555
    return sig, np.array([len(r) for r in reads], dtype=np.int32), int(stride)


def draw_drna(rng):
    kind, arg = DRNA_VARIANTS[int(rng.integers(len(DRNA_VARIANTS)))]
    P = dict(error=5, no_err_thresh=2500, w=1200, window=100, seg_dist=1200, t_start=1000, t_end=5000, std_scale=0.8,
             lim_low=0, lim_hi=1200)
    max_segs, route, stride, lost, crafted_at = 32, "list", None, "", None
    if kind == "signal":
        # the statistics: every window, pair of limits, std_scale and read count in turn; the scan's parameters with them
        i = arg
        w = DRNA_W[i % 10]
        (P["lim_low"], P["lim_hi"]), (P["t_start"], P["t_end"]) = DRNA_LIMITS[i % 5], DRNA_WINDOWS[(i + 2) % 7]
        short = i in (3, 4)                           # rows that k_prep_i16 keeps in LDS (its LDSCOMP instantiations)
        P.update(w=w, window=int(_pick(rng, (0, 1, 30, 100, 250))), error=DRNA_ERROR[i % 8],
                 seg_dist=DRNA_SEG_DIST[(i + 2) % 4], no_err_thresh=DRNA_NO_ERR[i % 6], std_scale=DRNA_STD[i % 7])
        if i >= 10:                                   # the script's parameters, std_scale aside: the one-look kernel
            P = dict(error=5, no_err_thresh=2500, w=1200, window=100, seg_dist=1200, t_start=1000, t_end=5000,
                     std_scale=DRNA_ONE_LOOK_STD[i - 10], lim_low=0, lim_hi=1200)
        R, route = DRNA_COUNTS[(i + 1) % 6], DRNA_ROUTES[i % 4]
        t0, t1 = P["t_start"], min(P["t_end"], 6000 if short else 20000)
        seams = list(DRNA_LENS) + [max(0, t0 - 1), t0, t0 + 1, t1 - 1, t1, t1 + 1]
        special = [rng.integers(300, 700, size=n).astype(np.int16) for n in dict.fromkeys(seams)]
        special.append(np.full(int(rng.integers(1, 3000)), DRNA_OUT, dtype=np.int16))          # nothing kept
        x = rng.integers(300, 700, size=2 * DRNA_TILE + int(rng.integers(0, 3000))).astype(np.int16)
        if DRNA_TILE <= t1 <= 2 * DRNA_TILE:
            # t1 kept samples in the first two tiles exactly: the collection is complete at a tile's end
            x[rng.choice(2 * DRNA_TILE, 2 * DRNA_TILE - t1, replace=False)] = DRNA_OUT
        special.append(x)
        special = [special[int(k)] for k in rng.permutation(len(special))][:R]
        fill = _fill_reads(rng, R - len(special), DRNA_SAMPLES - sum(len(s) for s in special), 300, 6000 if short else 40000)
        fracs = rng.choice([0.0, 0.01, 0.25], size=len(fill))
        fill = [_drop(rng, f, float(q)) for f, q in zip(fill, fracs)]
        lost = "".join("n" if q == 0 else "1" if q < 0.1 else "q" for q in fracs)[:40]
        reads = special + fill
    elif kind == "mask":
        # the scan: two-level reads with a drawn mask behind the clean prefix; w and error in turn, the rest drawn
        i = arg
        w = DRNA_W[i]
        # window against w (kw0, the first re-arming count): 0, 1, below, at and above w, a multiple of it -- in turn
        window = (0, 1, max(0, w - 1 - int(rng.integers(0, 3))), w, w + int(rng.integers(1, 9)), 2 * w)[(i + 1) % 6]
        if w >= (1 << 20):
            window = int(_pick(rng, (0, 1, 30, 100)))
        P.update(t_start=0, t_end=DRNA_PREFIX, std_scale=float(_pick(rng, (0.2, 0.8, 1.5))), w=w, window=window,
                 error=DRNA_ERROR[(i + 3) % 8], seg_dist=int(_pick(rng, DRNA_SEG_DIST + (50, 200))),
                 no_err_thresh=int(_pick(rng, (0, 0, -7, 100, 128, 300, 300, 10 ** 7, INT32_MAX))))
        R, route = int(_pick(rng, DRNA_COUNTS[1:])), _pick(rng, DRNA_ROUTES)
        lens = [int(_pick(rng, DRNA_LENS)) if rng.random() < 0.3 else int(rng.integers(DRNA_PREFIX, 6000)) for _ in range(R)]
        reads = [_mask_read(rng, n) for n in lens]
    elif kind == "crafted":
        cp, masks, max_segs = _drna_crafted(rng, arg)
        P.update(cp)
        R, route = int(_pick(rng, (63, 65, 130))), _pick(rng, DRNA_ROUTES)
        reads = [_two_level(m) for m in masks]
        if arg != "exact":                            # (exact: no read may hold more than max_segs segments)
            reads += [_mask_read(rng, int(rng.integers(DRNA_PREFIX, 3000))) for _ in range(R - len(reads))]
        else:
            reads += [_two_level(np.concatenate([_drna_prefix(), _mask_runs((0, 3), (1, int(rng.integers(3, 40))), (0, 9))]))
                      for _ in range(R - len(reads))]
        order = rng.permutation(len(reads))
        reads = [reads[int(k)] for k in order]
        crafted_at = [int(np.flatnonzero(order == k)[0]) for k in range(len(masks))]
    elif kind == "stride":
        # rows of at most `stride` samples that begin with eight out-of-band ones and end their collection at their own end
        # (fewer than t_end kept): the last block of finish_stats has idle wavefronts (see RANDOM_CASES.md, "Found")
        stride, route = int(arg), "equal"
        P.update(t_start=0, t_end=1000, std_scale=0.8, error=0, no_err_thresh=0, w=64, window=int(_pick(rng, (2, 3))),
                 seg_dist=int(_pick(rng, (0, 1, 50))))
        R = int(_pick(rng, (130, 257)))
        reads = []
        for _ in range(R):
            n = stride if rng.random() < 0.5 else int(rng.integers(max(1, stride - 63), stride + 1))
            if stride == 8:
                m = _mask_runs((0, 3), (1, 4), (0, 1))[:n] if rng.random() < 0.5 else rng.random(n) < 0.6
            else:
                body = _random_mask(rng, n)
                body[:8] = False
                k = int(body.sum())
                if 2 * k <= n:                        # (the median stays the in-band level)
                    body[8:8 + (n - 8) * 3 // 4] = True
                m = body
            reads.append(_two_level(np.asarray(m, dtype=bool)))
    else:
        from squigglekit_amd import synth
        R = int(_pick(rng, (3, 4, 6)))
        reads = _fill_reads(rng, R - 1, 200000, 3000, 60000)
        reads.append(synth.drna_reads(1, int(rng.integers(1 << 30)), min_len=DRNA_LONG, max_len=DRNA_LONG + 20000)[0])
        reads = [_drop(rng, x, float(_pick(rng, (0.0, 0.01)))) for x in reads]
        reads = [reads[int(k)] for k in rng.permutation(R)]
        if arg == "list":
            P.update(t_start=0, t_end=INT32_MAX)      # the whole read is the window: k_prep_i16 without WINDOWED
        else:
            # t_end = 16384 and 2048 histogram bins: 48 520 + 8 * ceil(stride / 64) bytes against the gate of 61 440
            route = "padded"
            P.update(lim_low=0, lim_hi=2049, t_start=int(_pick(rng, (0, 1000))), t_end=16384)
            stride = 103368 if arg == "lds-over" else 103360
    case = dict(family="drna", kind=kind, arg=arg, route=route, params=P, max_segs=max_segs, nreads=len(reads), reads=reads,
                longest=max([len(r) for r in reads] + [0]), lost=lost, env={})
    if crafted_at is not None:
        case["crafted_at"] = crafted_at
    if route == "list":
        case["stride"] = max(8, (case["longest"] + 7) // 8 * 8)                # api.pack_i16
    else:
        case["sig"], case["lens"], case["stride"] = _batch_rows(rng, reads, route, stride)
    return case


def expect_drna(ora, case):
    """Per read every segment of ora.scale_outliers + ora.drna_segs; `top` and the kept count with them (CPU leg)."""
    from concurrent.futures import ThreadPoolExecutor
    p = case["params"]
    op = ora.DrnaParams(**{k: v for k, v in p.items() if not k.startswith("lim")})

    def one(x):
        f = ora.scale_outliers(np.asarray(x, dtype=np.float64), p["lim_low"], p["lim_hi"])
        segs, top = ora.drna_segs(f, op, max_segs=16384)
        return segs, top, int(f.size)
    with ThreadPoolExecutor(16) as ex:
        rows = list(ex.map(one, case["reads"]))
    assert all(len(r[0]) < 16384 for r in rows)
    return dict(segs=[r[0] for r in rows], top=[r[1] for r in rows], kept=[r[2] for r in rows])


def call_drna(api, case, exp=None):
    from squigglekit_amd import _lib
    p = _lib.DrnaParams(**case["params"])
    if case["route"] == "list":
        return api.drna_segment_reads(case["reads"], p, max_segs=case["max_segs"])
    segs, nsegs = api.drna_segment_batch(case["sig"], case["lens"], p, max_segs=case["max_segs"])
    return [segs[r, :nsegs[r]].tolist() for r in range(case["nreads"])]


def diff_drna(case, got, exp):
    if len(got) != case["nreads"]:
        return "%d reads returned, want %d" % (len(got), case["nreads"])
    for r, (g, w) in enumerate(zip(got, exp["segs"])):
        if g != w:
            k = next((k for k in range(min(len(g), len(w))) if g[k] != w[k]), min(len(g), len(w)))
            return "read %d (%d samples, %d kept, top %r): %d segments, want %d; segment %d: got %s want %s" % (
                r, len(case["reads"][r]), exp["kept"][r], exp["top"][r], len(g), len(w), k, g[k:k + 2], w[k:k + 2])
    return None


# ======================================================================================================================
# dRNA segmenter, --signal branch: k_roll_stream / k_roll_one / k_roll_stats (sk_prep.hip), k_roll_walk
# ======================================================================================================================
ROLL_COUNTS = (1, 31, 32, 33, 63, 64, 65, 130)   # (the redo list of k_roll_stream runs on a grid of 32)
ROLL_W = (1, 2, 7, 63, 64, 65, 2000, 8192, 12000, 12001, 65535, 65536, 300000)      # 300 000: above every read
ROLL_STD = (0.5, 0.0, -3.0, 1e12, -1e12)
ROLL_CHUNK = (8191, 8192, 8193, 16384)           # numpy's summation chunks
ROLL_LDS_LONG = 35001                            # a row k_roll_one cannot hold in LDS
ROLL_SCRATCH_LONG = (1 << 17) + 1                # a row beyond sk_roll_one_lds' limit: prefix sums in a scratch row
ROLL_SHARED_BYTES = 2 * 16 * 4 * 2 + 5 * 64 * 8 + 6 * 8 + 2 * 8          # sizeof(RollShared)
ROLL_VARIANTS = [("signal", i) for i in range(len(ROLL_W))] + [("crafted", 0), ("crafted", 1000)]


def roll_stream_ok(stride, w, lo, hi):
    """sk_roll_stream_ok, restated."""
    if w > 12000 or stride > (1 << 21):
        return False
    smax = float(max(abs(lo), abs(hi))) * float(w)
    return smax < 2147483000.0 and smax * smax * float(stride) < 9.0e18


def roll_one_lds(stride, w):
    """sk_roll_one_lds, restated: the LDS bytes of k_roll_one for rows of `stride` samples, 0 when they do not fit."""
    if w >= 65536 or stride > (1 << 17):
        return 0
    i = stride + 1
    need = PREP_SCRATCH_BYTES + ROLL_SHARED_BYTES + (i + (i >> 3) + 4) * 4
    return need if need <= 160 * 1024 else 0


def roll_route(case, env=None):
    """drna_roll_dev's choice: 'stream' (k_roll_stream, its redo list through k_roll_one), 'one-look' (k_roll_one for every
    read) or 'two-kernels' (compaction + k_roll_stats)."""
    env = case["env"] if env is None else env
    p, stride = case["params"], case["stride"]
    lo, hi = max(p["lim_low"], -32769), min(p["lim_hi"], 32768)
    stream = roll_stream_ok(stride, p["w"], lo, hi) and "SK_ROLL_ONE_LOOK" not in env
    if (stream or roll_one_lds(stride, p["w"])) and "SK_ROLL_TWO_KERNELS" not in env and "SK_DRNA_STEP" not in env:
        return "stream" if stream else "one-look"
    return "two-kernels"


def roll_scan(t, bot, seg_dist):
    """dRNA_segmenter.py:296-316 on a rolling mean, sample by sample: (segments after merging, events).  Events:
    ('equal', c) a t == bot sample inside or outside a run; ('merge' | 'new', start - last_end) for every run closed behind
    another; ('open', start) a run still open at the end."""
    begin, start, end, last_end, segs, ev = False, 0, 0, 0, [], []
    for c, v in enumerate(t):
        if v == bot:
            ev.append(("equal", c, begin))
        if v < bot and not begin:
            start, begin = c, True
        elif v < bot:
            end = c
        elif v > bot and begin:
            if segs and start - last_end < seg_dist:
                ev.append(("merge", start - last_end))
                segs[-1][1] = end
            else:
                if segs:
                    ev.append(("new", start - last_end))
                segs.append([start, end])
            last_end = end
            start, end, begin = 0, 0, False
    if begin:
        ev.append(("open", start))
    return segs, ev


def _roll_numpy(x, w, std_scale):
    """(t, bot) of a short integer read in plain numpy (window sums are exact; for the draw only: the reference's
    t and bot are what the tests use)."""
    x = np.asarray(x, dtype=np.int64)
    if len(x) < w + 1:
        return np.full(len(x), np.nan), np.nan
    P = np.concatenate([[0], np.cumsum(x)])
    t = np.concatenate([np.full(w - 1, np.nan), (P[w:] - P[:-w]) / float(w)])
    v = t[w - 1:]
    return t, float(v.mean() - v.std(ddof=1) * std_scale)


def _blocks(*runs):
    return np.concatenate([np.full(int(n), int(v), dtype=np.int16) for v, n in runs])


def _roll_crafted(rng):
    """Two-level block reads for w = 4, std_scale = 0 (bot = the mean of t, between the levels): (reads, lo_thresh,
    hi_thresh, seg_dist).  Lengths and gaps are measured here in plain numpy and asserted by the CPU leg on the reference's
    own trace."""
    w, lo_v, hi_v, pad = 4, 400, 600, 60

    def seglen(L):
        x = _blocks((hi_v, pad), (lo_v, L), (hi_v, pad))
        s, _ = roll_scan(*_roll_numpy(x, w, 0.0), 0)
        return (s[0][1] - s[0][0]) if len(s) == 1 else None
    L0, L1 = int(rng.integers(30, 45)), int(rng.integers(90, 120))
    lo_t, hi_t = seglen(L0), seglen(L1)
    reads = [_blocks((lo_v, 40), (hi_v, 40))]                                  # one t == bot = 500.0
    reads += [_blocks((hi_v, pad), (lo_v, L), (hi_v, pad)) for L in (L0, L0 - 1, L1, L1 + 1)]
    # two low blocks G apart: seg_dist = the gap the scan sees at G, plus one (merged); at G + 1 the gap is seg_dist (not merged)
    seg_dist = None
    for G in range(int(rng.integers(12, 20)), 60):
        gaps = []
        for g in (G, G + 1):
            s, _ = roll_scan(*_roll_numpy(_blocks((hi_v, pad), (lo_v, 30), (hi_v, g), (lo_v, 30), (hi_v, pad)), w, 0.0), 0)
            gaps.append(s[1][0] - s[0][1] if len(s) == 2 else None)
        if None not in gaps and gaps[1] == gaps[0] + 1:
            seg_dist = gaps[0] + 1
            reads += [_blocks((hi_v, pad), (lo_v, 30), (hi_v, g), (lo_v, 30), (hi_v, pad)) for g in (G, G + 1)]
            break
    far = seg_dist + 40
    reads.append(_blocks((hi_v, pad), (lo_v, L0 - 12), (hi_v, far), (lo_v, L0 + 9), (hi_v, pad)))      # first too short
    reads.append(_blocks((hi_v, pad), (lo_v, 50)))                                                   # open at the end
    reads.append(_blocks((hi_v, pad), (lo_v, L0 + 3), (hi_v, far), (lo_v, 50)))                       # a segment, then an open run
    return reads, lo_t, hi_t, seg_dist


def draw_roll(rng):
    kind, arg = ROLL_VARIANTS[int(rng.integers(len(ROLL_VARIANTS)))]
    P = dict(w=2000, seg_dist=1500, hi_thresh=200000, lo_thresh=2000, shift=1000, std_scale=0.5, lim_low=0, lim_hi=1200)
    route = _pick(rng, ("list", "list", "padded", "odd"))
    lost = ""
    if kind == "signal":
        i = arg
        w = ROLL_W[i]
        P.update(w=w, std_scale=ROLL_STD[i % 5], lo_thresh=int(_pick(rng, (3, 100, 2000))), shift=int(_pick(rng, (0, 1000))),
                 seg_dist=int(_pick(rng, (2, 100, 1500, 100000))))
        if rng.random() < 0.4:
            P.update(lim_low=300, lim_hi=700)
        R = ROLL_COUNTS[i % 8]
        seams = [0, 1, w - 1, w, w + 1, 2 * w] + list(ROLL_CHUNK)
        if i % 3 == 0 and w <= 12000:
            seams.append(ROLL_LDS_LONG + int(rng.integers(0, 4000)))
        if w == 65536:
            seams.append(ROLL_SCRATCH_LONG + int(rng.integers(0, 3000)))
        if w == 12001:
            seams = [n for n in seams if n <= 34000]              # (this case stays on k_roll_one's LDS tier)
        seams = [n for n in dict.fromkeys(seams) if n <= 140000]
        special = []
        for n in seams:
            x = (450 + 60 * np.sin(np.arange(n) / 900.0) + rng.normal(0, 12, n)).astype(np.int16)
            if n > 4000:
                x[n // 3: n // 3 + 2500] -= 150                    # a low stretch of acceptable length
            special.append(x)
        special = [special[int(k)] for k in rng.permutation(len(special))][:R]
        hi_len = 34000 if w == 12001 else 30000
        fill = _fill_reads(rng, R - len(special), DRNA_SAMPLES - sum(len(s) for s in special), 2000, hi_len)
        fracs = rng.choice([0.0, 0.01, 0.25], size=len(fill))
        fill = [_drop(rng, f, float(q)) for f, q in zip(fill, fracs)]
        lost = "".join("n" if q == 0 else "1" if q < 0.1 else "q" for q in fracs)[:40]
        reads = special + fill
    else:
        reads, lo_t, hi_t, seg_dist = _roll_crafted(rng)
        P.update(w=4, std_scale=0.0, lo_thresh=lo_t, hi_thresh=hi_t, seg_dist=seg_dist, shift=int(arg))
        ncraft = len(reads)
        R = int(_pick(rng, (33, 65)))
        for _ in range(R - ncraft):                                 # block reads at random
            runs = [(int(_pick(rng, (400, 600, 500, 450))), int(rng.integers(1, 90))) for _ in range(int(rng.integers(2, 12)))]
            reads.append(_blocks(*runs))
        reads[ncraft][::7] = DRNA_OUT                               # (dropped samples: the shift applies to filtered coordinates)
    case = dict(family="roll", kind=kind, arg=arg, route=route, params=P, nreads=len(reads), reads=reads,
                longest=max([len(r) for r in reads] + [0]), lost=lost, env={})
    if kind == "crafted":
        case["ncrafted"] = ncraft
    if route == "list":
        case["stride"] = max(8, (case["longest"] + 7) // 8 * 8)
    else:
        case["sig"], case["lens"], case["stride"] = _batch_rows(rng, reads, route)
    return case


def expect_roll(ora, case):
    from concurrent.futures import ThreadPoolExecutor
    p = case["params"]
    op = ora.RollParams(**{k: v for k, v in p.items() if not k.startswith("lim")})

    def one(x):
        f = ora.scale_outliers(np.asarray(x, dtype=np.float64), p["lim_low"], p["lim_hi"])
        return ora.drna_roll(f, op), int(f.size)
    with ThreadPoolExecutor(16) as ex:
        rows = list(ex.map(one, case["reads"]))
    return dict(xy=[r[0] for r in rows], kept=[r[1] for r in rows])


def call_roll(api, case, exp=None):
    import ctypes as C
    from squigglekit_amd import _lib
    p = _lib.RollParams(**case["params"])
    if case["route"] == "list":
        return api.drna_roll_reads(case["reads"], p)
    # the C entry point on rows of the case's own stride (api.drna_roll_reads packs to a multiple of 8)
    L = _lib.ensure_init()
    R = case["nreads"]
    sig, lens = np.ascontiguousarray(case["sig"]), np.ascontiguousarray(case["lens"])
    xy, found = np.zeros((R, 2), dtype=np.int32), np.zeros(R, dtype=np.int32)
    _lib.check(L.sk_drna_roll_batch_i16(_lib.ptr(sig), case["stride"], _lib.ptr(lens), R, C.byref(p), _lib.ptr(xy),
                                        _lib.ptr(found)))
    return [(int(xy[i, 0]), int(xy[i, 1])) if found[i] else None for i in range(R)]


def diff_roll(case, got, exp):
    if len(got) != case["nreads"]:
        return "%d reads returned, want %d" % (len(got), case["nreads"])
    for r, (g, w) in enumerate(zip(got, exp["xy"])):
        if g != w:
            return "read %d (%d samples, %d kept): got %s want %s" % (r, len(case["reads"][r]), exp["kept"][r], g, w)
    return None


# ======================================================================================================================
# DTW over a pair list (sk_pairs.hip, k_sdtw's MODE_PAIRS / MODE_PAIRS_GLOBAL) and its warping paths (sk_pairpath.hip)
# ======================================================================================================================
# query lengths around the lane (16 | 64), row (16 R | 64 R) and stripe (64 s) boundaries; 32 and 256 are where
# sk_exact_shape changes the lane layout, 1 024 is the longest query
PAIRS_SEAM = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 256, 257, 512, 1023, 1024)
PAIRS_SMALL_MAX = 2048                           # sk_exact_shape: up to here a query of 32 .. 256 points takes 64 lanes
PAIRS_CELLS = 30_000_000                         # cost-matrix cells the oracle fills per case (see RANDOM_CASES.md)
PAIRS_TARGETS = (0, 1, 2, 3, 200, 513, 1025, 1500, 3000)
PAIRS_CLIFF = 3000                               # a target that keeps its wavefront running long after its mates ended
PAIRS_NATURAL_TARGET = 60                        # the natural L = 16 route: targets of a few dozen points
PAIRS_TILES = ((64, 40), (256, 128), (1024, 512))
# sk_pairpath.hip
PP_LDS_WORDS = PATH_LDS_BYTES // 4               # 6 400 direction words
PP_LDS_COLS = 1024
PP_ONE_WAVE = "1"                                # SK_PATH_SCRATCH_BYTES below any slab: one wavefront for all listed pairs
PP_TIERS = ({}, {"SK_PATH_LDS_BYTES": "0"}, {"SK_PATH_LDS_BYTES": "0", "SK_PATH_SCRATCH_BYTES": PP_ONE_WAVE})
PP_MAX_WAVES = 256                               # 8 wavefronts per CU: no device this runs on has fewer than 32 CUs


def pairs_cells(N, M, mode):
    """cells the oracle fills for one pair: the global mode runs between two sentinels"""
    if M == 0:
        return 0
    return (N + 2) * (M + 2) if mode == "global" else N * M


def _pairs_pool(rng, lens, ties):
    import pairs_ref
    return [pairs_ref.draw(rng, int(n), ties) for n in lens]


def _pairs_within(seqs, pairs, mode, budget, per_pair=1):
    """the longest prefix of `pairs` (one pair at least) whose reference stays inside the cell budget"""
    keep, total = [], 0
    for q, t in pairs:
        c = per_pair * pairs_cells(len(seqs[q]), len(seqs[t]), mode)
        if keep and total + c > budget:
            break
        keep.append((int(q), int(t)))
        total += c
    return keep, total


def _pairs_extras(rng, pairs, nq):
    """(i, i) pairs, a query used by three more pairs, a pair repeated verbatim -- mixed into the list"""
    pairs = list(pairs)
    pairs += [(q, q) for q in rng.integers(0, nq, size=int(rng.integers(0, 3))).tolist()]
    if rng.random() < 0.5:
        q = int(rng.integers(0, nq))
        pairs += [(q, pairs[int(rng.integers(len(pairs)))][1]) for _ in range(3)]
    if rng.random() < 0.5:
        pairs.insert(int(rng.integers(len(pairs) + 1)), pairs[int(rng.integers(len(pairs)))])
    return pairs


def draw_pairs(rng):
    """A pool and a pair list for api.dtw_pairs.  kind 'list': the draw of the fuzz tool's former pairs leg (queries around
    the seams, targets of 0 .. 3 000 points, repeats, (i, i) pairs); 'natural': more than PAIRS_SMALL_MAX pairs without a
    switch, a query for every R of L = 16 and some on 64 lanes, targets of a few dozen points; 'cliff': every target is
    either at least PAIRS_CLIFF points or at most 3, so that a wavefront's lane groups end far apart."""
    kind = _pick(rng, ("list", "list", "list", "natural", "cliff"))
    mode = _pick(rng, ("subsequence", "global"))
    ties = bool(rng.random() < 0.4)
    env = {}
    if kind == "natural":
        lens = [16 * R - int(_pick(rng, (0, 1, 15, int(rng.integers(16))))) for R in range(1, 17)]
        lens += [int(_pick(rng, (257, 300, 512, 1023, 1024))) for _ in range(int(rng.integers(1, 4)))]
        lens += [int(_pick(rng, PAIRS_SEAM[:17])) for _ in range(int(rng.integers(0, 6)))]
        nq = len(lens)
        tl = [0, 1] + [int(rng.integers(2, PAIRS_NATURAL_TARGET + 1)) for _ in range(int(rng.integers(6, 20)))]
        seqs = _pairs_pool(rng, lens + tl, ties)
        npairs = PAIRS_SMALL_MAX + 1 + int(_pick(rng, (0, 0, 1, 3, int(rng.integers(300)))))
        q = np.concatenate([np.arange(nq), rng.integers(0, nq, size=npairs - nq)])       # every query is used
        pairs = list(zip(q.tolist(), rng.integers(nq, len(seqs), size=npairs).tolist()))
        pairs[int(rng.integers(npairs))] = (0, 0)
        pairs[int(rng.integers(1, npairs))] = pairs[0]
    elif kind == "cliff":
        if rng.random() < 0.5:
            env["SK_DTW_NO_SMALL"] = "1"
        nq = int(rng.integers(2, 9))
        lens = [int(_pick(rng, (1, 2, 15, 16, 17, 31, 40, 100))) for _ in range(nq)]
        tl = [int(_pick(rng, (0, 1, 2, 3))) for _ in range(int(rng.integers(2, 6)))]
        tl += [PAIRS_CLIFF + int(rng.integers(0, 200)) for _ in range(int(rng.integers(1, 3)))]
        seqs = _pairs_pool(rng, lens + tl, ties)
        npairs = int(_pick(rng, (3, 5, 9, 14, 30)))
        pairs = list(zip(rng.integers(0, nq, size=npairs).tolist(), rng.integers(nq, len(seqs), size=npairs).tolist()))
        pairs = _pairs_extras(rng, pairs, nq)
    else:
        if rng.random() < 0.5:
            env["SK_DTW_NO_SMALL"] = "1"
        nq = int(rng.integers(1, 40))
        lens = [int(_pick(rng, PAIRS_SEAM)) if rng.random() < 0.4 else int(rng.integers(1, 400)) for _ in range(nq)]
        tl = [int(_pick(rng, PAIRS_TARGETS)) for _ in range(int(rng.integers(0, 6)))]
        seqs = _pairs_pool(rng, lens + tl, ties)
        npairs = int(_pick(rng, (1, 3, 4, 5, 16, 17, 64, 200)))
        pairs = list(zip(rng.integers(0, nq, size=npairs).tolist(), rng.integers(0, len(seqs), size=npairs).tolist()))
        pairs = _pairs_extras(rng, pairs, nq)
    pairs, cells = _pairs_within(seqs, pairs, mode, PAIRS_CELLS)
    form = _pick(rng, ("list", "flat"))
    pad = int(rng.integers(1, 9)) if form == "flat" else 0
    return dict(family="pairs", kind=kind, mode=mode, ties=ties, form=form, pad=pad, nseq=len(seqs), nq=nq,
                npairs=len(pairs), cells=cells, seqs=seqs, pairs=np.array(pairs, dtype=np.int64).reshape(-1, 2), env=env)


def pairs_pool_of(case):
    """the pool as the case's form hands it to the library: the list, or (values, off) with off[0] = pad > 0 and NaN in
    front of the first sequence"""
    if case["form"] == "list":
        return case["seqs"]
    seqs = case["seqs"]
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    values = np.concatenate([np.full(case["pad"], np.nan)] + [np.asarray(s, dtype=np.float64) for s in seqs])
    return values, off + case["pad"]


def pairs_plan(case):
    """The host plan of sk_pairs_run as include/squigglekit_hip.h and sk_pairs.hip state it, in plain Python: dict(shape =
    {query index: (L, R)} by sk_exact_shape(N, npairs) under the case's switches, groups = {(L, R): dict(count, P, order,
    M)} in launch order (L = 16 before 64, R rising)) -- count pairs, P the sorted short-lane counts L R - N of the group's
    queries, order the pair indices as the table holds them (longest target first, ties in list order: the stable sort),
    M their target lengths.  Lane group k of a launch serves order[k]; a wavefront holds 64 / L of them."""
    seqs, pairs = case["seqs"], case["pairs"]
    shape, members = {}, {}
    for p, (q, t) in enumerate(pairs.tolist()):
        if q not in shape:
            shape[q] = panel_shape(len(seqs[q]), len(pairs), case["env"])                # (sk_exact_shape, restated there)
        members.setdefault(shape[q], []).append(p)
    groups = {}
    for key in sorted(members):
        L, R = key
        order = sorted(members[key], key=lambda p: -len(seqs[pairs[p, 1]]))             # (sorted() is stable)
        groups[key] = dict(count=len(order), order=order, M=[len(seqs[pairs[p, 1]]) for p in order],
                           P=sorted({L * R - len(seqs[pairs[p, 0]]) for p in order}))
    return dict(shape=shape, groups=groups)


def expect_pairs(ora, case):
    import pairs_ref
    want = pairs_ref.records(ora, case["seqs"], case["pairs"].tolist(), case["mode"])
    empty = np.array([len(case["seqs"][t]) == 0 for t in case["pairs"][:, 1]], dtype=bool)
    assert np.array_equal(np.isnan(want["dist"]), empty)       # a NaN distance is expected for an empty target only
    return dict(want=want)


def call_pairs(api, case, exp=None):
    return api.dtw_pairs(pairs_pool_of(case), case["pairs"], case["mode"])


def diff_pairs(case, got, exp):
    import pairs_ref
    want = exp["want"]
    if got.shape != want.shape:
        return "records shaped %s, want %s" % (got.shape, want.shape)
    for p in range(len(want)):                                  # every pair, by the rule of pairs_ref.same_records
        if not pairs_ref.same_records(got[p:p + 1], want[p:p + 1].astype(got.dtype)):
            q, t = case["pairs"][p]
            return "pair %d (%d, %d) (N=%d, M=%d): got %s want %s" % (p, q, t, len(case["seqs"][q]), len(case["seqs"][t]),
                                                                      got[p], want[p])
    return None


# ---- warping paths ------------------------------------------------------------------------------------------------------
def draw_pairpaths(rng):
    """A pool and a pair list for api.dtw_pairs_paths: the draw of the fuzz tool's former pair-paths leg (queries around
    the stripe edges, targets of 0 .. 3 000 points, repeats, (i, i) pairs), either mode, a tier setting of PP_TIERS, and
    where the records come from -- 'computed' in the call; 'own': the reference's records supplied as they are (NaN,
    FLAG_EMPTY records of empty targets among them); 'tiles' (subsequence): per pair the reference's records of the
    query in the pieces of api.tile_targets, merged by api.merge_tiles, traced against the whole target; 'wrong': the
    reference's records with a drawn handful changed (expect_pairpaths says how)."""
    mode = _pick(rng, ("subsequence", "global"))
    ties = bool(rng.random() < 0.4)
    tier = int(rng.integers(3))
    records = _pick(rng, ("computed", "computed", "own", "wrong", "tiles"))
    if records == "tiles":
        mode = "subsequence"
    kind = _pick(rng, ("list", "list", "list", "thin"))
    if kind == "thin":                           # few points against one column or one row: N == 1, M == 1, W == 1
        nq = int(rng.integers(2, 8))
        lens = [int(_pick(rng, (1, 1, 2, 3, 64, 65))) for _ in range(nq)]
        tl = [int(_pick(rng, (1, 1, 2, 16, 17, 1025, 1040))) for _ in range(int(rng.integers(1, 5)))]
    else:
        nq = int(rng.integers(1, 30))
        lens = [int(_pick(rng, PAIRS_SEAM)) if rng.random() < 0.4 else int(rng.integers(1, 400)) for _ in range(nq)]
        tl = [int(_pick(rng, PAIRS_TARGETS)) for _ in range(int(rng.integers(0, 6)))]
    seqs = _pairs_pool(rng, lens + tl, ties)
    npairs = int(_pick(rng, (1, 3, 16, 65, 200)))
    first = nq if kind == "thin" else 0
    pairs = list(zip(rng.integers(0, nq, size=npairs).tolist(), rng.integers(first, len(seqs), size=npairs).tolist()))
    pairs = _pairs_extras(rng, pairs, nq)
    piece, overlap = _pick(rng, PAIRS_TILES)
    per_pair = 2 if records != "tiles" else 2 + -(-piece // (piece - overlap))           # records + path (+ the pieces)
    pairs, cells = _pairs_within(seqs, pairs, mode, PAIRS_CELLS, per_pair)
    case = dict(family="pairpaths", kind=kind, mode=mode, ties=ties, tier=tier, records=records, nseq=len(seqs), nq=nq,
                npairs=len(pairs), cells=cells, seqs=seqs, pairs=np.array(pairs, dtype=np.int64).reshape(-1, 2),
                env=dict(PP_TIERS[tier]))
    if records == "tiles":
        case.update(piece=piece, overlap=overlap)
    if records == "wrong":
        case.update(nwrong=int(rng.integers(1, 6)), wrong_seed=int(rng.integers(1 << 30)))
    return case


def _pairpaths_tiles(ora, case):
    """(records, spans per pair) of the 'tiles' kind: per pair the reference's records of the query in every piece of its
    target, merged into whole-target coordinates; the path is the reference's path in the winning piece (smallest dist,
    then smallest end, then first piece: merge_tiles' order), shifted by the piece's origin"""
    import pair_paths_ref
    import pairs_ref
    from squigglekit_amd import api
    seqs = case["seqs"]
    rec = np.zeros(len(case["pairs"]), dtype=pairs_ref.HIT)
    parts, memo = [], {}
    for p, (q, t) in enumerate(case["pairs"].tolist()):
        if (q, t) not in memo:
            x = seqs[q]
            pieces, tiling = api.tile_targets([seqs[t]], case["piece"], case["overlap"])
            per = pairs_ref.records(ora, [x] + pieces, [(0, 1 + k) for k in range(len(pieces))], "subsequence")
            merged = api.merge_tiles(per.astype(api.HIT_DTYPE).reshape(-1, 1), tiling)[0, 0]
            if np.isnan(merged["dist"]):
                sp = np.full((len(x), 2), -1, dtype=np.int32)
            else:
                win = min(range(len(pieces)), key=lambda k: (per["dist"][k], per["end"][k] + tiling["origin"][k], k))
                sp = pair_paths_ref.spans(ora, x, pieces[win], "subsequence") + np.int32(tiling["origin"][win])
                assert (sp[0, 0], sp[-1, 1]) == (merged["start"], merged["end"])
            memo[q, t] = (merged, sp)
        rec[p] = tuple(memo[q, t][0].tolist())
        parts.append(memo[q, t][1])
    return rec, parts


def _pairpaths_wrong(ora, case, rec):
    """(records, indices) of the 'wrong' kind: nwrong pairs with a distance (but never all of them) get their dist moved
    by one ulp or -- with normal draws, never with ties -- their start moved to another column of the target: in global mode any of 1 .. M - 1
    (the record no longer names the whole target), in subsequence mode a column of (start, end], which leaves the match's
    first column out of the window; the corner of that window must then differ from dist in its bits (asserted: the
    statement of the self-check, include/squigglekit_hip.h)."""
    rng = np.random.default_rng([97, case["wrong_seed"]])
    seqs, pairs = case["seqs"], case["pairs"]
    rec = rec.copy()
    good = np.flatnonzero(~np.isnan(rec["dist"]))
    count = min(case["nwrong"], good.size - 1)                 # (a good record at least stays as it is)
    which = sorted(rng.choice(good, size=count, replace=False).tolist()) if count > 0 else []
    for p in which:
        M = len(seqs[pairs[p, 1]])
        s, e = int(rec["start"][p]), int(rec["end"][p])
        move = not case["ties"] and rng.random() < 0.5 and (M >= 2 if case["mode"] == "global" else e > s)
        if move and case["mode"] == "global":
            rec["start"][p] = int(rng.integers(1, M))
        elif move:
            s2 = int(rng.integers(s + 1, e + 1))
            x, y = seqs[pairs[p, 0]], seqs[pairs[p, 1]]
            corner = ora.dtw_subsequence(x, y[s2:e + 1], want_cost=True)[3][-1, -1]
            assert np.float64(corner).tobytes() != np.float64(rec["dist"][p]).tobytes(), (p, s, s2, e)
            rec["start"][p] = s2
        else:
            rec["dist"][p] = np.nextafter(rec["dist"][p], np.inf if rng.random() < 0.5 else -np.inf)
    return rec, which


def pairpaths_plan(case, records, env=None):
    """What sk_pair_paths_run does with `records` under the switches (the case's, or `env`), restated: dict(listed =
    the pairs the LDS tier hands on, in list order; W = their windows; slab_bytes, waves as sk_last_pair_paths_tiers
    reports them; traced = (pair, N, W) of every pair that is traced).  A pair is traced when its record has a distance, no FLAG_EMPTY, 0 <= start <= end < M and, in global
    mode, names the whole target; it is listed when N ceil(W / 16) exceeds the LDS words or W exceeds PP_LDS_COLS."""
    env = case["env"] if env is None else env
    words_max = PP_LDS_WORDS
    if "SK_PATH_LDS_BYTES" in env:
        v = int(env["SK_PATH_LDS_BYTES"])
        if v >= 0 and v // 4 < PP_LDS_WORDS:
            words_max = v // 4
    listed, Ws, words, traced = [], [], [], []
    for p, (q, t) in enumerate(case["pairs"].tolist()):
        N, M, h = len(case["seqs"][q]), len(case["seqs"][t]), records[p]
        s, e = int(h["start"]), int(h["end"])
        if np.isnan(h["dist"]) or h["flags"] & 1 or s < 0 or e < s or e >= M:
            continue
        if case["mode"] == "global" and (s != 0 or e != M - 1):
            continue
        W = e - s + 1
        traced.append((p, N, W))
        if N * ((W + 15) // 16) > words_max or W > PP_LDS_COLS:
            listed.append(p)
            Ws.append(W)
            words.append(N * ((W + 15) // 16))
    if not listed:
        return dict(listed=[], W=[], slab_bytes=0, waves=0, traced=traced)
    slab_words = (2 * max(Ws) + max(words) + 1) & ~1
    budget = 1 << 30
    if "SK_PATH_SCRATCH_BYTES" in env and int(env["SK_PATH_SCRATCH_BYTES"]) > 0:
        budget = int(env["SK_PATH_SCRATCH_BYTES"])
    waves = max(1, min(budget // (slab_words * 4), PP_MAX_WAVES, len(listed)))
    return dict(listed=listed, W=Ws, slab_bytes=slab_words * 4, waves=waves, traced=traced)


def expect_pairpaths(ora, case):
    """dict(records: what the call returns as records; supplied: the records handed in, or None; off, spans; mismatches:
    the pairs the self-check must count; truth: the reference's records of the list)"""
    import pair_paths_ref
    import pairs_ref
    seqs, pairs, mode = case["seqs"], case["pairs"].tolist(), case["mode"]
    truth = pairs_ref.records(ora, seqs, pairs, mode)
    off = np.zeros(len(pairs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(seqs[q]) for q, _ in pairs])
    wrong = []
    if case["records"] == "tiles":
        supplied, parts = _pairpaths_tiles(ora, case)
        spans = np.concatenate(parts)
    else:
        woff, spans = pair_paths_ref.list_spans(ora, seqs, pairs, mode)
        assert np.array_equal(woff, off)
        supplied = None if case["records"] == "computed" else truth
        if case["records"] == "wrong":
            supplied, wrong = _pairpaths_wrong(ora, case, truth)
            spans = spans.copy()
            for p in wrong:
                spans[off[p]:off[p + 1]] = -1
    return dict(records=truth if supplied is None else supplied, supplied=supplied, off=off, spans=spans, wrong=wrong,
                mismatches=len(wrong), truth=truth)


def call_pairpaths(api, case, exp):
    """(records, span_off, spans, mismatches counted, (listed, slab_bytes, waves))"""
    sup = None if exp["supplied"] is None else exp["supplied"].astype(api.HIT_DTYPE)
    rec, off, spans = api.dtw_pairs_paths(case["seqs"], case["pairs"], case["mode"], records=sup)
    return rec, off, spans, api.last_path_mismatches(), api.last_pair_paths_tiers()


def diff_pairpaths(case, got, exp):
    import pairs_ref
    rec, off, spans, counted, tiers = got
    if not pairs_ref.same_records(rec, exp["records"].astype(rec.dtype)):
        want = exp["records"].astype(rec.dtype)
        p = next(p for p in range(len(rec)) if not pairs_ref.same_records(rec[p:p + 1], want[p:p + 1]))
        return "record of pair %d %s: got %s want %s" % (p, case["pairs"][p].tolist(), rec[p], want[p])
    if off.dtype != np.int64 or not np.array_equal(off, exp["off"]):
        return "span_off %s want %s" % (off.tolist()[:8], exp["off"].tolist()[:8])
    if spans.dtype != np.int32 or spans.shape != exp["spans"].shape:
        return "spans %s %s, want int32 %s" % (spans.dtype, spans.shape, exp["spans"].shape)
    for p in range(len(rec)):                                   # every pair
        a, b = int(off[p]), int(off[p + 1])
        if not np.array_equal(spans[a:b], exp["spans"][a:b]):
            i = int(np.flatnonzero((spans[a:b] != exp["spans"][a:b]).any(axis=1))[0])
            return "pair %d %s (record %s)%s: spans differ from row %d: got %s want %s" % (
                p, case["pairs"][p].tolist(), exp["records"][p], " [changed record]" if p in exp["wrong"] else "", i,
                spans[a + i:a + i + 3].tolist(), exp["spans"][a + i:a + i + 3].tolist())
    if counted != exp["mismatches"]:
        return "%d pairs failed the self-check, want %d %s" % (counted, exp["mismatches"], exp["wrong"])
    plan = pairpaths_plan(case, exp["records"])
    if tiers != (len(plan["listed"]), plan["slab_bytes"], plan["waves"]):
        return "tiers (listed, slab bytes, wavefronts) %s, want %s" % (tiers, (len(plan["listed"]), plan["slab_bytes"],
                                                                              plan["waves"]))
    return None


# ======================================================================================================================
# adaptive-band DTW over a pair list (sk_band.hip: k_band<K, PATHS>, K = W / 64)
# ======================================================================================================================
# lengths: the first points of a sequence, the half band h = W / 2 (cell (0, 0) sits at offset h: up to h points every cell
# is in its band), the 64-sample stream blocks and their refills (63 .. 129), the widest band and its neighbours
BAND_EDGES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257)
BAND_LONG = 4000                                 # uniform draws reach this length: 7 999 anti-diagonals in one pair
BAND_STEPS = 24_000                              # anti-diagonals the statement sweeps per case (see RANDOM_CASES_BAND.md)
BAND_POOL = 24
BAND_LIST = 40
BAND_FORMS = ("list", "flat", "device")
BAND_WAVES = (None, "1", "3", "7")               # SK_BAND_WAVES: the wavefronts of the launch, at most
BAND_KINDS = ("ties", "normal", "drift", "stall", "const", "ramps")
BAND_GUARD = 256                                 # bytes behind each output of the device form


def band_edges(W):
    return tuple(sorted(set(BAND_EDGES + (W // 2 - 1, W // 2, W // 2 + 1))))


def _band_len(rng, W):
    u = rng.random()
    if u < 0.5:
        return int(_pick(rng, band_edges(W)))
    return int(rng.integers(1, 401)) if u < 0.8 else int(rng.integers(1, BAND_LONG + 1))


def _band_unit(rng, kind, W):
    """one (query, target) of a kind of BAND_KINDS"""
    import band_ref
    if kind in ("drift", "stall"):
        return band_ref.drift_pair(rng, int(rng.integers(8, 1500)), float(rng.uniform(0.3, 0.7)), float(rng.uniform(0.1, 0.6)),
                                   int(_pick(rng, (40, 120))) if kind == "stall" else 0,
                                   int(_pick(rng, (40, 150))) if kind == "stall" else 0)
    N, M = _band_len(rng, W), _band_len(rng, W)
    if kind == "ties":
        return band_ref.ties(rng, N), band_ref.ties(rng, M)
    if kind == "const":                          # every move decision is a tie: parity alone steers the band
        v = float(_pick(rng, (0.0, 1.5, -2.0)))
        return np.full(N, v), np.full(M, v if rng.random() < 0.7 else v + 1.0)
    if kind == "ramps":                          # opposed monotone ramps
        return np.linspace(-1.0, 1.0, N), np.linspace(1.0, -1.0, M)
    return rng.normal(size=N), rng.normal(size=M)


def band_steps(N, M):
    return N + M - 1 if M else 0


def draw_band(rng):
    """A pool and a pair list for api.dtw_band: what the fuzz tool's former band leg drew (lengths up to BAND_LONG, forced
    wavefront counts, the records-only call) and more -- the call shape (W, end, with or without paths, the pool as a list,
    as (values, off) with off[0] > 0, or resident on the device), a pool of at most BAND_POOL sequences built from 1 .. 8
    (query, target) units of BAND_KINDS, a list of at most BAND_LIST entries over it (every unit, then drawn (q, t) over
    the whole pool, so a sequence is query here and target there; (i, i) pairs, a pair repeated verbatim, sometimes an
    empty target), cut to BAND_STEPS anti-diagonals over its distinct pairs and shuffled; and in a quarter of the cases
    one non-finite kind of band_ref.NONFINITE laid into a sequence of a listed pair."""
    import band_ref
    W = int(_pick(rng, band_ref.WIDTHS))
    end = _pick(rng, band_ref.ENDS)
    paths = bool(rng.random() < 0.6)
    form = _pick(rng, BAND_FORMS)
    waves = _pick(rng, BAND_WAVES)
    nunits = int(rng.integers(1, 9))
    kinds = [_pick(rng, BAND_KINDS) for _ in range(nunits)]
    seqs, pairs = [], []
    for kind in kinds:
        x, y = _band_unit(rng, kind, W)
        pairs.append((len(seqs), len(seqs) + 1))
        seqs += [x, y]
    nlive = len(seqs)                            # (every sequence so far can be a query)
    if rng.random() < 0.4:
        seqs.append(np.zeros(0))
        pairs.append((int(rng.integers(nlive)), len(seqs) - 1))
    for n in [_band_len(rng, W) for _ in range(int(rng.integers(0, BAND_POOL - len(seqs) + 1)) // 3)]:
        seqs.append(rng.normal(size=n) if rng.random() < 0.5 else np.rint(rng.normal(size=n) * 2))
    live = [k for k, s in enumerate(seqs) if len(s)]
    extra = int(rng.integers(0, BAND_LIST - len(pairs) + 1)) if rng.random() < 0.7 else 0
    pairs += list(zip(rng.choice(live, size=extra).tolist(), rng.integers(0, len(seqs), size=extra).tolist()))
    if rng.random() < 0.6:
        pairs += [(q, q) for q in rng.choice(live, size=int(rng.integers(1, 3))).tolist()]
    if rng.random() < 0.6:
        pairs.insert(int(rng.integers(len(pairs) + 1)), pairs[int(rng.integers(len(pairs)))])
    keep, seen, total = [], set(), 0             # the statement's CPU time: a pair that would pass the budget is left out
    for q, t in pairs[:BAND_LIST]:
        c = 0 if (q, t) in seen else band_steps(len(seqs[q]), len(seqs[t]))
        if keep and total + c > BAND_STEPS:
            continue
        keep.append((int(q), int(t)))
        seen.add((q, t))
        total += c
    pairs = [keep[int(i)] for i in rng.permutation(len(keep))]
    nonfinite = None
    if rng.random() < 0.25:
        nonfinite = _pick(rng, band_ref.NONFINITE)
        where = [(q, t) for q, t in pairs if len(seqs[t])] or pairs
        q, t = where[int(rng.integers(len(where)))]
        x, y = band_ref.lay_non_finite(rng, seqs[q], seqs[t], nonfinite)
        if x is not seqs[q]:
            seqs[q] = x
        else:
            seqs[t] = y
    env = {} if waves is None else {"SK_BAND_WAVES": waves}
    return dict(family="band", W=W, end=end, paths=paths, form=form, pad=int(rng.integers(1, 9)) if form != "list" else 0,
                kinds="".join(k[0] for k in kinds), nonfinite=nonfinite, nseq=len(seqs), npairs=len(pairs), steps=total,
                longest=max(band_steps(len(seqs[q]), len(seqs[t])) for q, t in pairs), seqs=seqs,
                pairs=np.array(pairs, dtype=np.int64).reshape(-1, 2), env=env)


def expect_band(ora, case):
    """dict(records, off, spans by band_ref.records; lost: pairs whose band lost the corner; mismatches: pairs with a
    target and without a path, failed walks included -- what a call with paths must count)"""
    import band_ref
    pairs = case["pairs"].tolist()
    rec, off, spans, lost = band_ref.records(case["seqs"], pairs, case["W"], case["end"])
    return dict(records=rec, off=off, spans=spans, lost=lost, mismatches=band_ref.mismatches(case["seqs"], pairs, off, spans))


def band_device_call(api, case, with_spans, nspans):
    """sk_dtw_band_dev on device buffers, the pool behind case['pad'] NaN: (records, spans [nspans, 2] or None, the
    mismatches counted, whether the bytes behind both outputs are still what was laid there)"""
    from squigglekit_amd import _lib
    L = _lib.ensure_init()
    values, off = pairs_pool_of(case)
    pr = api._as_pairs(case["pairs"])
    outs = [np.full(len(pr) * api.HIT_DTYPE.itemsize + BAND_GUARD, 0x5A, dtype=np.uint8),
            np.full(nspans * 8 + BAND_GUARD, 0x5A, dtype=np.uint8)]
    ptrs = []
    try:
        for a in [values if values.size else np.zeros(1)] + outs:
            ptrs.append(L.sk_dev_alloc(max(a.nbytes, 8)))
            _lib.check(L.sk_dev_upload(ptrs[-1], _lib.ptr(a), a.nbytes))
        _lib.check(L.sk_dtw_band_dev(ptrs[0], _lib.ptr(off), off.size - 1, _lib.ptr(pr), len(pr), case["W"],
                                     api.BAND_ENDS[case["end"]], ptrs[1], ptrs[2] if with_spans else None))
        _lib.check(L.sk_sync())
        for a, d in zip(outs, ptrs[1:]):
            _lib.check(L.sk_dev_download(_lib.ptr(a), d, a.nbytes))
    finally:
        for d in ptrs:
            L.sk_dev_free(d)
    rec = outs[0][:-BAND_GUARD].view(api.HIT_DTYPE).copy()
    spans = outs[1][:-BAND_GUARD].view(np.int32).reshape(-1, 2).copy()
    clean = bool(np.all(outs[0][-BAND_GUARD:] == 0x5A) and np.all(outs[1][-BAND_GUARD:] == 0x5A))
    if not with_spans:
        clean = clean and bool(np.all(outs[1] == 0x5A))
    return rec, (spans if with_spans else None), (int(L.sk_last_path_mismatches()) if with_spans else None), clean


def call_band(api, case, exp):
    """(records, span_off, spans, mismatches counted, api.last_band_plan(), clean) of the case's own call: span_off, spans
    and the count are None without paths; clean: nothing written behind an output of the device form"""
    if case["form"] == "device":
        rec, spans, counted, clean = band_device_call(api, case, case["paths"], int(exp["off"][-1]))
        return rec, exp["off"] if case["paths"] else None, spans, counted, api.last_band_plan(), clean
    got = api.dtw_band(pairs_pool_of(case), case["pairs"], case["W"], case["end"], paths=case["paths"])
    if not case["paths"]:
        return got, None, None, None, api.last_band_plan(), True
    return got[0], got[1], got[2], api.last_path_mismatches(), api.last_band_plan(), True


def band_slab_bytes(steps, W):
    """include/squigglekit_hip.h: one wavefront's slab for a longest pair of `steps` anti-diagonals"""
    return -(-steps * W // 1024) * 256 + -(-steps // 64) * 8 + 8


def diff_band(case, got, exp):
    import pairs_ref
    rec, off, spans, counted, plan, clean = got
    want = exp["records"]
    if rec.shape != want.shape:
        return "records shaped %s, want %s" % (rec.shape, want.shape)
    seqs, pairs = case["seqs"], case["pairs"]
    for p in range(len(want)):                                  # every pair, by the rule of pairs_ref.same_records
        if not pairs_ref.same_records(rec[p:p + 1], want[p:p + 1].astype(rec.dtype)):
            q, t = pairs[p]
            return "pair %d (%d, %d) (N=%d, M=%d): got %s want %s" % (p, q, t, len(seqs[q]), len(seqs[t]), rec[p], want[p])
    if not clean:
        return "bytes written behind an output of the device form"
    steps = case["longest"]
    slab, waves, steps_max = plan
    if steps_max != steps or slab != (band_slab_bytes(max(steps, 1), case["W"]) if case["paths"] else 0):
        return "plan (slab bytes, wavefronts, steps) %s for a longest pair of %d anti-diagonals" % (plan, steps)
    forced = case["env"].get("SK_BAND_WAVES")
    if not 1 <= waves <= min(case["npairs"], int(forced) if forced else case["npairs"]):
        return "%d wavefronts for %d pairs under SK_BAND_WAVES=%s" % (waves, case["npairs"], forced)
    if not case["paths"]:
        return None
    if off.dtype != np.int64 or not np.array_equal(off, exp["off"]):
        return "span_off %s want %s" % (off.tolist()[:8], exp["off"].tolist()[:8])
    if spans.dtype != np.int32 or spans.shape != exp["spans"].shape:
        return "spans %s %s, want int32 %s" % (spans.dtype, spans.shape, exp["spans"].shape)
    for p in range(len(want)):                                  # every pair
        a, b = int(off[p]), int(off[p + 1])
        if not np.array_equal(spans[a:b], exp["spans"][a:b]):
            i = int(np.flatnonzero((spans[a:b] != exp["spans"][a:b]).any(axis=1))[0])
            return "pair %d %s (record %s): spans differ from row %d: got %s want %s" % (
                p, pairs[p].tolist(), want[p], i, spans[a + i:a + i + 3].tolist(), exp["spans"][a + i:a + i + 3].tolist())
    if counted != exp["mismatches"]:
        return "%s pairs counted without a path, want %d (%d of them lost the corner)" % (counted, exp["mismatches"],
                                                                                         exp["lost"])
    return None


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
    if isinstance(got, (int, np.integer)):
        return b"%d" % int(got)
    return b"|".join(result_bytes(g) for g in got)


DRAW = dict(sweep=draw_sweep, hits=draw_hits, paths=draw_paths, pull=draw_pull, panel=draw_panel, detect=draw_detect,
            hmm=draw_hmm, levels=draw_levels, screen=draw_screen, drna=draw_drna, roll=draw_roll, pairs=draw_pairs,
            pairpaths=draw_pairpaths, band=draw_band, hmmpost=draw_hmmpost)
EXPECT = dict(sweep=expect_sweep, hits=expect_hits, paths=expect_paths, pull=expect_pull, segment=expect_plain,
              motifseq=expect_plain, pa=expect_plain, panel=expect_panel, detect=expect_detect, hmm=expect_hmm,
              levels=expect_levels, background=expect_background, events=expect_events, screen=expect_screen,
              drna=expect_drna, roll=expect_roll, pairs=expect_pairs, pairpaths=expect_pairpaths, band=expect_band,
              hmmpost=expect_hmmpost)
CALL = dict(sweep=call_sweep, hits=call_hits, paths=call_paths, pull=call_pull, segment=call_plain, motifseq=call_plain,
            pa=call_plain, panel=call_panel, detect=call_detect, hmm=call_hmm, levels=call_levels,
            background=call_background, events=call_events, screen=call_screen, drna=call_drna, roll=call_roll,
            pairs=call_pairs, pairpaths=call_pairpaths, band=call_band, hmmpost=call_hmmpost)
DIFF = dict(sweep=diff_sweep, hits=diff_hits, paths=diff_paths, pull=diff_pull, segment=diff_plain, motifseq=diff_plain,
            pa=diff_plain, panel=diff_panel, detect=diff_detect, hmm=diff_hmm, levels=diff_levels,
            background=diff_background, events=diff_events, screen=diff_screen, drna=diff_drna, roll=diff_roll,
            pairs=diff_pairs, pairpaths=diff_pairpaths, band=diff_band, hmmpost=diff_hmmpost)
TWIN_OF = dict(background="hits", events="paths")

# ---- the interleaved sequence (tests/test_gpu_random.py::test_interleaved_calls_share_the_context_buffers) --------
# (family, seed): committed cases by their seeds, the older calls by draw_plain seeds.  Filled beside SEEDS.
INTERLEAVE = [("paths", 50), ("sweep", 97), ("pull", 0), ("hits", 1), ("paths", 50), ("segment", 3), ("sweep", 22),
              ("motifseq", 2), ("pull", 21), ("paths", 12), ("pa", 3), ("hits", 324), ("sweep", 16), ("pull", 0),
              ("motifseq", 0), ("paths", 187), ("hits", 1), ("segment", 0), ("sweep", 97), ("paths", 29), ("pull", 3),
              ("pa", 2), ("hits", 214), ("sweep", 60), ("paths", 12), ("motifseq", 2)]


# the second sequence: the newer families (panel, detect, hmm, levels) and the two twins between the older calls; at its
# end three screening calls (one of them twice, several chunks, the hint, two motifs on different L) between calls of
# other families, so that the screening scheme's buffers are used again after those have grown the shared ones
INTERLEAVE2 = [("panel", 4), ("hmm", 3), ("detect", 4), ("background", 1), ("sweep", 97), ("levels", 13), ("panel", 29),
               ("events", 50), ("hmm", 35), ("pull", 0), ("detect", 27), ("panel", 4), ("hits", 1), ("levels", 22),
               ("hmm", 3), ("paths", 12), ("detect", 6), ("background", 324), ("panel", 36), ("segment", 3), ("levels", 13),
               ("events", 12), ("hmm", 10), ("detect", 4), ("motifseq", 2), ("panel", 93), ("screen", 268),
               ("levels", 22), ("screen", 337), ("hits", 1), ("screen", 268)]


# the third sequence: the two branches of the dRNA segmenter between segmenter, levels, hit-list and detector calls -- of
# each branch a large case before a small one (257 reads of 4 000 000 samples before 65 two-level reads; rows of 134 000
# samples on the two-kernel path before rows of 650), cases that come twice, the per-sample switches between them
INTERLEAVE3 = [("drna", 1), ("segment", 3), ("roll", 0), ("levels", 13), ("drna", 39), ("hits", 1), ("roll", 2),
               ("detect", 4), ("drna", 14), ("segment", 0), ("roll", 10), ("drna", 39), ("levels", 22), ("roll", 2),
               ("hits", 324), ("drna", 0), ("roll", 16), ("detect", 27), ("drna", 54), ("roll", 0), ("segment", 3),
               ("drna", 1), ("roll", 1), ("drna", 15)]


# the fourth sequence: pair lists and their warping paths between calls of the families whose buffers and counters they
# share -- sk_pairpath.hip lays an 8-word list header into c->pathlist where sk_path.hip lays 2, both count into
# c->pathcnt and take slabs of c->pathscratch, and a pair call resets the retry and profile state the screening scheme's
# counters are read through.  A large case of each kind before a small one (pairs 9: 202 pairs, 19.6 M cells, before
# pairs 130: 19 pairs; pairpaths 145: 204 pairs, every one listed, before pairpaths 22: 5 pairs), cases that come twice,
# the all-listed pairpaths 145 directly before and after paths 1, which puts every hit into its own scratch tier, and
# pairpaths 13 -- four records changed, four mismatches counted -- directly before a paths call that must count none
INTERLEAVE4 = [("pairs", 9), ("paths", 12), ("pairpaths", 145), ("paths", 1), ("pairpaths", 145), ("events", 50),
               ("pairs", 130), ("hits", 1), ("pairpaths", 22), ("screen", 268), ("pairs", 119), ("segment", 3),
               ("pairpaths", 13), ("paths", 187), ("pairpaths", 1), ("screen", 337), ("pairs", 9), ("events", 12),
               ("pairpaths", 17), ("hits", 324), ("pairs", 130), ("screen", 268), ("pairpaths", 22), ("segment", 0),
               ("pairs", 5), ("paths", 1), ("pairpaths", 36)]


# the fifth sequence: band lists between pair lists, their warping paths and hit lists.  sk_band_run counts into c->pathcnt
# through sk_path_begin, as sk_pairpath.hip and sk_path.hip do, and keeps a table and slabs of its own that only grow:
# pairpaths 13 (four mismatches counted) directly before band 54 (none), band 331 (one walk that fails) and band 27
# (three lost pairs) directly before pairpaths 7 and pairs 130 (none), the widest slabs (band 44: 256 cells, 4 875
# anti-diagonals) before a list of one pair of 205 (band 351) and again after it, cases that come twice
INTERLEAVE5 = [("band", 44), ("pairpaths", 13), ("band", 54), ("hits", 1), ("band", 351), ("pairs", 130), ("band", 331),
               ("pairpaths", 7), ("band", 297), ("hits", 324), ("band", 44), ("pairs", 5), ("band", 27), ("pairs", 130),
               ("band", 75), ("pairpaths", 13), ("band", 351), ("hits", 1), ("band", 331)]


# the sixth sequence: posterior calls between Viterbi, detector, levels, pair-list and band calls.  c->hmm holds the
# records of both HMM calls (with the calibration pairs behind them), c->hmmpost and c->hmmpostout only grow, c->sig / len /
# off are everyone's: the largest case (hmmpost 305: a list of 200 reads, 165 258 samples) before a call of one read of 33
# samples (hmmpost 427), hmmpost 185 -- four slices of one group under SK_HMM_SCRATCH_MB=1 -- directly after hmm 35, whose
# state-path call takes three slices of the same budget, cases that come twice
INTERLEAVE6 = [("hmmpost", 305), ("detect", 4), ("hmmpost", 427), ("hmm", 35), ("hmmpost", 185), ("levels", 13),
               ("hmmpost", 68), ("pairs", 130), ("hmmpost", 2), ("band", 351), ("hmmpost", 185), ("hmm", 3),
               ("hmmpost", 427), ("detect", 27), ("hmmpost", 34)]


def interleave_case(family, seed):
    if family in SEEDS:
        return case_of(family, seed)
    if family in TWIN_OF:
        return twin_case(family, case_of(TWIN_OF[family], seed))
    case = draw_plain(np.random.default_rng([99, ["segment", "motifseq", "pa"].index(family), int(seed)]), family)
    case["seed"] = int(seed)
    return case
