#!/usr/bin/env python3
"""Randomised GPU-vs-oracle sweep over shapes the unit tests do not pin: random read counts, ragged
lengths, strides, outlier limits, segmenter parameters; the segment levels of every
segmenter round against plain numpy; and, per round, one drawn case of every family of tests/randcases.py -- the
screening scheme of MotifSeq's first match under its switches, the segmenter sweep, the MotifSeq hit lists, the alignment paths, SquigglePull's text, the region + motif panel, event detection, the
signal HMM with its state paths, segment levels, both branches of the dRNA segmenter, and the background and events twins of
the hit family, DTW over a pair list, the warping paths of one and the adaptive-band DTW of one -- each against the
reference tests/test_gpu_random.py uses; and one MotifSeq session (random motif lengths, slot count, cuts, calibration
length, limits, both scale modes and lane layouts) against the prefix statement of tests/stream_ref.py; and one
mapping session (tests/mapstream_ref.draw_session: random targets, slot count, subsets, cuts up to 2 100 points, resets and peeks, both lane layouts) against the oracle on every slot's
concatenation after every push; and one event session (tests/evstream_ref.draw_session: random parameters, slot
count, reads of four kinds, cuts, subsets, ENDs and resets) against its statement on detect_ref after every push and
against the one-shot call on every ended read; and one hit-list round (tests/pair_hits_ref.py: a drawn pair list with its
K, max_dist and row budget, and a drawn session script whose hits() are read after every push) against the statement
there; and one posterior round (the `hmmpost` family of tests/randcases.py: draw_hmm's models, reads of up to 2 600
samples, feeds, outputs and switches, SK_HMM_POST_BLOCK among them) against tests/hmm_post_ref.py, every double by its bits; and one
filtered HMM session (hmmstream_ref.draw_session's script on a drawn model, beside a plain session) against
tests/hmmfilter_ref.py after every push, every double by its bits.  The DTW pair
lists, their warping paths and the adaptive band are three of the families of tests/randcases.py (`pairs`, `pairpaths`,
`band`: the draws that used to live here, against tests/pairs_ref.py, tests/pair_paths_ref.py and tests/band_ref.py).

    python tools/fuzz_gpu.py [seconds=120] [seed=1]

Prints one line per mismatch and exits non-zero if there was any.  (Test infrastructure.)"""
import os
import sys
import time

import numpy as np

os.environ["SK_TUNING"] = "1"      # this tool flips tuning switches

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))        # the seeded case generators and their references
import randcases                                      # noqa: E402
import stream_ref                                     # noqa: E402
import mapstream_ref                                  # noqa: E402
import evstream_ref                                   # noqa: E402
import pair_hits_ref                                  # noqa: E402
import hmmstream_ref                                  # noqa: E402
import hmmfilter_ref                                  # noqa: E402
from squigglekit_amd import api, synth               # noqa: E402
from squigglekit_amd._lib import SegParams           # noqa: E402
from oracle import oracle as ora                      # noqa: E402


def session_round(rng):
    """One drawn MotifSeq session: every record of every push (and of the closing flush) against
    stream_ref.record on the samples pushed so far.  Returns None, or what differed."""
    K = int(rng.integers(1, 4))
    Ns = [int(rng.choice([1, 2, 16, 17, 31, 32, 33, 64, 65, 256, 257, 1024])) if rng.random() < 0.4
          else int(rng.integers(1, 600)) for _ in range(K)]
    nslots, W = int(rng.integers(1, 12)), int(rng.choice([1, 2, 17, 100, 500, 2000]))
    lo, hi = [(0, 1200), (0, 900), (-50, 2500), (400, 650)][int(rng.integers(4))]
    mode = ["medmad", "zscale"][int(rng.integers(2))]
    n = int(rng.integers(1, 2500))
    no_small = rng.random() < 0.5
    desc = "K=%d N=%s slots=%d W=%d lo=%d hi=%d %s n=%d no_small=%s" % (K, Ns, nslots, W, lo, hi, mode, n, no_small)
    if no_small:
        os.environ["SK_DTW_NO_SMALL"] = "1"
    motifs = [synth.synthetic_motif(N, seed=int(rng.integers(1000))) for N in Ns]
    sig = synth.squiggle_batch(nslots, n, int(rng.integers(1 << 30)))
    k = int(rng.integers(0, 60))
    sig[rng.integers(0, nslots, k), rng.integers(0, n, k)] = rng.choice([-9, 0, 899, 900, 1199, 1200, 3000], k)
    raw = [np.zeros(0, dtype=np.int16) for _ in range(nslots)]
    at = [0] * nslots
    try:
        with api.MotifStream(motifs, nslots, mode, lo, hi, calib=W) as ms:
            for final in (False, True):
                while not final and min(at) < n:
                    live = [s for s in range(nslots) if at[s] < n and rng.random() < 0.7]
                    chunks = []
                    for s in live:
                        c = min(int(rng.choice([0, 1, 2, 15, 16, 17, 63, 64, 65, 200, 1000])), n - at[s])
                        chunks.append(sig[s, at[s]:at[s] + c])
                        raw[s] = np.concatenate([raw[s], chunks[-1]])
                        at[s] += c
                    if not live:
                        continue
                    rec = ms.push(live, chunks)
                    for kk in range(K):
                        for i, s in enumerate(live):
                            want = stream_ref.record(raw[s], motifs[kk], W, mode, lo, hi, False)
                            if not stream_ref.same(stream_ref.fields(rec[kk, i]), want):
                                return "%s: slot %d motif %d after %d samples: got %s want %s" % (
                                    desc, s, kk, len(raw[s]), stream_ref.fields(rec[kk, i]), want)
                if final:
                    rec = ms.flush(list(range(nslots)))
                    for kk in range(K):
                        for s in range(nslots):
                            want = stream_ref.record(raw[s], motifs[kk], W, mode, lo, hi, True)
                            if not stream_ref.same(stream_ref.fields(rec[kk, s]), want):
                                return "%s: slot %d motif %d after the flush: got %s want %s" % (
                                    desc, s, kk, stream_ref.fields(rec[kk, s]), want)
    finally:
        os.environ.pop("SK_DTW_NO_SMALL", None)
    return None


def mapstream_round(rng):
    """One drawn mapping session against the oracle on the concatenation.  Returns None, or what differed."""
    case = mapstream_ref.draw_session(rng)
    no_small = rng.random() < 0.5
    if no_small:
        os.environ["SK_DTW_NO_SMALL"] = "1"
    try:
        msg = mapstream_ref.run_session(api, ora, case)
    finally:
        os.environ.pop("SK_DTW_NO_SMALL", None)
    return None if msg is None else "no_small=%s %s: %s" % (no_small, mapstream_ref.describe_session(case), msg)


def pairhits_round(rng):
    """One drawn pair list and one drawn session script through the hit lists.  Returns None, or what differed."""
    msg = pair_hits_ref.run_pairs_case(api, ora, pair_hits_ref.draw_pairs_case(rng), os.environ)
    if msg is not None:
        return "pair list: " + msg
    msg = pair_hits_ref.run_session_case(api, pair_hits_ref.draw_session_case(rng))
    return None if msg is None else "session: " + msg


def hmm_post_round(rng):
    """One drawn posterior call -- randcases.DRAW["hmmpost"] with the running generator: the family the suite's committed
    seeds come from -- against tests/hmm_post_ref.py through randcases.diff_hmmpost, every double by its bits; then the
    complementary call (the other outputs, the other k_hmm_bwd).  Returns None, or what differed."""
    case = randcases.DRAW["hmmpost"](rng)
    exp = randcases.EXPECT["hmmpost"](ora, case)
    for key in randcases.SWITCHES:
        os.environ.pop(key, None)
    os.environ.update(case["env"])
    try:
        for c in (case, dict(case, counts=not case["counts"], dense=not case["dense"])):
            msg = randcases.DIFF["hmmpost"](c, randcases.CALL["hmmpost"](api, c, exp), exp)
            if msg is not None:
                return "%s counts=%s dense=%s: %s" % (randcases.describe(case), c["counts"], c["dense"], msg)
    finally:
        for key in case["env"]:
            os.environ.pop(key, None)
    return None


def hmmfilter_round(rng):
    """One drawn filtered HMM session (hmmstream_ref.draw_session: slot count, subsets, cuts, both feeds, resets with and
    without calibration pairs; a drawn tie model or a preset) beside a plain one: after every push the records of both and
    the filter against tests/hmmfilter_ref.py, bit for bit.  Returns None, or what differed."""
    kind = int(rng.integers(3))
    if kind == 0:
        model, draw = hmmstream_ref.tie_model(rng), lambda r, n: r.integers(0, 4, n).astype(np.int16)
    else:
        model, draw = api.polya_model(("synth_raw", "rna_pa")[kind - 1]), lambda r, n: r.integers(380, 620, n).astype(np.int16)
    nslots = int(rng.integers(1, 200))
    sess = hmmstream_ref.draw_session(rng, nslots=nslots, budget=150 * nslots, maxlen=int(rng.integers(1, 200)), draw_chunk=draw)
    try:
        hmmfilter_ref.play_session(api, model, sess, "%d slots" % nslots)
    except AssertionError as e:
        return "%s model: %s" % (("tie", "synth_raw", "rna_pa")[kind], str(e)[:600])
    return None


def evstream_round(rng):
    """One drawn event session: every push against evstream_ref.run_session, every ended read against the one-shot call,
    no guard hit.  Returns None, or what differed."""
    sess = evstream_ref.draw_session(rng)
    try:
        evstream_ref.play_session(api, sess, "fuzz")
    except AssertionError as e:
        return str(e)[:3000]
    return None


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    t_end = time.time() + budget
    bad = rounds = 0
    while time.time() < t_end:
        rounds += 1
        R = int(rng.choice([1, 3, 64, 255, 256, 300, 700, 1100]))
        M = int(rng.choice([8, 63, 512, 1000, 2047, 4000, 4001, 6000]))
        sig = synth.squiggle_batch(R, M, int(rng.integers(1 << 30)))
        if rng.random() < 0.3:
            sig = np.clip(sig, 300, 700).astype(np.int16)
        elif rng.random() < 0.3 and M >= 512:
            sig = synth.pattern_reads(rng, R, M)          # in-band masks built to defeat the jumping walk (round 4)
        k = int(rng.integers(0, 40))
        sig[rng.integers(0, R, k), rng.integers(0, M, k)] = rng.choice([-9, 0, 899, 900, 1199, 1200, 3000], k)
        lens = rng.integers(0, M + 1, R).astype(np.int32)
        lens[rng.integers(0, R)] = M
        # ---- MotifSeq ----
        # randcases.DRAW["screen"] with this tool's generator: one int16 first-match call of 256 reads and more through
        # the screening scheme -- every rows-per-lane instantiation of its kernels can come up (8 and 16 lanes x 1..32
        # rows, 64 x 1..16), with the start hint forced on, forced off or left to its gate, the checkpoint distance, the
        # sorted window order, several chunks, the fused / separate filter + statistics, the early / late exact retry,
        # second windows, both scalings, four limit pairs, a stride beyond the longest row, one to three motifs on
        # different lane layouts -- against the oracle, byte for byte
        case = randcases.DRAW["screen"](rng)
        for key in randcases.SWITCHES:
            if key in case["env"]:
                os.environ[key] = case["env"][key]
            else:
                os.environ.pop(key, None)
        exp = randcases.EXPECT["screen"](ora, case)
        mgot = randcases.CALL["screen"](api, case, exp)
        for key in randcases.SWITCHES:
            os.environ.pop(key, None)
        for N, got, want in zip(case["Ns"], mgot, exp["want"]):
            ok = randcases.screen_compared(got, want)           # MAD == 0 / std == 0 rows aside
            nan = np.isnan(got["dist"]) & np.isnan(want["dist"])
            same = (got["start"] == want["start"]) & (got["end"] == want["end"]) & (got["n"] == want["n"]) & \
                   ((got["dist"] == want["dist"]) | nan)
            if not np.all(same[ok]):
                bad += 1
                r = int(np.nonzero(~same & ok)[0][0])
                print("MOTIFSEQ mismatch R=%d M=%d N=%d %s lo=%d hi=%d QL=%s read %d: got %s want %s"
                      % (case["R"], case["stride"], N, case["scale"], case["lo"], case["hi"], case["ql"], r, got[r], want[r]))
                print("  %s" % randcases.describe(case))
        guard = api.last_dtw_guard()
        if any(guard[k] for k in ("premise_violations", "audit_mismatches", "alarm", "exact_fallback")):
            bad += 1
            print("MOTIFSEQ guard counters not all zero round %d %s: %s" % (rounds, randcases.describe(case), guard))
        # ---- segmenter ----
        # (round 4: the default walk jumps between stretches of quiet mask entries, k_seg_walk4 -- window >= 127 and
        # error < min(corrector, 32) take it, with the statistics kernel's hints up to 4 096 samples and a pass of its
        # own beyond or under SK_WALK_OWNPASS; the other draws take the older walks)
        kw = [dict(), dict(error=10, corrector=3), dict(window=20, seg_dist=5), dict(std_scale=1.5, stall_len=0.9),
              dict(lim_low=300, lim_hi=800), dict(error=3), dict(window=127, stall_len=0.05), dict(error=0, seg_dist=0),
              dict(window=400, error=8, corrector=20), dict(std_scale=0.4, stall_len=1.2)][int(rng.integers(10))]
        if rng.random() < 0.25:
            os.environ["SK_WALK_OWNPASS"] = "1"
        p = SegParams(**kw)
        segs, nsegs = api.segment_batch(sig, lens, p, max_segs=64)
        okw = {a: b for a, b in kw.items() if a not in ("lim_low", "lim_hi")}
        osegs, onsegs = ora.segment_batch_i16(sig, lens, ora.SegParams(**okw), lo=p.lim_low, hi=p.lim_hi,
                                              max_segs=segs.shape[1])
        if not np.array_equal(nsegs, onsegs) or any(
                not np.array_equal(segs[r, :nsegs[r]], osegs[r, :nsegs[r]]) for r in range(R)):
            bad += 1
            print("SEGMENTER mismatch R=%d M=%d %s ownpass=%s" % (R, M, kw, os.environ.get("SK_WALK_OWNPASS")))
        # ---- segment levels: the same call with its records, against plain numpy on the oracle's segments ----
        s2, n2, lv, rl = api.segment_levels_batch(sig, lens, p, max_segs=segs.shape[1])
        if not np.array_equal(n2, nsegs) or not np.array_equal(s2, segs):
            bad += 1
            print("LEVELS segs differ from segment_batch R=%d M=%d %s" % (R, M, kw))
        else:
            want = randcases.levels_expected(lv.dtype, [sig[r, :lens[r]] for r in range(R)],
                                             [osegs[r, :onsegs[r]] for r in range(R)], lv.shape, p.lim_low, p.lim_hi)
            why = randcases.levels_mismatch(lv, rl, *want)
            if why:
                bad += 1
                print("LEVELS mismatch R=%d M=%d %s: %s" % (R, M, kw, why))
        os.environ.pop("SK_WALK_OWNPASS", None)
        # ---- float64 reads (pA-like), per-read oracle composition ----
        # (round 4: reads of up to 4 096 samples take the streaming statistics kernel, sk_f64stat.hip -- histogram median,
        # certified comparisons, numpy-order redo list; longer ones, and everything under SK_F64_OLD, the numpy-order
        # kernel.  Drawn per round: the data kind, segmenter parameters and limits, the certification margin blown up so
        # that every read takes the redo, the old kernel, and once in a while a read too long for the streaming path.)
        kinds = int(rng.integers(6))
        freads = []
        for _ in range(int(rng.choice([1, 3, 12, 70, 300]))):
            n = int(rng.choice([1, 2, 5, 63, 64, 65, 257, 1500, 4000, 4095, 4096]))
            if kinds == 0:
                x = np.round(rng.normal(90.0, 14.0, n), 1)                      # 0.1 pA steps: many ties
            elif kinds == 1:
                x = rng.normal(90.0, 14.0, n)
            elif kinds == 2:
                x = 500.0 + rng.integers(0, 3, n) * 2.0 ** -40                  # near constant
            elif kinds == 3:
                x = np.exp(rng.normal(4.0, 1.0, n))
            elif kinds == 4:                                                    # SquigglePull's pA image of a squiggle
                x = np.round((synth.squiggle_batch(1, n, int(rng.integers(1 << 30)))[0].astype(np.int64) + 16.0)
                             * (1493.94 / 8192.0), 2)
            else:                                                               # gridded, a far outlier, NaN / inf inside
                x = np.round(rng.normal(96.0, 9.0, n), 2)
                x[rng.integers(0, n)] = rng.choice([899.99, 0.01, np.nan, np.inf, -np.inf, 1199.0])
            freads.append(x)
        if rng.random() < 0.25:
            # a longer read decides the batch's kernel: the workgroup-per-read one (4 / 8 / 12 wavefronts by length, round 5),
            # the window-by-window one under SK_F64_LONG_LOOKS or beyond 41 472 samples
            top = int(rng.choice([9000, 10240, 12000, 20480, 30000, 41472, 45000]))
            freads.append(np.round(rng.normal(96.0, 15.0, int(rng.integers(4097, top + 1))), 2))
            if rng.random() < 0.5:
                freads.append(rng.normal(96.0, 15.0, int(rng.integers(4097, top + 1))))
        for key, val in (("SK_F64_OLD", "1" if rng.random() < 0.15 else None),
                         ("SK_F64_LONG_LOOKS", "1" if rng.random() < 0.2 else None),
                         ("SK_SEG_DELTA_SCALE", "1e13" if rng.random() < 0.2 else None)):
            if val is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = val
        fm = synth.synthetic_motif(int(rng.choice([3, 50, 163])), seed=int(rng.integers(1000)))
        fscale = ["medmad", "zscale"][int(rng.integers(2))]
        flo, fhi = [(0, 1200), (0, 900), (60, 130), (-1000, 1000)][int(rng.integers(4))]
        fgot = api.motifseq_reads_f64(freads, fm, scale=fscale, scale_low=flo, scale_hi=fhi)
        for i, x in enumerate(freads):
            f = ora.scale_outliers(x, flo, fhi)
            if f.size == 0:
                if not (fgot["flags"][i] & 1):
                    bad += 1
                    print("F64 empty read not flagged, kind %d" % kinds)
                continue
            y = ora.medmad(f)[0] if fscale == "medmad" else ora.zscale(f)[0]
            if not np.all(np.isfinite(y)):
                continue                                                         # MAD == 0: flagged, not compared
            d, s0, e0 = ora.dtw_subsequence(fm, y)
            if (fgot["dist"][i], fgot["start"][i], fgot["end"][i], fgot["n"][i]) != (d, s0, e0, f.size):
                bad += 1
                print("F64 mismatch kind %d %s n=%d lo=%d hi=%d: got %s want %s" % (kinds, fscale, len(x), flo, fhi, fgot[i], (d, s0, e0)))
        fkw = [dict(), dict(error=10, corrector=3), dict(window=20, seg_dist=5), dict(std_scale=0.2, stall_len=0.9),
               dict(lim_low=60, lim_hi=130), dict(std_scale=-0.3)][int(rng.integers(6))]
        fp = SegParams(**fkw)
        fokw = {a: b for a, b in fkw.items() if a not in ("lim_low", "lim_hi")}
        fsegs = api.segment_reads_f64(freads, fp)
        for x, gsegs in zip(freads, fsegs):
            f = ora.scale_outliers(x, fp.lim_low, fp.lim_hi)
            wsegs = ora.get_segs(f, ora.SegParams(**fokw)) if f.size else False
            if gsegs != wsegs:
                bad += 1
                print("F64 SEGMENTER mismatch kind %d n=%d %s" % (kinds, len(x), fkw))
        os.environ.pop("SK_F64_OLD", None)
        os.environ.pop("SK_F64_LONG_LOOKS", None)
        os.environ.pop("SK_SEG_DELTA_SCALE", None)
        # ---- round 6: raw rows through the pA conversion in the RAW domain (k_seg_stats<.., PA> / k_seg_stats_wg), the
        # wavefront-per-read walk, centi-unit batches -- against the oracle on the float64 values numpy makes the reference's way
        # (segmenter.py:345-349, :385) ----
        if rounds % 2 == 1:
            Rp = int(rng.choice([1, 5, 64, 200]))
            Mp = int(rng.choice([8, 512, 4000, 4096, 4104, 9000, 16384, 20000, 33000, 50000, 66000]))
            Sp = (Mp + 7) // 8 * 8
            praw = synth.squiggle_batch(Rp, Sp, int(rng.integers(1 << 30)))
            kind = int(rng.integers(5))
            if kind == 1:                                         # PromethION-like: raw window starts high
                praw = np.clip(np.rint(praw * 0.6 + 237), -32768, 32767).astype(np.int16)
            elif kind == 2 and Mp >= 512:
                praw = synth.pattern_reads(rng, Rp, Sp)
            elif kind == 3:                                       # spikes: kept ones above the window, dropped ones, negatives
                k2 = int(rng.integers(1, 60))
                praw[rng.integers(0, Rp, k2), rng.integers(0, Sp, k2)] = rng.choice([2500, 3000, 6000, 32767, -5, -300], k2)
            plens = rng.integers(0, Mp + 1, Rp).astype(np.int32)
            plens[rng.integers(0, Rp)] = Mp
            cal = np.empty((Rp, 3))
            cal[:, 0] = rng.choice([8192.0, 2048.0, 4096.0], Rp)
            cal[:, 1] = np.round(rng.uniform(-250, 40, Rp), 1) if kind == 1 else np.round(rng.uniform(-40, 40, Rp), 1)
            cal[:, 2] = rng.uniform(600, 1600, Rp)
            if rng.random() < 0.2:
                cal[rng.integers(0, Rp)] = [[8192.0, 16.0, 8192.0 * 5], [8192.0, 16.0, -1493.94], [8192.0, np.nan, 1493.94],
                                            [8192.0, 16.0, 8192.0 * 0.012]][int(rng.integers(4))]
            pkw = [dict(), dict(lim_low=60, lim_hi=140), dict(std_scale=0.3), dict(window=40, error=2), dict(error=40, corrector=10),
                   dict(lim_low=-50, lim_hi=2000), dict(std_scale=2.5, stall_len=0.9)][int(rng.integers(7))]
            for key, val in (("SK_SEG_DELTA_SCALE", "1e13" if rng.random() < 0.15 else None),
                             ("SK_WALK_NOWAVE", "1" if rng.random() < 0.3 else None),
                             ("SK_SEG_WG_ALL", "1" if rng.random() < 0.4 else None),
                             ("SK_SEG_NO_WG", "1" if rng.random() < 0.2 else None)):
                if val is None:
                    os.environ.pop(key, None)
                else:
                    os.environ[key] = val
            pp = SegParams(**pkw)
            psegs, pn = api.segment_batch_pa(praw, plens, cal, pp)
            opp = ora.SegParams(**{a: b for a, b in pkw.items() if a not in ("lim_low", "lim_hi")})
            for r in range(Rp):
                unit = float("{0:.2f}".format(cal[r, 2])) / cal[r, 0]
                pa = np.round((praw[r, :plens[r]].astype(np.int64) + cal[r, 1]) * unit, 2)
                f = ora.scale_outliers(pa, pp.lim_low, pp.lim_hi)
                w = (ora.get_segs(f, opp) or []) if f.size else []
                if psegs[r, :pn[r]].tolist() != w:
                    bad += 1
                    print("PA mismatch R=%d M=%d kind %d read %d cal %s %s env %s" % (Rp, Mp, kind, r, cal[r].tolist(), pkw,
                          {k: os.environ.get(k) for k in ("SK_SEG_DELTA_SCALE", "SK_WALK_NOWAVE", "SK_SEG_WG_ALL", "SK_SEG_NO_WG")}))
                    break
            # the same rows as --raw_signal input (int16 route) through the same kernel choices
            if Mp <= 50000:
                isegs, inn = api.segment_batch(praw, plens, SegParams(**{a: b for a, b in pkw.items() if a not in ("lim_low", "lim_hi")}), max_segs=64)
                osegs2, onn2 = ora.segment_batch_i16(praw, plens, opp, lo=0, hi=900, max_segs=isegs.shape[1])
                if not np.array_equal(inn, onn2) or any(not np.array_equal(isegs[r, :inn[r]], osegs2[r, :inn[r]]) for r in range(Rp)):
                    bad += 1
                    print("LONG I16 SEGMENTER mismatch R=%d M=%d kind %d %s" % (Rp, Mp, kind, pkw))
            for key in ("SK_SEG_DELTA_SCALE", "SK_WALK_NOWAVE", "SK_SEG_WG_ALL", "SK_SEG_NO_WG"):
                os.environ.pop(key, None)
            # centi-unit batch == float64 batch of the same tokens (both tools)
            cn = [rng.integers(-2000, 120000, int(rng.choice([1, 50, 3000, 4097]))).astype(np.int32) for _ in range(int(rng.choice([1, 7, 40])))]
            cflat = np.concatenate(cn)
            coff = np.concatenate([[0], np.cumsum([c.size for c in cn])]).astype(np.int64)
            ca, cb = api.segment_ragged_f64(cflat, coff), api.segment_ragged_f64(cflat / 100.0, coff)
            cm = synth.synthetic_motif(int(rng.choice([5, 60])), seed=3)
            ha, hb = api.motifseq_multi_ragged_f64(cflat, coff, [cm]), api.motifseq_multi_ragged_f64(cflat / 100.0, coff, [cm])
            if not (np.array_equal(ca[0], cb[0]) and np.array_equal(ca[1], cb[1]) and ha[0].tobytes() == hb[0].tobytes()):
                bad += 1
                print("CENTI mismatch: %d reads" % len(cn))
        # ---- dRNA_segmenter: both branches, randcases.DRAW["drna"] / DRAW["roll"] with this tool's generator ----
        # (read counts up to 257 over several wavefronts, batch routes with odd and padded strides, every statistics route and
        # both scans of the slow5 branch, two-level reads with drawn and crafted band masks; the three routes of the rolling
        # branch, windows up to 65 536 and rows above 2^17 samples) against the oracle through EXPECT / CALL / DIFF, under a
        # drawn switch
        if rounds % 2 == 0:
            for fam, line, switches in (
                    ("drna", "DRNA mismatch", (None, None, None, None, ("SK_DRNA_STEP", "1"))),
                    ("roll", "DRNA ROLL mismatch", (None, None, None, None, None, None, ("SK_ROLL_TWO_KERNELS", "1"),
                                                    ("SK_ROLL_ONE_LOOK", "1"), ("SK_ROLL_DELTA_SCALE", "1e13"),
                                                    ("SK_DRNA_STEP", "1")))):
                case = randcases.DRAW[fam](rng)
                sw = switches[int(rng.integers(len(switches)))]
                for key in randcases.SWITCHES:
                    os.environ.pop(key, None)
                if sw:
                    os.environ[sw[0]] = sw[1]
                exp = randcases.EXPECT[fam](ora, case)
                msg = randcases.DIFF[fam](case, randcases.CALL[fam](api, case, exp), exp)
                if msg is not None:
                    bad += 1
                    print("%s round %d %s switch=%s: %s" % (line, rounds, randcases.describe(case), sw, msg))
                for key in randcases.SWITCHES:
                    os.environ.pop(key, None)
        # ---- tests/randcases.py's draws with this tool's running generator, against the same references as
        # tests/test_gpu_random.py: the sweep (the oracle per (set, read)), the hit lists (reference_hits), the paths
        # (reference_paths), pull (numpy_pull_text), the panel (reference_panel), event detection (detect_ref), the signal
        # HMM with its state paths (hmm_ref, hmm_path_ref), segment levels (numpy on the oracle's segments); then a
        # hit-list draw through the background twin (numpy on the oracle's last row, test_background_host.py) and a paths
        # draw through the events twin with pooling (test_events_host.py); then a DTW pair list (pairs_ref.records) and the
        # warping paths of one (pair_paths_ref.list_spans; mismatch count and tiers as the case's plan says), then an
        # adaptive-band list (its statement's records, spans and mismatch count; with paths or records only, host or device
        # form and wavefront count as drawn).  A mismatch line carries the round, so
        # `fuzz_gpu.py <seconds> <seed>` up to that round rebuilds the case, and the drawn parameters and switches.
        for fam in ("sweep", "hits", "paths", "pull", "panel", "detect", "hmm", "levels", "background", "events", "pairs",
                    "pairpaths", "band"):
            if fam in randcases.TWIN_OF:
                case = randcases.DRAW[randcases.TWIN_OF[fam]](rng)
                case = randcases.twin_case(fam, case, use_seed=int(rng.integers(1 << 30)))
            else:
                case = randcases.DRAW[fam](rng)
            for key in randcases.SWITCHES:
                if key in case["env"]:
                    os.environ[key] = case["env"][key]
                else:
                    os.environ.pop(key, None)
            exp = randcases.EXPECT[fam](ora, case)
            got = randcases.CALL[fam](api, case, exp)
            msg = randcases.DIFF[fam](case, got, exp)
            if msg is None and fam == "paths" and api.last_path_mismatches() != 0:
                msg = "%d hits failed the path kernel's self-check" % api.last_path_mismatches()
            if msg is None and fam == "panel":
                guard = api.last_dtw_guard()                 # the screening scheme's guard, as test_gpu_panel.same reads it
                if any(guard[k] for k in ("premise_violations", "audit_mismatches", "alarm", "exact_fallback")):
                    msg = "the guard counters are not all zero: %s" % guard
            if msg is None and fam in ("pairs", "pairpaths") and any(api.last_dtw_guard().values()):
                msg = "the guard counters are not all zero after a pair call: %s" % api.last_dtw_guard()
            if msg is None and fam == "band":                # the other of the two calls: its own diff, the same record bytes
                other = dict(case, paths=not case["paths"])
                again = randcases.CALL[fam](api, other, exp)
                msg = randcases.DIFF[fam](other, again, exp)
                if msg is None and again[0].tobytes() != got[0].tobytes():
                    msg = "the call with paths and the records-only call give other records"
                if msg is not None:
                    msg = "paths=%s instead: %s" % (other["paths"], msg)
            if msg is not None and fam == "detect":          # (the lines of the sections these draws replaced, as they were)
                bad += 1
                print("DETECT mismatch round %d: %d reads, max length %d, stride %d, params %s -- %s" %
                      (rounds, case["R"], case["dmax"], case["stride"], case["params"], msg))
            elif msg is not None and fam == "hmm":
                bad += 1
                what = "float64 feed" if case["feed"] == "f64" else "list" if case["feed"] == "list" else \
                    "int16 feed, %s" % ("calibrated" if case["calibrated"] else "raw")
                print("%s mismatch round %d: %d reads, max length %d, stride %d, %d states%s, limit %d, %s -- %s" %
                      ("HMM" if randcases.diff_hmm_records(case, got, exp) else "HMM PATH", rounds, case["R"], case["dmax"],
                       case.get("stride", 0), case["S"], " (integer scores)" if case["integer"] else "", case["limit"], what,
                       msg))
            elif msg is not None:
                bad += 1
                print("%s mismatch round %d %s: %s" % (fam.upper(), rounds, randcases.describe(case), msg))
            for key in randcases.SWITCHES:
                os.environ.pop(key, None)
        # ---- a MotifSeq session against the prefix statement (tests/stream_ref.py) ----
        msg = session_round(rng)
        if msg is not None:
            bad += 1
            print("SESSION mismatch round %d %s" % (rounds, msg))
        # ---- a mapping session against the oracle on the concatenation (tests/mapstream_ref.py) ----
        msg = mapstream_round(rng)
        if msg is not None:
            bad += 1
            print("MAPSTREAM mismatch round %d %s" % (rounds, msg))
        # ---- an event session against its statement on detect_ref (tests/evstream_ref.py) ----
        msg = evstream_round(rng)
        if msg is not None:
            bad += 1
            print("EVSTREAM mismatch round %d %s" % (rounds, msg))
        # ---- hit lists over a pair list and from a session's stored rows (tests/pair_hits_ref.py) ----
        msg = pairhits_round(rng)
        if msg is not None:
            bad += 1
            print("PAIRHITS mismatch round %d %s" % (rounds, msg))
        # ---- the signal HMM's posteriors against their statement (tests/hmm_post_ref.py) ----
        msg = hmm_post_round(rng)
        if msg is not None:
            bad += 1
            print("HMM POSTERIOR mismatch round %d %s" % (rounds, msg))
        # ---- one filtered HMM session against its statement (tests/hmmfilter_ref.py) ----
        msg = hmmfilter_round(rng)
        if msg is not None:
            bad += 1
            print("HMM FILTER mismatch round %d %s" % (rounds, msg))
    print("fuzz: %d rounds, %d mismatching configurations" % (rounds, bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
