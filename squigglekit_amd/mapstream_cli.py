"""squiggle_map_stream: replay a file as if every read's events arrived live, and map them as they arrive, on the GPU.

    squiggle_map_stream.py -s signals.tsv | --blow5 FILE | --i16 FILE.npy  -m reference.model [--both] [--prefix N] [--rna]
                           [--piece N --overlap N] [--chunk E] [--calib C] [--channels S]
                           [--min_events N] [--max_dist_per_event X] [--min_margin X] [--give_up N]
                           [--live [--sample_chunk N] [--fused]] [--locus_margin [--hits K]]

Inputs and targets are squiggle_map's.  Without --live, events are cut ONCE per read, by api.detect_events on its first
--prefix samples, and the replay is in event space: a read is dealt to a free channel (a slot of one api.MapStream over
all targets) and its event levels are pushed --chunk at a time; after every push api.map_decide looks at the read's
records.

--live: the replay is in SAMPLE space.  Each read's first --prefix samples are pushed --sample_chunk (default 2 000) at
a time through a slot of an api.EventStream, END with the last chunk; the events every push closes are normalised and
pushed to the api.MapStream slot of the same number, and api.map_decide runs after every such push.  --live needs
--calib >= 2 (all events of the prefix are not knowable live): levels are held back until the read has --calib of them
(or ends), then normalised with their mean and standard deviation, fixed from then on.  --chunk is not used.
--live --fused: the same replay through ONE api.LiveMap: levels, hold-back, normalisation and the hand-over to the mapping
side happen on the device, and so does the decision unless --piece or --locus_margin is given (merged records and hit
lists are decided on the host, from the returned records and LiveMap.hits).  The output is --live's, byte for byte.

--calib C: every level is normalised with the mean and the standard deviation of the read's first C event levels, fixed
from then on; the read's first push then holds at least those C events.  C = 0 (the default) takes all events of the
prefix -- squiggle_map's z-score, which only a replay can know -- so the last record of a read is squiggle_map's.
--channels S: slots of the session; reads are dealt to slots in file order as slots come free.
Decision (api.map_decide): accept when events >= --min_events, dist / events <= --max_dist_per_event and (second-best
dist - best dist) / events >= --min_margin; reject when not accepted and events >= --give_up; otherwise the read goes on,
and a read whose events run out prints `end`.
--locus_margin: the margin is taken to the next LOCUS, not to the next target: after every push the slots' hit lists
(MapStream.hits, up to --hits loci per target, default 2; with --piece merged by api.merge_tile_hits) go to
api.map_decide_loci, whose second dist is the best of all other listed loci -- the second copy of a repeat on the best
target included.  A read with one locus in all has an infinite margin.  The columns are the same.

Output: the header line, then one line per read at the moment of its decision (so not in file order):
    readID target strand start end events dist dist_per_event second_target second_dist decision pushes events_seen
the first ten columns as squiggle_map writes them for the events seen so far, decision one of accept / reject / end.
A read with fewer than 2 events or with levels without deviation (over its calibration events) gets `.` fields, decision
`.` and a note on stderr, as in squiggle_map; a read with more than 1 024 events is mapped like any other."""
import sys
from collections import deque

import numpy as np

from . import _lib, api
from .detect_cli import iter_tsv_reads
from .map_cli import HEADER as MAP_HEADER
from .map_cli import _Parser, load_targets, map_lines

HEADER = MAP_HEADER + ("decision", "pushes", "events_seen")
DECISIONS = {1: "accept", -1: "reject"}


def build_parser():
    p = _Parser(description="squiggle_map_stream (MI355X) - map each read's event levels to reference squiggles as they arrive")
    src = p.add_mutually_exclusive_group()
    src.add_argument("-s", "--signal", help="signal TSV of raw integer samples written by SquigglePull -r (.gz accepted)")
    src.add_argument("--blow5", help="BLOW5 file (uncompressed or zlib records)")
    src.add_argument("--i16", help="packed reads: a .npy file holding an int16 array [reads, samples] (read name = row index)")
    p.add_argument("-m", "--model", help="reference squiggles: scrappie squiggle text, every #name record is a target")
    p.add_argument("--both", action="store_true", help="also search each record's reversal (strand -)")
    p.add_argument("--prefix", type=int, default=4000, help="raw samples of each read that are cut into events (default 4000)")
    p.add_argument("--rna", action="store_true", help="the rna event-detection preset instead of dna")
    p.add_argument("--piece", type=int, default=0, help="cut targets into pieces of this many points (0: whole targets)")
    p.add_argument("--overlap", type=int, default=0, help="points neighbouring pieces share (a match no longer than this is never cut)")
    p.add_argument("--chunk", type=int, default=50, help="events per push (default 50)")
    p.add_argument("--calib", type=int, default=0, help="events whose mean / stdev normalise the read (0: all events of the prefix)")
    p.add_argument("--channels", type=int, default=512, help="slots of the session: reads in progress at a time (default 512)")
    p.add_argument("--min_events", type=int, default=100, help="accept: at least this many events (default 100)")
    p.add_argument("--max_dist_per_event", type=float, default=0.5, help="accept: dist / events at most this (default 0.5)")
    p.add_argument("--min_margin", type=float, default=0.05, help="accept: (second dist - best dist) / events at least this (default 0.05)")
    p.add_argument("--give_up", type=int, default=400, help="reject a read not accepted after this many events (default 400)")
    p.add_argument("--device", type=int, default=None, help="GPU index (default $SK_DEVICE or 0)")
    p.add_argument("--batch", type=int, default=4096, help="reads per event-detection call")
    p.add_argument("--live", action="store_true", help="replay in sample space: cut events on the GPU as each read's samples arrive")
    p.add_argument("--sample_chunk", type=int, default=2000, help="--live: raw samples per push (default 2000)")
    p.add_argument("--fused", action="store_true", help="--live: one live mapping session -- events, normalisation, mapping and the decision without a host round trip")
    p.add_argument("--locus_margin", action="store_true", help="accept on the margin to the next locus on any target (hit lists) instead of the next target")
    p.add_argument("--hits", type=int, default=2, help="--locus_margin: loci listed per read and target, 1 .. 64 (default 2)")
    return p


def normalise(levels, calib):
    """(levels - mean) / std with the statistics of the first `calib` levels (0: all of them), or None when fewer than 2
    levels or no deviation among those"""
    v = np.asarray(levels, dtype=np.float64)
    if v.size < 2:
        return None
    head = v if calib <= 0 else v[:max(calib, 1)]
    sd = head.std()
    if head.size < 2 or not sd > 0:
        return None
    return (v - head.mean()) / sd


def iter_reads(args):
    """(read id, samples) of the input, in file order"""
    if args.signal:
        for _, rid, sig in iter_tsv_reads(args.signal):
            yield rid, sig
    elif args.blow5:
        from .blow5 import read_slow5
        for rec in read_slow5(args.blow5):
            yield rec["read_id"], rec["signal"]
    else:
        a = np.load(args.i16, mmap_mode="r")
        if a.ndim != 2 or a.dtype != np.int16:
            raise ValueError("need a 2-D int16 array, got {} {}".format(a.dtype, a.shape))
        for i in range(a.shape[0]):
            yield str(i), np.asarray(a[i])


def read_samples(args, src):
    """[(read id, int16 samples)] of the input: each read's first --prefix samples, for the live replay"""
    out = []
    for rid, sig in iter_reads(args):
        b = api.as_int16_exact(np.asarray(sig)[:args.prefix])
        if b is None:
            raise ValueError("read {} is not int16-exact: event detection takes raw samples".format(rid))
        out.append((rid, np.ascontiguousarray(np.asarray(b).reshape(-1), dtype=np.int16)))
    return out


def read_levels(args, src):
    """[(read id, event levels)] of the input, events cut on each read's prefix in batches"""
    params = api.det_params("rna" if args.rna else "dna")
    out, ids, reads = [], [], []

    def flush():
        live = [i for i, r in enumerate(reads) if len(r)]
        lev = {}
        if live:
            off, rec = api.detect_events([reads[i] for i in live], params)
            values, _ = api.event_levels(off, rec)
            for k, i in enumerate(live):
                lev[i] = np.array(values[int(off[k]):int(off[k + 1])], dtype=np.float64)
        out.extend((rid, lev.get(i, np.zeros(0))) for i, rid in enumerate(ids))
        del ids[:], reads[:]

    def add(rid, sig):
        ids.append(rid)
        reads.append(np.asarray(sig)[:args.prefix])
        if len(reads) >= max(1, args.batch):
            flush()

    for rid, sig in iter_reads(args):
        add(rid, sig)
    flush()
    return out


def decide(args, ms, slots, full, tiling):
    """the decisions int8 [m] after a push: full = the (merged) records [T, m] of the named slots with their counters"""
    rule = (args.min_events, args.max_dist_per_event, args.min_margin, args.give_up)
    if not args.locus_margin:
        return api.map_decide(full, *rule)[1]
    hits, count = ms.hits(slots, args.hits)
    if tiling is not None:
        hits, count = api.merge_tile_hits(hits, count, tiling, args.hits)
    return api.map_decide_loci(hits, count, full["rows"][0], *rule)[1]


def replay(args, targets, reads, src, write):
    """deal the reads to the channels, push their events chunk by chunk, write one line per read when it is decided"""
    ys = [t[2] for t in targets]
    tiling = None
    if args.piece > 0:
        ys, tiling = api.tile_targets(ys, args.piece, args.overlap)
    queue = deque(reads)
    S = args.channels
    slot_read = [None] * S                                          # per slot: [read id, z, events pushed]
    first = max(args.chunk, args.calib)                             # the first push holds the calibration events

    def deal(s):
        while queue:
            rid, lev = queue.popleft()
            z = normalise(lev, args.calib)
            if z is None:
                sys.stderr.write("squiggle_map_stream: {} in read {} of {}\n".format(
                    "fewer than 2 events" if len(lev) < 2 else "event levels without deviation", rid, src))
                write("{}\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\t0\t0\n".format(rid))
                continue
            slot_read[s] = [rid, z, 0]
            return True
        return False

    with api.MapStream(ys, S) as ms:
        while True:
            fresh = [s for s in range(S) if slot_read[s] is None and deal(s)]
            if fresh:
                ms.reset(fresh)
            live = [s for s in range(S) if slot_read[s] is not None]
            if not live:
                break
            chunks = []
            for s in live:
                _, z, seen = slot_read[s]
                n = first if seen == 0 else args.chunk
                chunks.append(z[seen:seen + n])
                slot_read[s][2] = min(len(z), seen + n)
            rec = ms.push(live, chunks)
            hits = api.map_hits(rec)
            if tiling is not None:
                hits = api.merge_tiles(hits, tiling)
            full = np.zeros(hits.shape, dtype=api.MAPREC_DTYPE)
            for f in api.HIT_DTYPE.names:
                full[f] = hits[f]
            full["rows"], full["pushes"] = rec["rows"][:1], rec["pushes"][:1]
            dec = decide(args, ms, live, full, tiling)
            for i, s in enumerate(live):
                rid, z, seen = slot_read[s]
                word = DECISIONS.get(int(dec[i])) or ("end" if seen >= len(z) else None)
                if word is None:
                    continue
                line = map_lines([rid], [z[:seen]], hits[:, i:i + 1], targets)[0]
                write("{}\t{}\t{}\t{}\n".format(line[:-1], word, int(rec["pushes"][0, i]), seen))
                slot_read[s] = None


class _LiveRead:
    """a read in a channel of the live replay"""

    def __init__(self, rid, samples):
        self.rid, self.samples, self.at = rid, samples, 0           # at: samples pushed
        self.levels = np.zeros(0)                                   # every event level so far
        self.mean = self.sd = None                                  # fixed once --calib levels exist (or the read ends)
        self.z = np.zeros(0)                                        # the normalised levels pushed to the mapping session
        self.ended = False


def replay_live(args, targets, reads, src, write):
    """deal the reads to the channels, push their SAMPLES chunk by chunk through an event session, normalise the events
    every push closes and push them to the mapping session; one line per read when it is decided"""
    ys = [t[2] for t in targets]
    tiling = None
    if args.piece > 0:
        ys, tiling = api.tile_targets(ys, args.piece, args.overlap)
    queue = deque(reads)
    S, N, Cal = args.channels, args.sample_chunk, args.calib
    chan = [None] * S
    params = api.det_params("rna" if args.rna else "dna")

    def undecidable(r):
        sys.stderr.write("squiggle_map_stream: {} in read {} of {}\n".format(
            "fewer than 2 events" if len(r.levels) < 2 else "event levels without deviation", r.rid, src))
        write("{}\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\t0\t0\n".format(r.rid))

    with api.EventStream(params, S) as es, api.MapStream(ys, S) as ms:
        while True:
            fresh = []
            for s in range(S):
                if chan[s] is None and queue:
                    chan[s] = _LiveRead(*queue.popleft())
                    fresh.append(s)
            if fresh:
                es.reset(fresh)
                ms.reset(fresh)
            live = [s for s in range(S) if chan[s] is not None]
            if not live:
                break
            # ---- samples in, events out
            chunks, end = [], []
            for s in live:
                r = chan[s]
                chunks.append(r.samples[r.at:r.at + N])
                r.at = min(len(r.samples), r.at + N)
                r.ended = r.at >= len(r.samples)
                end.append(r.ended)
            off, rec = es.push(live, chunks, end=end)
            values, _ = api.event_levels(off, rec)
            # ---- the new levels, normalised once the calibration levels exist
            mslots, mchunks = [], []
            for i, s in enumerate(live):
                r = chan[s]
                had = len(r.levels)
                r.levels = np.concatenate([r.levels, values[int(off[i]):int(off[i + 1])]])
                if r.sd is None:
                    if len(r.levels) < Cal and not r.ended:
                        continue                                    # held back
                    head = r.levels[:Cal]
                    sd = head.std() if head.size >= 2 else 0.0
                    if not sd > 0:
                        undecidable(r)
                        chan[s] = None
                        continue
                    r.mean, r.sd = head.mean(), sd
                    had = 0
                new = (r.levels[had:] - r.mean) / r.sd
                if new.size == 0 and not r.ended:
                    continue
                r.z = np.concatenate([r.z, new])
                mslots.append(s)
                mchunks.append(new)
            if not mslots:
                continue
            mrec = ms.push(mslots, mchunks)
            hits = api.map_hits(mrec)
            if tiling is not None:
                hits = api.merge_tiles(hits, tiling)
            full = np.zeros(hits.shape, dtype=api.MAPREC_DTYPE)
            for f in api.HIT_DTYPE.names:
                full[f] = hits[f]
            full["rows"], full["pushes"] = mrec["rows"][:1], mrec["pushes"][:1]
            dec = decide(args, ms, mslots, full, tiling)
            for i, s in enumerate(mslots):
                r = chan[s]
                word = DECISIONS.get(int(dec[i])) or ("end" if r.ended else None)
                if word is None:
                    continue
                line = map_lines([r.rid], [r.z], hits[:, i:i + 1], targets)[0]
                write("{}\t{}\t{}\t{}\n".format(line[:-1], word, int(mrec["pushes"][0, i]), len(r.z)))
                chan[s] = None
    guard = api.last_event_plan()["guard_hits"]
    if guard:
        raise ValueError("event session: {} slots stopped at a guard".format(guard))


def replay_fused(args, targets, reads, src, write):
    """replay_live through one api.LiveMap: the samples go in, the records, the slots' states and (without --piece and
    --locus_margin) the decisions come out; the same lines in the same order"""
    ys = [t[2] for t in targets]
    tiling = None
    if args.piece > 0:
        ys, tiling = api.tile_targets(ys, args.piece, args.overlap)
    queue = deque(reads)
    S, N = args.channels, args.sample_chunk
    chan = [None] * S
    params = api.det_params("rna" if args.rna else "dna")
    rule = None
    if tiling is None and not args.locus_margin:
        rule = api.live_rule(args.min_events, args.max_dist_per_event, args.min_margin, args.give_up)

    with api.LiveMap(params, args.calib, ys, S) as lm:
        while True:
            fresh = []
            for s in range(S):
                if chan[s] is None and queue:
                    chan[s] = _LiveRead(*queue.popleft())
                    chan[s].mapped = 0
                    fresh.append(s)
            if fresh:
                lm.reset(fresh)
            live = [s for s in range(S) if chan[s] is not None]
            if not live:
                break
            chunks, end = [], []
            for s in live:
                r = chan[s]
                chunks.append(r.samples[r.at:r.at + N])
                r.at = min(len(r.samples), r.at + N)
                r.ended = r.at >= len(r.samples)
                end.append(r.ended)
            res = lm.push(live, chunks, end=end, rule=rule)
            rec, info = res[0], res[1]
            # ---- the slots whose read cannot be normalised, then the ones that were handed levels (or ended)
            idx = []
            for i, s in enumerate(live):
                r = chan[s]
                state = int(info["state"][i])
                if state == _lib.SK_LIVE_UNDECIDABLE:
                    sys.stderr.write("squiggle_map_stream: {} in read {} of {}\n".format(
                        "fewer than 2 events" if int(info["events"][i]) < 2 else "event levels without deviation", r.rid, src))
                    write("{}\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\t0\t0\n".format(r.rid))
                    chan[s] = None
                    continue
                if state != _lib.SK_LIVE_MAPPING:
                    continue                                        # held back
                new, r.mapped = int(info["mapped"][i]) - r.mapped, int(info["mapped"][i])
                if new == 0 and not r.ended:
                    continue
                idx.append(i)
            if not idx:
                continue
            mslots = [live[i] for i in idx]
            mrec = rec[:, idx]
            hits = api.map_hits(mrec)
            if tiling is not None:
                hits = api.merge_tiles(hits, tiling)
            if rule is not None:
                dec = res[2]["decision"][idx]
            else:
                full = np.zeros(hits.shape, dtype=api.MAPREC_DTYPE)
                for f in api.HIT_DTYPE.names:
                    full[f] = hits[f]
                full["rows"], full["pushes"] = mrec["rows"][:1], mrec["pushes"][:1]
                dec = decide(args, lm, mslots, full, tiling)
            for i, s in enumerate(mslots):
                r = chan[s]
                word = DECISIONS.get(int(dec[i])) or ("end" if r.ended else None)
                if word is None:
                    continue
                line = map_lines([r.rid], [range(r.mapped)], hits[:, i:i + 1], targets)[0]
                write("{}\t{}\t{}\t{}\n".format(line[:-1], word, int(mrec["pushes"][0, i]), r.mapped))
                chan[s] = None
    guard = api.last_event_plan()["guard_hits"]
    if guard:
        raise ValueError("event session: {} slots stopped at a guard".format(guard))


def main(argv=None):
    parser = build_parser()
    argv = sys.argv[1:] if argv is None else argv
    args = parser.parse_args(argv)
    if len(argv) == 0:
        parser.print_help(sys.stderr)
        sys.exit(1)
    if not (args.signal or args.blow5 or args.i16):
        parser.error("one of -s/--signal, --blow5, --i16 is needed")
    if not args.model:
        parser.error("-m/--model is needed")
    if args.prefix < 1:
        parser.error("--prefix must be at least 1")
    if args.piece < 0 or args.overlap < 0 or (args.piece > 0 and args.overlap >= args.piece):
        parser.error("need 0 <= --overlap < --piece")
    if args.overlap and not args.piece:
        parser.error("--overlap needs --piece")
    if not 1 <= args.chunk <= _lib.SK_MAP_MAX_CHUNK:
        parser.error("--chunk must be in 1 .. {}".format(_lib.SK_MAP_MAX_CHUNK))
    if not 0 <= args.calib <= _lib.SK_MAP_MAX_CHUNK:
        parser.error("--calib must be in 0 .. {}".format(_lib.SK_MAP_MAX_CHUNK))
    if not 1 <= args.channels <= _lib.SK_MAP_MAX_SLOTS:
        parser.error("--channels must be in 1 .. {}".format(_lib.SK_MAP_MAX_SLOTS))
    if args.min_events < 0:
        parser.error("--min_events must not be negative")
    if args.give_up < 1:
        parser.error("--give_up must be at least 1")
    if args.max_dist_per_event != args.max_dist_per_event or args.min_margin != args.min_margin:
        parser.error("--max_dist_per_event and --min_margin must be numbers")
    if not 1 <= args.hits <= 64:
        parser.error("--hits must be in 1 .. 64")
    if args.hits != 2 and not args.locus_margin:
        parser.error("--hits needs --locus_margin")
    if args.live:
        if args.calib < 2:
            parser.error("--live needs --calib >= 2 (the statistics of all events of the prefix are not knowable live)")
        if args.sample_chunk < 1:
            parser.error("--sample_chunk must be at least 1")
        if args.calib + args.sample_chunk > _lib.SK_MAP_MAX_CHUNK:
            parser.error("--calib + --sample_chunk must be at most {}".format(_lib.SK_MAP_MAX_CHUNK))
        if args.channels > _lib.SK_EVS_MAX_SLOTS:
            parser.error("--channels must be in 1 .. {}".format(_lib.SK_EVS_MAX_SLOTS))
        if args.fused and args.calib > _lib.SK_LIVE_MAX_CALIB:
            parser.error("--fused: --calib must be at most {}".format(_lib.SK_LIVE_MAX_CALIB))
    elif args.fused:
        parser.error("--fused needs --live")
    try:
        targets = load_targets(args.model, args.both)
    except (ValueError, IndexError, OSError) as e:
        sys.stderr.write("squiggle_map_stream: {}: {}\n".format(args.model, e))
        sys.exit(2)

    _lib.warm_start(args.device, also=())
    src = args.signal or args.blow5 or args.i16
    sys.stdout.write("\t".join(HEADER) + "\n")
    try:
        if args.live:
            (replay_fused if args.fused else replay_live)(args, targets, read_samples(args, src), src, sys.stdout.write)
        else:
            replay(args, targets, read_levels(args, src), src, sys.stdout.write)
    except (ValueError, EOFError, OSError) as e:
        sys.stdout.flush()
        sys.stderr.write("squiggle_map_stream: {}: {}\n".format(src, e))
        sys.exit(2)
    sys.stdout.flush()


if __name__ == "__main__":
    main()
