"""squiggle_map_stream: replay a file as if every read's events arrived live, and map them as they arrive, on the GPU.

    squiggle_map_stream.py -s signals.tsv | --blow5 FILE | --i16 FILE.npy  -m reference.model [--both] [--prefix N] [--rna]
                           [--piece N --overlap N] [--chunk E] [--calib C] [--channels S]
                           [--min_events N] [--max_dist_per_event X] [--min_margin X] [--give_up N]
                           [--live [--sample_chunk N] [--fused] [--polya_gate ...]] [--locus_margin [--hits K]]

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
--live --polya_gate [--gate_preset P | --gate_model FILE] [--min_body N] [--gate_margin X] [--gate_give_up N]
[--gate_hold G]: direct RNA.  A read begins with open pore, leader, adapter and poly(A); none of it belongs to a target.
Every channel's samples also go through the signal HMM of dRNA_polya_stream (api.HmmStream; under a pA --gate_preset a
BLOW5 record's calibration pair goes to the slot, with --gate_model too: the preset says which units the model is in), and api.polya_decide's rule -- the path ends in TRANSCRIPT, has been there
--min_body samples, leads every other state by --gate_margin -- opens the channel's gate at the transcript start.  Only
events that START at or after it are levels of the read: the hold-back, the --calib statistics and the mapping begin
there.  While the gate is shut the channel keeps its last --gate_hold events, so the ones between the start and the
decision are not lost.  A read whose gate has not opened after --gate_give_up samples (0: never), or when it ends, prints
`gate_reject` at that moment.  Lines carry one more column, transcript_start (-1: the gate never opened).  Without --fused
the gate runs on the host from HmmStream, polya_decide, EventStream and MapStream; with --fused one gated api.LiveMap
does it on the device; the two print the same lines byte for byte.

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
    p.add_argument("--polya_gate", action="store_true", help="--live: map from the transcript start a signal HMM finds (direct RNA): events before it are dropped")
    p.add_argument("--gate_preset", default="rna_pa", choices=sorted(api.POLYA_PRESETS), help="--polya_gate: the HMM's preset (default rna_pa)")
    p.add_argument("--gate_model", metavar="FILE", help="--polya_gate: model description (JSON, api.hmm_spec_to_json) in place of the preset's numbers")
    p.add_argument("--min_body", type=int, default=2000, help="--polya_gate: open when the path has been in TRANSCRIPT for this many samples (default 2000)")
    p.add_argument("--gate_margin", type=float, default=20.0, help="--polya_gate: ... and TRANSCRIPT leads every other state by this (default 20)")
    p.add_argument("--gate_give_up", type=int, default=0, help="--polya_gate: reject a read whose gate has not opened after this many samples (0: never)")
    p.add_argument("--gate_hold", type=int, default=1024, help="--polya_gate: events a channel keeps while its gate is shut, 1 .. 4096 (default 1024)")
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
    return [(rid, _prefix_i16(args, rid, sig)) for rid, sig in iter_reads(args)]


def _prefix_i16(args, rid, sig):
    """a read's first --prefix samples as int16"""
    b = api.as_int16_exact(np.asarray(sig)[:args.prefix])
    if b is None:
        raise ValueError("read {} is not int16-exact: event detection takes raw samples".format(rid))
    return np.ascontiguousarray(np.asarray(b).reshape(-1), dtype=np.int16)


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


def read_samples_cal(args, src):
    """[(read id, int16 samples, (offset, unit))] for --polya_gate: read_samples with the calibration pair the gate's
    model sees the samples through.  The pairs come from the file as dRNA_polya_stream takes them (polya_cli.iter_input):
    the BLOW5 record's under a pA --gate_preset, with or without --gate_model, and (0, 1) otherwise.  Each pair travels
    with its own record: nothing is looked up by read id."""
    from .polya_cli import PA_PRESETS, iter_input
    if args.blow5:
        reads = iter_input(args, args.gate_preset in PA_PRESETS, args.batch)
    else:
        reads = ((rid, sig, None) for rid, sig in iter_reads(args))
    out = []
    for rid, sig, cal in reads:
        out.append((rid, _prefix_i16(args, rid, sig), (0.0, 1.0) if cal is None else cal))
    return out


class _GatedRead(_LiveRead):
    """a read in a channel of the gated live replay"""

    def __init__(self, rid, samples, cal):
        _LiveRead.__init__(self, rid, samples)
        self.cal = cal
        self.mapped = 0                                             # normalised levels handed to the mapping side
        self.t0 = -1
        self.gate, self.ring = _lib.SK_LIVE_GATE_GATING, None       # the gate's state; the host gate's ring of held events


class _HostGate:
    """What a gated api.LiveMap does, from existing parts on the host: HmmStream -> polya_decide -> EventStream -> the
    filter start >= t0 behind a ring of --gate_hold events -> hold-back and normalisation -> MapStream.  push() returns
    the slots' states as the LiveMap's info and gate() would; records() pushes the levels of the named entries on."""

    def __init__(self, args, params, ys, S, model):
        self.args = args
        self.hs, self.es, self.ms = api.HmmStream(model, S), api.EventStream(params, S), api.MapStream(ys, S)
        self.hits = self.ms.hits

    def close(self):
        for x in (self.hs, self.es, self.ms):
            x.close()

    def reset(self, slots, reads):
        self.hs.reset(slots, np.array([r.cal for r in reads], dtype=np.float64))
        self.es.reset(slots)
        self.ms.reset(slots)
        for r in reads:
            r.ring = deque(maxlen=self.args.gate_hold)

    def push(self, live, reads, chunks, end):
        a = self.args
        gating = [i for i, r in enumerate(reads) if r.gate == _lib.SK_LIVE_GATE_GATING]
        hrec = self.hs.push([live[i] for i in gating], [chunks[i] for i in gating])
        dec = api.polya_decide(hrec, a.min_body, a.gate_margin, a.gate_give_up)
        off, rec = self.es.push(live, chunks, end=end)
        was = [r.gate for r in reads]
        for k, i in enumerate(gating):
            r = reads[i]
            if dec[k] == 1:
                r.gate, r.t0 = _lib.SK_LIVE_GATE_OPEN, int(hrec["enter"][k][api.TRANSCRIPT])
            elif dec[k] == -1 or end[i]:
                r.gate = _lib.SK_LIVE_GATE_REJECTED
        info = np.zeros(len(live), dtype=api.LIVEINFO_DTYPE)
        gate = np.zeros(len(live), dtype=api.GATE_DTYPE)
        self.handed = []
        for i, r in enumerate(reads):
            new = rec[int(off[i]):int(off[i + 1])]
            released = new[:0]
            if r.gate == _lib.SK_LIVE_GATE_OPEN:
                cand = (list(r.ring) if was[i] == _lib.SK_LIVE_GATE_GATING else []) + list(new)
                keep = [e for e in cand if int(e["start"]) >= r.t0]
                released = np.array(keep, dtype=rec.dtype) if keep else new[:0]
                r.ring.clear()
            elif r.gate == _lib.SK_LIVE_GATE_GATING:
                r.ring.extend(new)
            # ---- the live side on the released events: replay_live's hold-back and normalisation
            lev = released["sum"].astype(np.float64) / released["length"].astype(np.float64)
            had = len(r.levels)
            r.levels = np.concatenate([r.levels, lev])
            state, chunk = _lib.SK_LIVE_CALIBRATING, np.zeros(0)
            if r.sd is None and r.mean is None:
                if not (len(r.levels) < a.calib and not r.ended):
                    head = r.levels[:a.calib]
                    sd = head.std() if head.size >= 2 else 0.0
                    if not sd > 0:
                        r.mean = np.nan                             # undecidable from here on
                    else:
                        r.mean, r.sd = head.mean(), sd
                        had = 0
            if r.sd is not None:
                state, chunk = _lib.SK_LIVE_MAPPING, (r.levels[had:] - r.mean) / r.sd
            elif r.mean is not None:
                state = _lib.SK_LIVE_UNDECIDABLE
            self.handed.append(chunk)
            info[i] = (np.nan, np.nan, len(r.levels), r.mapped + len(chunk), 0, state, int(r.ended), len(lev))
            gate[i]["state"], gate[i]["t0"] = r.gate, r.t0
        return info, gate

    def records(self, live, idx):
        return self.ms.push([live[i] for i in idx], [self.handed[i] for i in idx])


class _FusedGate:
    """the same through one gated api.LiveMap"""

    def __init__(self, args, params, ys, S, model, rule):
        gate = api.live_gate(model, args.min_body, args.gate_margin, args.gate_give_up, args.gate_hold)
        self.lm, self.rule = api.LiveMap(params, args.calib, ys, S, gate=gate), rule
        self.hits = self.lm.hits

    def close(self):
        self.lm.close()

    def reset(self, slots, reads):
        self.lm.reset(slots, np.array([r.cal for r in reads], dtype=np.float64))

    def push(self, live, reads, chunks, end):
        self.res = self.lm.push(live, chunks, end=end, rule=self.rule)
        gate, _ = self.lm.gate()
        for r, g in zip(reads, gate):
            r.gate, r.t0 = int(g["state"]), int(g["t0"])
        return self.res[1], gate

    def records(self, live, idx):
        return self.res[0][:, idx]


def replay_gated(args, targets, reads, src, write):
    """--live --polya_gate: replay_live / replay_fused behind a poly(A) gate -- every read's samples also go through the
    signal HMM, and only the events from the transcript start it finds on reach the calibration head and the mapping
    session.  One line per read when it is decided, rejected by the gate or found undecidable; the unfused and the fused
    route print the same lines in the same order."""
    ys = [t[2] for t in targets]
    tiling = None
    if args.piece > 0:
        ys, tiling = api.tile_targets(ys, args.piece, args.overlap)
    queue = deque(reads)
    S, N = args.channels, args.sample_chunk
    chan = [None] * S
    params = api.det_params("rna" if args.rna else "dna")
    if args.gate_model:
        with open(args.gate_model) as fh:
            model = api.hmm_model(*api.hmm_spec_from_json(fh.read()))
    else:
        model = api.polya_model(args.gate_preset)
    if model.nstates != 6:
        raise ValueError("the gate reads the six states of api.POLYA_STATES; the model has {}".format(model.nstates))
    rule = None
    if args.fused and tiling is None and not args.locus_margin:
        rule = api.live_rule(args.min_events, args.max_dist_per_event, args.min_margin, args.give_up)
    eng = _FusedGate(args, params, ys, S, model, rule) if args.fused else _HostGate(args, params, ys, S, model)
    dots = "\t.\t.\t.\t.\t.\t.\t.\t.\t.\t"
    try:
        while True:
            fresh = []
            for s in range(S):
                if chan[s] is None and queue:
                    chan[s] = _GatedRead(*queue.popleft())
                    fresh.append(s)
            if fresh:
                eng.reset(fresh, [chan[s] for s in fresh])
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
            info, gate = eng.push(live, [chan[s] for s in live], chunks, end)
            # ---- the reads the gate has rejected, the ones that cannot be normalised, then the ones handed levels (or ended)
            idx = []
            for i, s in enumerate(live):
                r = chan[s]
                state = int(info["state"][i])
                if int(gate["state"][i]) == _lib.SK_LIVE_GATE_REJECTED:
                    write("{}{}gate_reject\t0\t0\t-1\n".format(r.rid, dots))
                    chan[s] = None
                    continue
                if state == _lib.SK_LIVE_UNDECIDABLE:
                    sys.stderr.write("squiggle_map_stream: {} in read {} of {}\n".format(
                        "fewer than 2 events" if int(info["events"][i]) < 2 else "event levels without deviation", r.rid, src))
                    write("{}{}.\t0\t0\t{}\n".format(r.rid, dots, r.t0))
                    chan[s] = None
                    continue
                if state != _lib.SK_LIVE_MAPPING:
                    continue                                        # gating, or held back
                new, r.mapped = int(info["mapped"][i]) - r.mapped, int(info["mapped"][i])
                if new == 0 and not r.ended:
                    continue
                idx.append(i)
            if not idx:
                continue
            mslots = [live[i] for i in idx]
            mrec = eng.records(live, idx)
            hits = api.map_hits(mrec)
            if tiling is not None:
                hits = api.merge_tiles(hits, tiling)
            if rule is not None:
                dec = eng.res[2]["decision"][idx]
            else:
                full = np.zeros(hits.shape, dtype=api.MAPREC_DTYPE)
                for f in api.HIT_DTYPE.names:
                    full[f] = hits[f]
                full["rows"], full["pushes"] = mrec["rows"][:1], mrec["pushes"][:1]
                dec = decide(args, eng, mslots, full, tiling)
            for i, s in enumerate(mslots):
                r = chan[s]
                word = DECISIONS.get(int(dec[i])) or ("end" if r.ended else None)
                if word is None:
                    continue
                line = map_lines([r.rid], [range(r.mapped)], hits[:, i:i + 1], targets)[0]
                write("{}\t{}\t{}\t{}\t{}\n".format(line[:-1], word, int(mrec["pushes"][0, i]), r.mapped, r.t0))
                chan[s] = None
    finally:
        eng.close()
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
        if args.polya_gate:
            if args.min_body < 1:
                parser.error("--min_body must be at least 1")
            if not 1 <= args.gate_hold <= _lib.SK_LIVE_MAX_GATE_HOLD:
                parser.error("--gate_hold must be in 1 .. {}".format(_lib.SK_LIVE_MAX_GATE_HOLD))
            if args.gate_margin != args.gate_margin:
                parser.error("--gate_margin must be a number")
            if args.calib + args.gate_hold + args.sample_chunk > _lib.SK_MAP_MAX_CHUNK:
                parser.error("--calib + --gate_hold + --sample_chunk must be at most {}".format(_lib.SK_MAP_MAX_CHUNK))
    elif args.fused:
        parser.error("--fused needs --live")
    if args.polya_gate and not args.live:
        parser.error("--polya_gate needs --live")
    try:
        targets = load_targets(args.model, args.both)
    except (ValueError, IndexError, OSError) as e:
        sys.stderr.write("squiggle_map_stream: {}: {}\n".format(args.model, e))
        sys.exit(2)

    _lib.warm_start(args.device, also=())
    src = args.signal or args.blow5 or args.i16
    sys.stdout.write("\t".join(HEADER + (("transcript_start",) if args.polya_gate else ())) + "\n")
    try:
        if args.polya_gate:
            replay_gated(args, targets, read_samples_cal(args, src), src, sys.stdout.write)
        elif args.live:
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
