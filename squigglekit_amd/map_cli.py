"""squiggle_map: search the event levels of each read's first samples in reference squiggles, on the GPU.

    squiggle_map.py -s signals.tsv | --blow5 FILE | --i16 FILE.npy  -m reference.model [--both] [--prefix N] [--rna]
                    [--piece N --overlap N] [--align FILE] [--whole FILE [--band 64|128|256]]
                    [--hits K --secondary FILE [--max_dist_per_event X]]
                    [--pileup FILE [--pileup_of align|whole]]

Per read: event detection on the first --prefix raw samples (api.detect_events), the level of every event
(api.event_levels), (level - mean) / std in numpy, then subsequence DTW of those levels against every target in one call
(api.map_queries).  The targets are the records of a scrappie squiggle text (-m): each `#name` record's per-base currents
(tsvio.read_scrappie_levels), z-scored the same way; --both adds each record's reversal as a second target (strand -).
--piece / --overlap cut long targets into overlapping pieces (api.tile_targets / api.merge_tiles).

Output: the header line, then one line per read (tab separated, floats as Python's "{}" writes them):
    readID target strand start end events dist dist_per_event second_target second_dist
start / end: the first and last target point of the match, in the coordinates of the target searched (for strand - those
of the reversed record).  second_target: the best of the other targets as name + strand, `.` when there is one target
only.  A read with fewer than 2 events, with levels of zero deviation or with more than 1 024 events gets `.` fields and
a note on stderr.

--align FILE: the event alignment table.  For every read that printed a match, one line per event of the read against
its best target, under a header line:
    readID target strand event sample_start sample_length level z ref_first ref_last
event: the 0-based index; sample_start / sample_length: the event record's start and length; level: its level; z: its
z-scored value (the query point); ref_first / ref_last: the target points the event covers on the warping path of the
match (api.map_paths), in the coordinates of the target searched, as start / end above.  With --piece the merged record
is traced against the whole target.  stdout is the same with and without --align.

--whole FILE: the alignment of the WHOLE read, once the prefix has found its locus.  For every read that printed a match:
event detection on all its samples, the levels z-scored as above, then adaptive-band DTW (api.align_reads, --band cells
per anti-diagonal, default 128; start pinned, end free) against target[start : start + span] of the matched target and
strand, span = min(len - start, ceil(N_all * (end - start + 1) / n_prefix * 1.5) + band) with N_all / n_prefix the events of
the whole read / of its prefix.  FILE gets the --align header and one line per event, ref_first / ref_last in the
coordinates of the target searched.  A read whose band lost the end, or with fewer than 2 events or levels without
deviation, writes no lines and a note on stderr.  stdout and --align are the same with and without --whole.

--hits K --secondary FILE: every locus, not only the best.  Up to K non-overlapping loci per read and target
(api.map_queries_hits; with --piece the pieces' lists go through api.merge_tile_hits), --max_dist_per_event X keeps those
with dist / events <= X.  FILE gets a header line and one line per listed locus of every read that has some, a read's loci
in the order of (dist, target, end):
    readID rank target strand start end dist dist_per_event margin
rank: 1 for the read's best locus; margin: dist minus the dist of the read's best locus.  stdout is the same with and
without these flags.

--pileup FILE [--pileup_of align|whole]: the alignment table turned round.  The rows one of the two tables has -- those of
--align (the default; the paths are traced whether or not --align is given) or those of --whole (which then must be given)
-- are kept over the whole run, 20 bytes per event (z, sample_length and the two ends of its span) and 8 per read, and go
through api.pileup in one call at the end.  FILE gets a header line and one line per point of every target, in the order of
the targets:
    target strand pos ref_z depth events shared level level_sd min max dwell_mean dwell_sd
pos: the point, in the coordinates of the target searched; ref_z: the target's z-scored level there; depth: the reads that
cover the point; events: the table rows that do (events - depth of them stayed on the point); shared: the rows among them
that also cover a neighbour (a skip); level / level_sd / min / max: mean, standard deviation (ddof 0), minimum and maximum
of the rows' z in table order, as numpy computes them; dwell_mean / dwell_sd: the same of their sample_length.  A point
nobody covers has `.` in the six statistics.  stdout, --align, --whole and --secondary are the same with and without
--pileup; a FILE that cannot be written fails before the run."""
import argparse
import math
import sys

import numpy as np

from . import api
from .detect_cli import iter_tsv_reads

HEADER = ("readID", "target", "strand", "start", "end", "events", "dist", "dist_per_event", "second_target", "second_dist")
SECONDARY_HEADER = ("readID", "rank", "target", "strand", "start", "end", "dist", "dist_per_event", "margin")
ALIGN_HEADER = ("readID", "target", "strand", "event", "sample_start", "sample_length", "level", "z", "ref_first", "ref_last")
PILEUP_HEADER = ("target", "strand", "pos", "ref_z", "depth", "events", "shared", "level", "level_sd", "min", "max",
                 "dwell_mean", "dwell_sd")
MAX_EVENTS = 1024


class _Parser(argparse.ArgumentParser):
    def error(self, message):
        sys.stderr.write("error: %s\n" % message)
        self.print_help()
        sys.exit(2)


def build_parser():
    p = _Parser(description="squiggle_map (MI355X) - map the event levels of each read's prefix to reference squiggles by DTW")
    src = p.add_mutually_exclusive_group()
    src.add_argument("-s", "--signal", help="signal TSV of raw integer samples written by SquigglePull -r (.gz accepted)")
    src.add_argument("--blow5", help="BLOW5 file (uncompressed or zlib records)")
    src.add_argument("--i16", help="packed reads: a .npy file holding an int16 array [reads, samples] (read name = row index)")
    p.add_argument("-m", "--model", help="reference squiggles: scrappie squiggle text, every #name record is a target")
    p.add_argument("--both", action="store_true", help="also search each record's reversal (strand -)")
    p.add_argument("--prefix", type=int, default=4000, help="raw samples of each read that are searched (default 4000)")
    p.add_argument("--rna", action="store_true", help="the rna event-detection preset instead of dna")
    p.add_argument("--piece", type=int, default=0, help="cut targets into pieces of this many points (0: whole targets)")
    p.add_argument("--overlap", type=int, default=0, help="points neighbouring pieces share (a match no longer than this is never cut)")
    p.add_argument("--align", help="write the event alignment table to this file: one line per event of every matched read")
    p.add_argument("--whole", help="write the alignment table of the WHOLE read against the matched locus to this file (adaptive-band DTW)")
    p.add_argument("--band", type=int, default=128, help="cells per anti-diagonal of the --whole alignment: 64, 128 or 256 (default 128)")
    p.add_argument("--hits", type=int, default=0, help="list up to this many non-overlapping loci per read and target (1..64; needs --secondary)")
    p.add_argument("--secondary", help="write every listed locus of every read to this file (needs --hits)")
    p.add_argument("--max_dist_per_event", type=float, default=None, help="list only loci with dist / events at most this (needs --hits)")
    p.add_argument("--pileup", help="write per-point statistics of the aligned events (one line per point of every target) to this file; "
                                    "keeps 20 bytes per aligned event until the end of the run")
    p.add_argument("--pileup_of", choices=("align", "whole"), default="align",
                   help="the table --pileup turns round: the prefix alignment of --align (default; traced also without --align) "
                        "or the whole-read alignment of --whole")
    p.add_argument("--device", type=int, default=None, help="GPU index (default $SK_DEVICE or 0)")
    p.add_argument("--batch", type=int, default=4096, help="reads per GPU call")
    return p


def zscore(v):
    """(v - mean) / std in numpy (ddof 0), or None when fewer than 2 values or no deviation"""
    v = np.asarray(v, dtype=np.float64)
    if v.size < 2:
        return None
    sd = v.std()
    if not sd > 0:
        return None
    return (v - v.mean()) / sd


def load_targets(path, both):
    """[(name, strand, z-scored levels)] of a scrappie squiggle text; ValueError for a record that cannot be z-scored"""
    from .tsvio import read_scrappie_levels
    levels, order, _ = read_scrappie_levels(path)
    if not order:
        raise ValueError("no #name record")
    out = []
    for name in order:
        z = zscore(levels[name])
        if z is None:
            raise ValueError("record {}: fewer than 2 levels, or levels without deviation".format(name))
        out.append((name, "+", z))
        if both:
            out.append((name, "-", np.ascontiguousarray(z[::-1])))
    return out


def map_lines(read_ids, queries, records, targets):
    """the output lines of a batch: queries[r] the z-scored levels or None, records [T, Q] over the reads that have some
    (in order), targets as load_targets returns them"""
    out, q = [], 0
    for rid, z in zip(read_ids, queries):
        if z is None:
            out.append("{}\t.\t.\t.\t.\t.\t.\t.\t.\t.\n".format(rid))
            continue
        col = records[:, q]
        q += 1
        d = np.where(np.isnan(col["dist"]), np.inf, col["dist"])
        b = int(np.argmin(d))
        rest = d.copy()
        rest[b] = np.inf
        s = int(np.argmin(rest)) if len(d) > 1 else -1
        h = col[b]
        out.append("{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\n".format(
            rid, targets[b][0], targets[b][1], int(h["start"]), int(h["end"]), len(z), float(h["dist"]),
            float(h["dist"]) / len(z), "." if s < 0 else targets[s][0] + targets[s][1],
            "." if s < 0 else float(col[s]["dist"])))
    return out


def secondary_lines(read_ids, queries, hits, count, targets, max_dist_per_event=None):
    """the --secondary lines of a batch: hits [T, Q, K] / count [T, Q] over the reads that have a query (in order)"""
    out, q = [], 0
    for rid, z in zip(read_ids, queries):
        if z is None:
            continue
        loci = [(float(hits[t, q, k]["dist"]), t, int(hits[t, q, k]["end"]), int(hits[t, q, k]["start"]))
                for t in range(count.shape[0]) for k in range(int(count[t, q]))]
        q += 1
        if max_dist_per_event is not None:
            loci = [c for c in loci if c[0] / len(z) <= max_dist_per_event]
        loci.sort()
        for rank, (d, t, e, a) in enumerate(loci):
            out.append("{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\n".format(
                rid, rank + 1, targets[t][0], targets[t][1], a, e, d, d / len(z), d - loci[0][0]))
    return out


def align_lines(rid, target, events, levels, z, spans):
    """the table lines of one read: events its DET_EVENT_DTYPE records, levels / z the level and query point per event,
    spans [events, 2] of its path in target = (name, strand, ...); none for a read without a path (spans -1)"""
    spans = np.asarray(spans).reshape(-1, 2)
    if spans.size == 0 or spans[0, 0] < 0:
        return []
    return ["{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\n".format(
        rid, target[0], target[1], e, int(events["start"][e]), int(events["length"][e]), float(levels[e]), float(z[e]),
        int(spans[e, 0]), int(spans[e, 1])) for e in range(len(z))]


def whole_span(length, start, end, n_prefix, n_all, band):
    """target points the whole read is aligned against, from `start` on: the prefix's points per event, scaled to the
    whole read's events, half as much again, plus the band; cut at the target's end"""
    return min(length - start, int(math.ceil(n_all * (end - start + 1) / n_prefix * 1.5)) + band)


class _Pile:
    """the rows --pileup keeps over the run: per matched read its z, sample lengths and spans, its target and shift"""

    def __init__(self):
        self.z, self.length, self.spans, self.target, self.shift = [], [], [], [], []

    def add(self, z, events, spans, target, shift):
        self.z.append(np.asarray(z, dtype=np.float64))
        self.length.append(np.asarray(events["length"], dtype=np.int32))
        self.spans.append(np.asarray(spans, dtype=np.int32).reshape(-1, 2))
        self.target.append(int(target))
        self.shift.append(int(shift))

    def table(self, targets):
        """the text of FILE: one api.pileup call over everything kept"""
        span_off = np.concatenate([[0], np.cumsum([len(z) for z in self.z])]).astype(np.int64)
        cat = lambda parts, empty: np.concatenate(parts) if parts else empty                     # noqa: E731
        pile = api.pileup(span_off, cat(self.spans, np.zeros((0, 2), dtype=np.int32)), cat(self.z, np.zeros(0)),
                          dwell=cat(self.length, np.zeros(0, dtype=np.int32)), target=np.array(self.target, dtype=np.int32),
                          shift=np.array(self.shift, dtype=np.int32), tlen=[len(t[2]) for t in targets])
        return pileup_text(targets, pile)


def pileup_text(targets, pile):
    """the --pileup table: targets as load_targets returns them, pile the PILE_DTYPE records of all their points"""
    out = ["\t".join(PILEUP_HEADER) + "\n"]
    for (name, strand, y), part in zip(targets, api.pile_split(pile, [len(t[2]) for t in targets])):
        for j in range(len(y)):
            r = part[j]
            stats = ["."] * 6 if r["n"] == 0 else ["{}".format(float(r[k])) for k in
                                                   ("level", "level_sd", "vmin", "vmax", "dwell_mean", "dwell_sd")]
            out.append("\t".join([name, strand, str(j), "{}".format(float(y[j])), str(int(r["depth"])), str(int(r["n"])),
                                  str(int(r["shared"]))] + stats) + "\n")
    return "".join(out)


class _Batcher:
    def __init__(self, args, targets, tool_input, align=None, whole=None, secondary=None, pile=None):
        self.args, self.targets, self.input, self.align, self.whole = args, targets, tool_input, align, whole
        self.secondary = secondary
        self.pile = pile                                            # the rows --pileup keeps (a _Pile), or None
        self.pile_align = pile is not None and args.pileup_of == "align"
        self.params = api.det_params("rna" if args.rna else "dna")
        self.ids, self.reads, self.full = [], [], []

    def add(self, rid, sig):
        self.ids.append(rid)
        self.reads.append(np.asarray(sig)[:self.args.prefix])
        if self.whole is not None:
            self.full.append(np.asarray(sig))
        if len(self.reads) >= max(1, self.args.batch):
            self.flush()

    def flush(self):
        if not self.reads:
            return
        live = [i for i, r in enumerate(self.reads) if len(r)]
        lev, evs = {}, {}
        if live:
            off, rec = api.detect_events([self.reads[i] for i in live], self.params)
            values, _ = api.event_levels(off, rec)
            for k, i in enumerate(live):
                lev[i] = values[int(off[k]):int(off[k + 1])]
                evs[i] = rec[int(off[k]):int(off[k + 1])]
        queries = []
        for i, rid in enumerate(self.ids):
            v = lev.get(i, np.zeros(0))
            z = zscore(v) if v.size <= MAX_EVENTS else None
            if z is None:
                why = ("more than {} events".format(MAX_EVENTS) if v.size > MAX_EVENTS else
                       "fewer than 2 events" if v.size < 2 else "event levels without deviation")
                sys.stderr.write("squiggle_map: {} in read {} of {}\n".format(why, rid, self.input))
            queries.append(z)
        qs = [z for z in queries if z is not None]
        ys = [t[2] for t in self.targets]
        records = np.zeros((len(ys), 0), dtype=api.HIT_DTYPE)
        if qs:
            if self.args.piece > 0:
                pieces, tiling = api.tile_targets(ys, self.args.piece, self.args.overlap)
                records = api.merge_tiles(api.map_queries(qs, pieces)[0], tiling)
            else:
                records = api.map_queries(qs, ys)[0]
        sys.stdout.write("".join(map_lines(self.ids, queries, records, self.targets)))
        if self.secondary is not None and qs:
            if self.args.piece > 0:
                hits, count = api.map_queries_hits(qs, pieces, self.args.hits)
                hits, count = api.merge_tile_hits(hits, count, tiling, self.args.hits)
            else:
                hits, count = api.map_queries_hits(qs, ys, self.args.hits)
            self.secondary.write("".join(secondary_lines(self.ids, queries, hits, count, self.targets,
                                                         self.args.max_dist_per_event)))
        if (self.align is not None or self.pile_align) and qs:
            best = api.best_targets(records)
            span_off, spans = api.map_paths(qs, ys, records, best)
            rows = [i for i, z in enumerate(queries) if z is not None]
            for q, i in enumerate(rows):
                if best[q] >= 0:
                    sp = spans[int(span_off[q]):int(span_off[q + 1])]
                    if self.align is not None:
                        self.align.write("".join(align_lines(self.ids[i], self.targets[int(best[q])], evs[i], lev[i],
                                                             queries[i], sp)))
                    if self.pile_align and len(sp) and sp[0, 0] >= 0:
                        self.pile.add(queries[i], evs[i], sp, best[q], 0)
        if self.whole is not None and qs:
            self.write_whole(queries, records)
        self.ids, self.reads, self.full = [], [], []

    def write_whole(self, queries, records):
        """the --whole table of the batch: queries / records as flush made them"""
        best = api.best_targets(records)
        rows = [i for i, z in enumerate(queries) if z is not None]
        todo = [(q, i) for q, i in enumerate(rows) if best[q] >= 0]
        if not todo:
            return
        off, rec = api.detect_events([self.full[i] for _, i in todo], self.params)
        values, _ = api.event_levels(off, rec)
        jobs = []                                                   # (read, target, record, events, levels, z, window)
        for k, (q, i) in enumerate(todo):
            lev, ev = values[int(off[k]):int(off[k + 1])], rec[int(off[k]):int(off[k + 1])]
            z = zscore(lev)
            if z is None:
                sys.stderr.write("squiggle_map: whole read: {} in read {} of {}\n".format(
                    "fewer than 2 events" if lev.size < 2 else "event levels without deviation", self.ids[i], self.input))
                continue
            t = int(best[q])
            h = records[t, q]
            y = self.targets[t][2]
            start = int(h["start"])
            span = whole_span(len(y), start, int(h["end"]), len(queries[i]), len(z), self.args.band)
            jobs.append((i, t, start, ev, lev, z, y[start:start + span]))
        if not jobs:
            return
        hits, span_off, spans = api.align_reads([j[5] for j in jobs], [j[6] for j in jobs], self.args.band, "free")
        for k, (i, t, start, ev, lev, z, _) in enumerate(jobs):
            sp = spans[int(span_off[k]):int(span_off[k + 1])]
            if hits["flags"][k] or sp[0, 0] < 0:
                sys.stderr.write("squiggle_map: whole read: the band lost the path in read {} of {}\n".format(self.ids[i], self.input))
                continue
            self.whole.write("".join(align_lines(self.ids[i], self.targets[t], ev, lev, z, sp + start)))
            if self.pile is not None and not self.pile_align:
                self.pile.add(z, ev, sp, t, start)                  # the spans as traced: inside target[start:]


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
    if args.band not in api.BAND_WIDTHS:
        parser.error("--band must be 64, 128 or 256")
    if args.band != 128 and not args.whole:
        parser.error("--band needs --whole")
    if bool(args.hits) != bool(args.secondary):
        parser.error("--hits and --secondary go together")
    if args.secondary and not 1 <= args.hits <= 64:
        parser.error("--hits must be in 1 .. 64")
    if args.max_dist_per_event is not None and (not args.hits or args.max_dist_per_event != args.max_dist_per_event):
        parser.error("--max_dist_per_event needs --hits and a number")
    if args.pileup_of == "whole" and not args.pileup:
        parser.error("--pileup_of needs --pileup")
    if args.pileup and args.pileup_of == "whole" and not args.whole:
        parser.error("--pileup_of whole needs --whole")
    try:
        targets = load_targets(args.model, args.both)
    except (ValueError, IndexError, OSError) as e:
        sys.stderr.write("squiggle_map: {}: {}\n".format(args.model, e))
        sys.exit(2)

    from . import _lib
    _lib.warm_start(args.device, also=())
    src = args.signal or args.blow5 or args.i16
    align = None
    if args.align:
        try:
            align = open(args.align, "w")
        except OSError as e:
            sys.stderr.write("squiggle_map: {}: {}\n".format(args.align, e))
            sys.exit(2)
        align.write("\t".join(ALIGN_HEADER) + "\n")
    whole = None
    if args.whole:
        try:
            whole = open(args.whole, "w")
        except OSError as e:
            sys.stderr.write("squiggle_map: {}: {}\n".format(args.whole, e))
            sys.exit(2)
        whole.write("\t".join(ALIGN_HEADER) + "\n")
    secondary = None
    if args.secondary:
        try:
            secondary = open(args.secondary, "w")
        except OSError as e:
            sys.stderr.write("squiggle_map: {}: {}\n".format(args.secondary, e))
            sys.exit(2)
        secondary.write("\t".join(SECONDARY_HEADER) + "\n")
    pileup = None
    if args.pileup:
        try:
            pileup = open(args.pileup, "w")
        except OSError as e:
            sys.stderr.write("squiggle_map: {}: {}\n".format(args.pileup, e))
            sys.exit(2)
    out = _Batcher(args, targets, src, align, whole, secondary, _Pile() if pileup is not None else None)
    sys.stdout.write("\t".join(HEADER) + "\n")
    try:
        if args.signal:
            for _, rid, sig in iter_tsv_reads(args.signal):
                out.add(rid, sig)
        elif args.blow5:
            from .blow5 import read_slow5
            for rec in read_slow5(args.blow5):
                out.add(rec["read_id"], rec["signal"])
        else:
            a = np.load(args.i16, mmap_mode="r")
            if a.ndim != 2 or a.dtype != np.int16:
                raise ValueError("need a 2-D int16 array, got {} {}".format(a.dtype, a.shape))
            for lo in range(0, a.shape[0], max(1, args.batch)):
                for i, row in enumerate(np.asarray(a[lo:lo + max(1, args.batch)])):
                    out.add(str(lo + i), row)
        out.flush()
        if pileup is not None:
            pileup.write(out.pile.table(targets))
    except (ValueError, EOFError, OSError) as e:
        sys.stdout.flush()
        sys.stderr.write("squiggle_map: {}: {}\n".format(src, e))
        for fh in (align, whole, secondary, pileup):
            if fh is not None:
                fh.close()
        sys.exit(2)
    sys.stdout.flush()
    for fh in (align, whole, secondary, pileup):
        if fh is not None:
            fh.close()


if __name__ == "__main__":
    main()
