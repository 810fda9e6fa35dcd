"""Drop-in for /root/reference/MotifSeq.py's command line (MotifSeq.py:80-311, 431-449).

Same flags, the same stderr banner, the same 12/13-column TSV on stdout.  Per read,
scale_outliers + medmad/zscale + dtw_subsequence run on the GPU (batched, C ABI);
the scoring of MotifSeq.py:441-445 stays in Python so the printed floats are the
reference's digit for digit.  fast5 input (-f / -p) goes through h5py when it is importable and
through the built-in reader (hdf5min.py) otherwise, with the reference's stderr messages.
Additive flags: --device, --gpus, --batch, --after_stall, --strict-compat, --blow5, --i16, --hits, --min_hit_p, --paths,
--background, --max_local_Z, --region, --panel, --pool.
Whole chunks of plain integer reads (TSV chunks, BLOW5 / packed blocks) go to the GPU as one batch and their rows are
formatted natively (csrc/sk_io.cpp writes floats as Python does); anything unusual takes the per-read route.
"""
import argparse
import os
import sys

import numpy as np

from . import _lib, api, fastio, tsvio
from ._warm import mark as _mark, Stats as _Stats

_KEEP = []       # input mappings / page-locked buffers of a finished reader: released with the process

VERSION = "1.3.0"          # the reference's MotifSeq version string (MotifSeq.py:84)
HEADER = ["fast5", "readID", "model", "start", "end", "length", "distance_score", "model_mean",
          "model_stdev", "Z-score", "p-value", "hit_Probability"]
BANNER = ("\n\n**********************************************************\n"
          "*  z-score, p-value, probability, etc. are based on      *\n"
          "*     preliminary experimental modeling only             *\n"
          "*                Use at own risk                         *\n"
          "**********************************************************\n\n\n")
NO_SIGNAL = "No Signal found - please check signal format\n"      # MotifSeq.py:271-273


class _Parser(argparse.ArgumentParser):
    def error(self, message):                      # MotifSeq.py:73-77
        sys.stderr.write("error: %s\n" % message)
        self.print_help()
        sys.exit(2)


def build_parser():
    p = _Parser(description="MotifSeq (MI355X) - find a sequence motif's signal inside raw nanopore reads")
    src = p.add_mutually_exclusive_group()
    mod = p.add_mutually_exclusive_group()
    src.add_argument("-f", "--f5f", help="text file listing fast5 paths")
    src.add_argument("-p", "--f5_path", help="directory searched recursively for fast5 files")
    src.add_argument("-s", "--signal", help="signal TSV written by SquigglePull (.gz accepted)")
    src.add_argument("--blow5", help="[extension] BLOW5 file (stored or zlib records): raw ADC values, decoded natively")
    src.add_argument("--i16", help="[extension] packed reads: a .npy file holding an int16 array [reads, samples] "
                                   "(readID = row index)")
    p.add_argument("-l", "--scale", default="medmad", choices=["zscale", "medmad"],
                   help="per-read normalisation applied before the search")
    mod.add_argument("-i", "--fasta_input", help="fasta of motifs, turned into squiggles with scrappy")
    p.add_argument("--scrappie_model", default="squiggle_r94",
                   choices=["squiggle_r94", "squiggle_r94_rna", "squiggle_r10"],
                   help="scrappie squiggle model used for -i")
    mod.add_argument("-m", "--model", help="pre-computed motif signal: scrappie squiggle text or name/len/x/values TSV")
    p.add_argument("-x", "--sig_extract", action="store_true", help="append the matched normalised signal")
    p.add_argument("--after_stall", action="store_true",
                   help="[extension] run the segmenter first and search only the signal after its first segment "
                        "(the stall); coordinates then index that slice and a last column `search_from` gives "
                        "the raw sample index where it starts")
    p.add_argument("--slope", type=float, default=2.90, help="[experimental] distance model slope")
    p.add_argument("--intercept", type=float, default=-9.6, help="[experimental] distance model intercept")
    p.add_argument("--std_const", type=float, default=0.08468, help="[experimental] distance model stdev factor")
    p.add_argument("-v", "--view", action="store_true", help="plot each hit (not available in this build)")
    p.add_argument("--save", help="directory for hit images (not available in this build)")
    p.add_argument("--img", default="png", help="image type for --save")
    p.add_argument("-scale_hi", "--scale_hi", type=int, default=1200, help="samples >= this are dropped")
    p.add_argument("-scale_low", "--scale_low", type=int, default=0, help="samples <= this are dropped")
    p.add_argument("-V", "--version", action="store_true", help="print the version and exit")
    p.add_argument("--verbose", action="store_true", help="dump the parsed arguments to stderr")
    p.add_argument("--device", type=int, default=None, help="[extension] GPU index (default $SK_DEVICE or 0)")
    p.add_argument("--batch", type=int, default=2048, help="[extension] reads per GPU call")
    p.add_argument("--gpus", type=int, default=1,
                   help="[extension] shard every batch of reads over this many GPUs of the node")
    p.add_argument("--stats-json", dest="stats_json", default=None, metavar="PATH",
                   help="[extension] write reads / reads per second / input GB per second / GPU calls of this run to PATH "
                        "as JSON (also $SK_STATS_JSON); stdout and stderr stay the reference's")
    p.add_argument("--stats", action="store_true", help="[extension] the same as one line on stderr at the end")
    p.add_argument("--strict-compat", action="store_true",
                   help="[extension] keep the reference's -m defect (empty model order: header only)")
    p.add_argument("--hits", type=int, default=None, metavar="K",
                   help="[extension] up to K non-overlapping matches per read and motif (1..64), best first")
    p.add_argument("--min_hit_p", type=float, default=None, metavar="P",
                   help="[extension] with --hits: leave out the lines whose hit_Probability is below P")
    p.add_argument("--paths", default=None, metavar="FILE",
                   help="[extension] write to FILE, per printed hit and motif base, the samples the alignment path gives "
                        "that base (start, end, length, mean normalised signal); stdout is unchanged")
    p.add_argument("--background", default=None, metavar="FILE",
                   help="[extension] write to FILE, per printed line, the read's own background for that motif -- mean, "
                        "stdev, median and MAD of the whole last DTW row (view_region's M and S, MotifSeq.py:507-513) -- "
                        "and the hit's local_Z and robust_Z against it; stdout is unchanged")
    p.add_argument("--max_local_Z", type=float, default=None, metavar="Z",
                   help="[extension] with --background: leave out the lines whose local_Z is above Z")
    p.add_argument("--pool", default=None, metavar="FILE",
                   help="[extension] write to FILE after the run, per model and motif point, the model the printed hits show "
                        "when pooled: hits, level (sample weighted), its spread over the hits, the noise inside an event, "
                        "dwell and cost; stdout is unchanged")
    p.add_argument("--region", default=None, metavar="A:B",
                   help="[extension] search only the raw samples [A:B] of every read, cut as a Python slice before the outlier "
                        "filter (either side may be empty or negative: 0:2000, --region=-3000:); coordinates then index "
                        "that slice and a last column `search_from` gives the raw sample index where it starts")
    p.add_argument("--panel", action="store_true",
                   help="[extension] two or more motifs: one row per read naming the motif with the smallest Z-score, the "
                        "runner-up and their difference (ranked on the GPU)")
    return p


def parse_region(parser, text):
    """'A:B' -> (begin, end); an empty side is None."""
    parts = text.split(":")
    try:
        if len(parts) != 2:
            raise ValueError(text)
        begin, end = (None if x.strip() == "" else int(x) for x in parts)
    except ValueError:
        parser.error("--region takes A:B with integer or empty sides, got {!r}".format(text))
    if any(v is not None and not -2 ** 31 <= v < 2 ** 31 - 1 for v in (begin, end)):
        parser.error("--region bounds must fit int32")
    return (0 if begin is None else begin, end)


PANEL_HEADER = ["fast5", "readID", "best_model", "start", "end", "length", "distance_score", "Z-score", "p-value",
                "hit_Probability", "second_model", "second_Z", "delta_Z", "search_from"]
BACKGROUND_HEADER = ["fast5", "readID", "model", "hit", "distance_score", "row_mean", "row_stdev", "local_Z", "row_median",
                     "row_mad", "robust_Z", "below_1sd", "n"]
POOL_HEADER = ["model", "point", "pos", "base", "model_current", "hits", "level", "level_sd", "sd_mean", "dwell_mean",
               "dwell_sd", "cost_mean"]
PATHS_HEADER = ["fast5", "readID", "model", "hit", "pos", "base", "model_current", "start", "end", "length", "mean_signal"]


def check_hit_flags(parser, args):
    """--hits / --min_hit_p / --paths / --background / --max_local_Z: what they take, and what they do not combine
    with."""
    if args.max_local_Z is not None and args.background is None:
        parser.error("--max_local_Z needs --background")
    if args.max_local_Z is not None and args.max_local_Z != args.max_local_Z:
        parser.error("--max_local_Z is NaN (with --background)")
    if args.background is not None and args.after_stall:
        parser.error("--background does not combine with --after_stall")
    if args.background is not None and args.panel:
        parser.error("--background writes one line per printed hit: it does not combine with --panel")
    if args.paths is not None and args.after_stall:
        parser.error("--paths does not combine with --after_stall")
    if args.pool is not None and args.after_stall:
        parser.error("--pool does not combine with --after_stall")
    if args.pool is not None and args.panel:
        parser.error("--pool pools the printed hits: it does not combine with --panel")
    if args.hits is not None and not 1 <= args.hits <= 64:
        parser.error("--hits must be between 1 and 64")
    if args.min_hit_p is not None and args.hits is None:
        parser.error("--min_hit_p needs --hits")
    if args.hits is not None and args.after_stall:
        parser.error("--hits does not combine with --after_stall")
    if args.region is not None and args.after_stall:
        parser.error("--region does not combine with --after_stall")
    args.region = None if args.region is None else parse_region(parser, args.region)
    if args.panel and (args.hits is not None or args.paths is not None or args.sig_extract or args.after_stall):
        parser.error("--panel prints one row per read: it does not combine with --hits, --paths, -x or --after_stall")


def norm_cdf(z):
    """scipy.stats.norm.cdf == scipy.special.ndtr (MotifSeq.py:444), the same doubles without the 0.1-0.35 s that
    importing scipy.special costs every run: fastio.ndtr (csrc/sk_io.cpp) restates the Cephes routine scipy uses."""
    return fastio.ndtr(z)


class DistanceModel:
    """The scoring of MotifSeq.py:441-445.  mean[c] = slope * L_c + intercept and stdev[c] = mean[c] * std_const per
    motif, made once; score() turns distances into the three printed scores."""

    def __init__(self, args, lens):
        self.mean = np.array([(args.slope * n) + args.intercept for n in lens], dtype=np.float64)
        self.stdev = self.mean * args.std_const

    def score(self, dist, c):
        """(Z-score, p-value, hit_Probability) of distances to motif(s) c -- a scalar and an index, or arrays of both:
        the same IEEE operations in the same order either way, so the same digits."""
        with np.errstate(all="ignore"):
            z = (dist - self.mean[c]) / self.stdev[c]
            p_value = norm_cdf(z)
            return z, p_value, (1 - p_value) * 100


def load_models(args):
    if args.model:
        models, order, lens = tsvio.read_model_auto(args.model)
        if args.strict_compat:
            order, lens = [], []                     # MotifSeq.py:413-428 never fills them
        elif order:
            sys.stderr.write("MotifSeq: note: -m searches for the model's motif(s); the reference's read_bait_model "
                             "never registers them and prints the header only (--strict-compat reproduces that)\n")
        return models, order, lens
    if args.fasta_input:
        try:
            return tsvio.fasta_to_models(args.fasta_input, args.scrappie_model)
        except ImportError:
            side = os.path.splitext(args.fasta_input)[0] + ".model"
            if os.path.exists(side):
                sys.stderr.write("MotifSeq: scrappy is not installed; using the pre-computed scrappie "
                                 "squiggle {}\n".format(side))
                return tsvio.read_scrappie_model(side)
            sys.stderr.write("MotifSeq: -i needs the scrappy package (not installed) or a scrappie squiggle "
                             "file next to the fasta; use -m <file.model>\n")
            sys.exit(1)
    return {}, [], []


_STATS = [_Stats("MotifSeq")]       # this run's throughput counters (--stats-json / --stats)


def skipped(read_id, flags, mad_tail=""):
    """The stderr line of a read the search left out -- flag 1: no sample survived the filter, flag 2: MAD = 0 (mad_tail:
    what the caller adds to that line).  False, and nothing written, for any other read."""
    if flags & 1:
        sys.stderr.write("MotifSeq: no sample of {} survived the outlier limits; skipped\n".format(read_id))
    elif flags & 2:                                              # SK_FLAG_DEGENERATE
        sys.stderr.write("MotifSeq: the MAD of {} is 0 (medmad divides by it, MotifSeq.py:196-199); "
                         "skipped{}\n".format(read_id, mad_tail))
    else:
        return False
    return True


def first_matches(recs):
    """One record per read and motif (recs[c][r]) in the shape of a hit list: per motif (records [n, 1], count 1)."""
    return [(h[:, None], np.ones(len(h), dtype=np.int32)) for h in recs]


class _Batcher:
    """Reads in, lines out.  A search result has one shape on every route: per motif (records [n, K], count [n]) --
    first match is K = 1, count 1 -- and slot 0 carries the read's flags."""

    def __init__(self, args, models, order, lens):
        self.args, self.models, self.order = args, models, order
        self.motifs = [np.asarray(models[name], dtype=np.float64) for name in order]
        self.model = DistanceModel(args, lens)
        names = [nm.encode() for nm in order] + [b"."]              # ("." = index -1: the panel's missing runner-up)
        noff = np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.int64)
        self.name_blob, self.name_span = b"".join(names), np.stack([noff[:-1], noff[1:]], axis=1)
        self.meta, self.sigs = [], []
        self._pending, self._worker = None, None
        self.pooled = {name: [] for name in order}    # --pool: per model the events [N] of every printed hit
        # --paths / --background / --pool work per printed line: every read takes the per-read route (emit)
        self.per_line = args.paths is not None or args.background is not None or args.pool is not None
        # --region / --panel: every read goes through the per-read queue (add / flush), --batch reads per GPU call
        self.queued = args.region is not None or args.panel
        # --paths / --pool: base table per model (scrappie text)
        self.bases = {}
        if (args.paths is not None or args.pool is not None) and args.model:
            self.bases = tsvio.model_bases_auto(args.model)
        if args.pool is not None:
            open(args.pool, "w").close()              # (an unwritable FILE fails before the run, not after it)
        self.paths_fh = self.side_file(args.paths, PATHS_HEADER)
        self.background_fh = self.side_file(args.background, BACKGROUND_HEADER)

    @staticmethod
    def side_file(path, header):
        if path is None:
            return None
        fh = open(path, "w")
        fh.write("\t".join(header) + "\n")
        return fh

    def close(self):
        """The end of the input: what is still queued, then the side files."""
        self.drain()
        self.flush()
        for fh in (self.paths_fh, self.background_fh):
            if fh is not None:
                fh.close()
        if self.args.pool is not None:
            sys.stdout.flush()
            self.pool_table(self.args.pool)

    def search(self, route, *batch):
        """The GPU call of one batch through api.motifseq_{multi,hits,paths,background,events}<route> (route: "" per read,
        "_batch" packed int16 rows, "_ragged_f64" ragged values; looked up when called): (hit lists per motif, spans
        per motif or None, background records per motif or None, events per motif or None).  --paths takes the paths call
        -- hit lists plus spans -- and --background the background call -- hit lists plus each read's row statistics;
        without --hits their rank-1 records stand in for the default path's (the same records bit for bit).  --pool takes
        the events call, whose records also give the spans of --paths."""
        a = self.args
        tail = (a.scale, a.scale_low, a.scale_hi)

        def call(family):
            return getattr(api, "motifseq_" + family + route)(*batch, self.motifs, a.hits or 1, float("inf"), *tail)
        spans = bgs = evs = None
        if a.background is not None:
            res = call("background")
            bgs = [b for _, _, b in res]
        if a.pool is not None:
            # (with --background this is a second search of the batch: no entry point returns row statistics and events
            # together yet.  Both calls give the same hit lists bit for bit; the events call's are the ones printed.)
            res = call("events")
            evs = [ev for _, _, ev in res]
            if a.paths is not None:
                spans = [api.spans_of_events(ev) for ev in evs]
        elif a.paths is not None:
            res = call("paths")
            spans = [sp for _, _, sp in res]
        elif a.background is None and a.hits is not None:
            res = call("hits")
        elif a.background is None:
            res = first_matches(getattr(api, "motifseq_multi" + route)(*batch, self.motifs, *tail))
        if a.hits is None:                            # first match: rank 1 of whatever the family listed, count 1
            return first_matches([r[0][:, 0] for r in res]), spans, bgs, evs
        return [r[:2] for r in res], spans, bgs, evs

    def pool_table(self, path):
        """--pool: one pool_events call per model over the events of its printed hits, one line per motif point."""
        with open(path, "w") as fh:
            fh.write("\t".join(POOL_HEADER) + "\n")
            for name in self.order:
                motif = self.models[name]
                evs = self.pooled[name]
                pool = api.pool_events(np.stack(evs) if evs else api.no_events((0, len(motif))))
                where = {}
                for pos, base, _, first, cnt in self.bases.get(name) or []:
                    for i in range(first, first + cnt):
                        where[i] = (pos, base)
                for i, rec in enumerate(pool):
                    pos, base = where.get(i, (".", "."))
                    row = (name, i, pos, base, float(motif[i]), int(rec["hits"]), float(rec["level"]), float(rec["level_sd"]),
                           float(rec["sd_mean"]), float(rec["dwell_mean"]), float(rec["dwell_sd"]), float(rec["cost_mean"]))
                    fh.write("\t".join("{}".format(v) for v in row) + "\n")

    def background_line(self, fast5, read_id, name, rank, dist, bg, local_z, robust_z):
        """One line of the --background file for one printed hit."""
        row = (fast5, read_id, name, rank, dist, float(bg["mean"]), float(bg["std"]), local_z, float(bg["median"]),
               float(bg["mad"]), robust_z, int(bg["below"]), int(bg["n"]))
        self.background_fh.write("\t".join("{}".format(v) for v in row) + "\n")

    def path_lines(self, fast5, read_id, name, rank, spans, norm):
        """One line per base of the model (per motif point when it has no base table) for one printed hit."""
        motif = self.models[name]
        table = self.bases.get(name) or [(i, ".", float(motif[i]), i, 1) for i in range(len(motif))]
        out = []
        for pos, base, current, first, cnt in table:
            if cnt == 0 or spans[0, 0] < 0:
                lo, hi, length, mean = -1, -1, 0, float("nan")
            else:
                lo, hi = int(spans[first, 0]), int(spans[first + cnt - 1, 1])
                length, mean = hi - lo + 1, np.mean(norm[lo:hi + 1])
            out.append("\t".join("{}".format(v) for v in (fast5, read_id, name, rank, pos, base, current, lo, hi, length, mean)))
        self.paths_fh.write("\n".join(out) + "\n")

    def add(self, fast5, read_id, sig):
        self.meta.append((fast5, read_id))
        self.sigs.append(sig)
        if len(self.sigs) >= self.args.batch:
            self.flush()

    def note(self, message):
        """A stderr message that must keep its place between the reads around it."""
        self.meta.append((None, message))
        self.sigs.append(None)

    def entries(self, sig_of=lambda r: None, cut_of=lambda r: None):
        """The queue in order as deliver() takes it: (fast5, readID, slot among the queued reads, signal, cut) per read,
        (None, message, ...) per note."""
        r = 0
        for (fast5, read_id), sig in zip(self.meta, self.sigs):
            if sig is None:
                yield None, read_id, None, None, None
            else:
                yield fast5, read_id, r, sig_of(r), cut_of(r)
                r += 1

    def deliver(self, entries, hits, spans=None, bgs=None, evs=None):
        """The per-read route over a searched batch: every read's rows from its slices of the batch's results, every
        note to stderr in its place."""
        for fast5, read_id, r, sig, cut in entries:
            if fast5 is None:
                sys.stderr.write(read_id)
                continue
            self.emit(fast5, read_id, [(h[r], cnt[r]) for h, cnt in hits], sig, cut,
                      *(None if per_motif is None else [v[r] for v in per_motif] for per_motif in (spans, bgs, evs)))

    def flush(self):
        self.drain()                                  # (a pipelined block's table comes first)
        if not self.sigs:
            return
        a = self.args
        sigs = [s for s in self.sigs if s is not None]
        if sigs:
            _STATS[0].batch(len(sigs))
        if self.queued and sigs:
            self.flush_region(sigs)
        else:
            cuts = None
            if a.after_stall and sigs:                # [extension] search only after the segmenter's first segment
                cuts = api.stall_cuts(sigs)
                sigs = [np.asarray(s)[c:] for s, c in zip(sigs, cuts)]
            self.deliver(self.entries(lambda r: sigs[r], lambda r: None if cuts is None else int(cuts[r])),
                         *(self.search("", sigs) if sigs else ([],)))
        self.meta, self.sigs = [], []

    def windows(self, sigs, region):
        """The reads cut to the region: (windows, raw index each starts at).  Integer reads are gathered on the GPU
        (api.region_rows), the rest sliced here -- the same slice either way."""
        out, frm = [None] * len(sigs), np.zeros(len(sigs), dtype=np.int64)
        ints, arrs, flts = api._split_int16(sigs)
        if ints:
            rows, wlen, f = api.region_rows(*api.pack_i16(arrs), region)
            for k, i in enumerate(ints):
                out[i], frm[i] = rows[k, :wlen[k]], f[k]
        for i in flts:
            s = np.asarray(sigs[i])
            lo, hi = slice(*region).indices(s.size)[:2]
            out[i], frm[i] = s[lo:hi], lo
        return out, frm

    def flush_region(self, sigs):
        """--region / --panel over the queued reads.  --hits / --paths: the window rows go to the existing hit-list and
        path calls; otherwise the panel call searches every motif inside the region in one GPU call."""
        a = self.args
        region = a.region if a.region is not None else (0, None)
        panel = (self.motifs, self.model.mean, self.model.stdev, region, None, a.scale, a.scale_low, a.scale_hi)
        if a.panel:
            recs, frm = api.motifseq_panel(sigs, *panel)
            keep = []
            for fast5, read_id, r, _, _ in self.entries():
                if fast5 is None:
                    self.panel_table(keep, recs, frm)
                    keep = []
                    sys.stderr.write(read_id)
                elif recs[r]["best"] >= 0:
                    keep.append((fast5, read_id, r))
                elif not skipped(read_id, int(recs[r]["hit"]["flags"])):
                    sys.stderr.write("MotifSeq: no motif has a finite score in {}; skipped\n".format(read_id))
            self.panel_table(keep, recs, frm)
            return
        if a.hits is not None or self.per_line:
            wins, frm = self.windows(sigs, region)
            found = self.search("", wins)
            sig_of = wins.__getitem__
        else:
            _, frm, recs = api.motifseq_panel(sigs, *panel, records=True)
            found = (first_matches(recs),)

            def sig_of(r):                                                  # (-x / --strict-compat normalise the slice)
                return np.asarray(sigs[r])[slice(*region)] if (a.sig_extract or a.strict_compat) else None
        self.deliver(self.entries(sig_of, lambda r: int(frm[r])), *found)

    def panel_table(self, keep, recs, frm):
        """The --panel rows of the reads in `keep` [(fast5, readID, slot)] through the native formatter: the GPU's scores,
        scipy's ndtr restated (fastio.ndtr) and Python's float text (fastio.fmt_rows)."""
        if not keep:
            return
        idx = np.array([r for _, _, r in keep], dtype=np.int64)
        rec = recs[idx]

        def strs(items):
            enc = [x.encode() if isinstance(x, str) else bytes(x) for x in items]
            return ("str", b"".join(enc), np.concatenate([[0], np.cumsum([len(x) for x in enc])]).astype(np.int64))
        z, z2 = rec["score_best"], rec["score_second"]
        with np.errstate(all="ignore"):
            pv = norm_cdf(z)
            hp = (1 - pv) * 100
            dz = z2 - z
        h = rec["hit"]
        cols = [strs([k[0] for k in keep]), strs([k[1] for k in keep]), ("span", self.name_blob, self.name_span[rec["best"]]),
                ("i32", h["start"]), ("i32", h["end"]), ("i32", h["end"] - h["start"]), ("f64", h["dist"]), ("f64", z),
                ("f64", pv), ("f64", hp), ("span", self.name_blob, self.name_span[rec["second"]]), ("f64", z2), ("f64", dz),
                ("i32", frm[idx])]
        fastio.write_stdout(fastio.fmt_rows(len(keep), cols))

    def emit(self, fast5, read_id, hits, sig, cut, spans=None, bgs=None, evs=None):
        """The rows of one read, one per motif and match, best first (MotifSeq.py:436-449).  hits: per motif the read's
        (records [K], count).
        spans (--paths): per motif the read's [K, N, 2]; every printed hit also writes its lines to the paths file.
        bgs (--background): per motif the read's background record; every printed hit also writes its line to the
        background file, and --max_local_Z leaves out of both the hits that score above it.
        evs (--pool): per motif the read's events [K, N]; those of every printed hit are kept for the pool table."""
        a = self.args
        norm = None
        for c, name in enumerate(self.order):
            recs, count = hits[c]
            flags = int(recs[0]["flags"])
            if flags & 1 or (flags & 2 and not a.strict_compat):
                skipped(read_id, flags, " (--strict-compat prints the reference's nan row)")
                break
            if flags & 2:
                # the reference divides by zero and hands inf / nan to mlpy: the same division, then mlpy's C arithmetic
                # evaluated literally on the GPU (sk_dtw_subsequence_cref) -- a nan distance at the first sample that
                # equals the median
                if norm is None:
                    norm = api.normalise(sig, a.scale, a.scale_low, a.scale_hi)
                try:
                    found = [api.dtw_subsequence_cref(self.motifs[c], norm)]
                except _lib.SquiggleKitError as e:
                    if e.code != -5:                                # SK_ERR_UNSUPPORTED: more than 2^28 cells of cost matrix
                        raise
                    sys.stderr.write("MotifSeq: {} has MAD 0 and is too long for the literal evaluation of the reference's "
                                     "nan row ({} samples x {} points); skipped\n".format(read_id, len(norm), len(self.models[name])))
                    break
            else:
                found = [(float(x["dist"]), int(x["start"]), int(x["end"])) for x in recs[:count]]
            for rank, (dist, start, end) in enumerate(found):
                z, p_value, hit_p = self.model.score(dist, c)
                if a.min_hit_p is not None and hit_p < a.min_hit_p:
                    continue
                if bgs is not None:
                    local_z, robust_z = (float(v) for v in api.local_scores(dist, bgs[c]))
                    if a.max_local_Z is not None and local_z > a.max_local_Z:
                        continue
                row = [fast5, read_id, name, start, end, end - start, dist, self.model.mean[c], self.model.stdev[c], z,
                       p_value, hit_p]
                if a.sig_extract:
                    if norm is None:
                        norm = api.normalise(sig, a.scale, a.scale_low, a.scale_hi)
                    row.append("\t".join(str(v) for v in norm[start:end]))
                if cut is not None:
                    row.append(cut)
                print("\t".join("{}".format(v) for v in row))
                if bgs is not None:
                    self.background_line(fast5, read_id, name, rank + 1, dist, bgs[c], local_z, robust_z)
                if spans is not None and not flags & 2:
                    if norm is None:
                        norm = api.normalise(sig, a.scale, a.scale_low, a.scale_hi)
                    self.path_lines(fast5, read_id, name, rank + 1, spans[c][rank], norm)
                if evs is not None and not flags & 2:
                    self.pooled[name].append(evs[c][rank])

    def table(self, n, fast5_col, id_col, hits):
        """The rows of n reads through the native formatter (file order, read-major): per read and motif its `count`
        matches in rank order, lines below --min_hit_p left out.  fast5_col / id_col: one entry per read.  Returns
        False -- nothing written -- when some read needs the per-read route (-x, a side file, a flagged read)."""
        a = self.args
        K = len(self.order)
        if a.sig_extract or self.per_line or any(bool((h[:, 0]["flags"] & 3).any()) for h, _ in hits):
            return False
        mean, stdev, names = self.model.mean, self.model.stdev, self.name_span[:K]
        if all(bool((cnt == 1).all()) for _, cnt in hits):
            # first match (or one match everywhere): the lines are the (read, motif) pairs as they stand, so the columns
            # are [n, K] arrays scored by broadcasting and the per-motif ones tiled.  (The gathers of the general case
            # cost 0.4 ms per block of 16 384 reads, 3 % of the packed routes' runs.)
            ri = None if K == 1 else np.repeat(np.arange(n), K)
            dist, start, end = (np.stack([h[:, 0][f] for h, _ in hits], axis=1) for f in ("dist", "start", "end"))
            lines = [v.ravel() for v in (start, end, dist) + self.model.score(dist, slice(None))]
            lines += [np.tile(mean, n), np.tile(stdev, n), np.tile(names, (n, 1))]
        else:
            cnt = np.stack([c for _, c in hits], axis=1).ravel().astype(np.int64)    # per (read, motif), read-major
            pair = np.repeat(np.arange(n * K), cnt)
            rank = np.arange(pair.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            ri, ci = pair // K, pair % K
            sel = np.stack([h for h, _ in hits], axis=1)[ri, ci, rank]           # [n, K motifs, slots] -> lines
            lines = [sel["start"], sel["end"], sel["dist"], *self.model.score(sel["dist"], ci), mean[ci], stdev[ci], names[ci]]
        if a.min_hit_p is not None:
            keep = ~(lines[5] < a.min_hit_p)
            ri = np.flatnonzero(keep) if ri is None else ri[keep]
            lines = [v[keep] for v in lines]
        start, end, dist, z, pv, hp, mean, stdev, names = lines

        def each_line(col):                                                  # one entry per read -> one per line
            if ri is None or col[0] == "const":
                return col
            return col[:-1] + (np.asarray(col[-1])[ri],)
        cols = [each_line(fast5_col), each_line(id_col), ("span", self.name_blob, names), ("i32", start), ("i32", end),
                ("i32", end - start), ("f64", dist), ("f64", mean), ("f64", stdev), ("f64", z), ("f64", pv), ("f64", hp)]
        if dist.size:
            fastio.write_stdout(fastio.fmt_rows(int(dist.size), cols))
        return True

    def submit(self, kind, route, batch, n, fast5_col, id_col, name_of, id_of, sig_of):
        """One block of n reads to the GPU worker.  One block deep pipeline: the search of this block runs on the worker
        thread while the previous block's table is written (drain() at the end); name_of / id_of / sig_of(i) give read
        i to the per-read route should the block need it."""
        if self._worker is None:
            from concurrent.futures import ThreadPoolExecutor
            self._worker = ThreadPoolExecutor(1)
        _mark("block of %d %sreads to the GPU worker" % (n, kind))

        def call():
            _mark("GPU call starts")
            try:
                return self.search(route, *batch)
            finally:
                _mark("GPU call ends")
        prev, self._pending = self._pending, (self._worker.submit(call), n, fast5_col, id_col, name_of, id_of, sig_of)
        if prev is not None:
            self._finish(prev)

    def rows(self, rows, nsamp, fast5_col, id_col, name_of, id_of):
        """A block of plain int16 reads (BLOW5 / packed input, a TSV chunk): one GPU batch, native table; the per-read
        route only when a read is flagged.  The caller keeps `rows` alive one call longer (submit())."""
        if not len(nsamp):
            return
        a = self.args
        if a.after_stall or self.queued:
            # get_segs first, then the search behind the stall: the per-read queue does that (api.motifseq_after_stall,
            # up to --batch reads per GPU call) and prints the search_from column; `rows` is reused by the reader
            self.drain()
            for i in range(len(nsamp)):
                self.add(name_of(i), id_of(i), np.array(rows[i, :nsamp[i]], dtype=np.float64))
            return
        self.submit("", "_batch", (rows, nsamp), len(nsamp), fast5_col, id_col, name_of, id_of,
                    lambda i, r=rows, ns=nsamp: r[i, :ns[i]])
        if a.sig_extract or a.paths is not None:            # (they normalise on the GPU from this thread: no overlap)
            self.drain()

    def rows_f64(self, fb):
        """A chunk of plain decimal (pA) lines as the float64 tokenizer leaves it (tsvio.FloatBlock: flat values +
        offsets): one GPU batch, one native table, pipelined like rows()."""
        self.submit("float64 ", "_ragged_f64", (fb.batch_values(), fb.off), fb.n, ("span", fb.buf, fb.spans("name")),
                    ("span", fb.buf, fb.spans("id")), lambda i: fb.text("name", i), lambda i: fb.text("id", i),
                    lambda i: fb.values[fb.off[i]:fb.off[i + 1]])

    def drain(self):
        prev, self._pending = self._pending, None
        if prev is not None:
            self._finish(prev)

    def _finish(self, p):
        job, n, fast5_col, id_col, name_of, id_of, sig_of = p
        found = job.result()
        _STATS[0].batch(n)
        _mark("block of %d reads back from the GPU" % n)
        if self.table(n, fast5_col, id_col, found[0]):
            _mark("table written")
            return
        if self._pending is not None and (self.args.sig_extract or self.args.strict_compat):
            # emit() may call the GPU from THIS thread (api.normalise, api.dtw_subsequence_cref for a MAD = 0 read under
            # --strict-compat) while the worker runs the next block on the same device context -- one stream, one set
            # of scratch buffers, no lock: the next block's call has to be over first (its result stays in the future)
            self._pending[0].exception()
        need_sig = self.args.sig_extract or self.args.strict_compat or found[1] is not None
        self.deliver(((name_of(i), id_of(i), i, sig_of(i) if need_sig else None, None) for i in range(n)), *found)

    def block(self, blk):
        """A parsed TSV chunk (tsvio.TsvBlock): its integer lines go to the GPU as ONE int16 batch straight from the
        tokenizer's rows (every motif against them); any other line takes the per-read route, in its place."""
        a = self.args
        queue = a.after_stall or self.per_line or self.queued               # (they need the raw reads on the host)
        fast = (blk.flags & 27) == 3                                        # ALLINT | ANY, not SLOW / SHORT
        if queue:
            fast[:] = False
        idx = np.flatnonzero(fast)
        no = blk.base + blk._no.astype(np.int64)
        io = blk.base + blk._io.astype(np.int64)
        name_span, id_span = np.stack([no, no + blk._nl], axis=1), np.stack([io, io + blk._il], axis=1)
        if idx.size == blk.n and blk.n and not a.sig_extract:
            # every line of the chunk is a plain integer read: one GPU batch, the whole table in one native call,
            # pipelined with the next chunk (rows())
            self.rows(blk.rows, blk.nsamp, ("span", blk.buf, name_span), ("span", blk.buf, id_span), blk.name, blk.read_id)
            return
        self.drain()                                                        # (what follows prints directly)
        slot = np.full(blk.n, -1, dtype=np.int64)                           # line -> its row in the batch of fast lines
        direct = np.zeros(blk.n + 1, dtype=bool)                            # lines the table writer prints as they stand
        if idx.size:
            hits = self.search("_batch", blk.rows[idx] if idx.size != blk.n else blk.rows, blk.nsamp[idx])[0]
            slot[idx] = np.arange(idx.size)
            if not a.sig_extract:
                direct[idx] = ~np.any([(h[:, 0]["flags"] & 3) != 0 for h, _ in hits], axis=0)
        i = 0
        while i < blk.n:
            if direct[i]:
                # a run of consecutive such lines: one table (consecutive lines of the chunk are consecutive rows of
                # the batch)
                j = i + int(np.argmin(direct[i:]))
                lo, hi = int(slot[i]), int(slot[i]) + j - i
                self.table(j - i, ("span", blk.buf, name_span[i:j]), ("span", blk.buf, id_span[i:j]),
                           [(h[lo:hi], cnt[lo:hi]) for h, cnt in hits])
                i = j
                continue
            fl = int(blk.flags[i]) & 27
            if slot[i] >= 0:                                                # the general route: -x, flagged reads
                sig = blk.rows[i, :blk.nsamp[i]] if (a.sig_extract or a.strict_compat) else None
                self.deliver([(blk.name(i), blk.read_id(i), int(slot[i]), sig, None)], hits)
            elif fl == 1:                                                   # integers, all zero
                self.note(NO_SIGNAL)
            elif fl == 3:
                self.add(blk.name(i), blk.read_id(i), blk.rows[i, :blk.nsamp[i]].astype(np.float64))
            else:
                fast5, read_id, sig = tsvio.parse_motifseq_line(blk.line(i).decode())   # the reference's own parse
                if sig.any():
                    self.add(fast5, read_id, sig)
                else:
                    self.note(NO_SIGNAL)
            if not queue:
                # lines of this chunk were printed directly: each other one goes out in its place.  (Otherwise the queue
                # alone keeps the file order: reads wait for up to --batch per GPU call.)
                self.flush()
            i += 1


def main(argv=None):
    parser = build_parser()
    argv = sys.argv[1:] if argv is None else argv
    args = parser.parse_args(argv)
    check_hit_flags(parser, args)
    if len(argv) == 0:                               # MotifSeq.py:129-131
        parser.print_help(sys.stderr)
        sys.exit(1)
    if args.version:                                 # MotifSeq.py:134-136
        sys.stderr.write("SquiggleKit MotifSeq: {}\n".format(VERSION))
        sys.exit(1)
    if args.verbose:
        sys.stderr.write("Verbose mode active - dumping info to stderr\n")
        sys.stderr.write("SquiggleKit MotifSeq: {}\n".format(VERSION))
        sys.stderr.write("args: {}\n".format(args))
    sys.stderr.write(BANNER)                         # MotifSeq.py:147-151
    if args.view or args.save:
        sys.stderr.write("MotifSeq: -v/--save plotting is not part of this build; ignoring\n")

    _mark("main() entered")
    _STATS[0] = _Stats("MotifSeq")
    del _KEEP[:]                                     # (a previous call in this process: its buffers can go now)
    models, order, lens = load_models(args)
    _mark("models loaded")
    if args.panel and len(order) < 2:
        parser.error("--panel needs two or more motifs, got {}".format(len(order)))
    if args.panel:
        print("\t".join(PANEL_HEADER))
    else:
        print("\t".join(HEADER + (["normalised_signal"] if args.sig_extract else [])
                        + (["search_from"] if args.after_stall or args.region is not None else [])))   # MotifSeq.py:160-163

    if not (args.f5f or args.f5_path or args.signal or args.blow5 or args.i16):
        sys.stderr.write("Unknown file or path input")
        parser.print_help(sys.stderr)
        sys.exit(1)
    if not order:                                    # nothing to search for: header only
        return

    _lib.warm_start(args.device)                    # HIP start-up runs beside the parsing of the first chunk
    if args.gpus > 1:
        api.set_devices(range(args.gpus))
    out = _Batcher(args, models, order, lens)
    if args.signal:
        # native tokenizer (csrc/sk_tsv.cpp): integer lines arrive as int16 rows, one GPU batch per chunk of the
        # file; decimal (pA) chunks go through the float64 tokenizer, odd lines through the reference's own parse
        for blk in tsvio.iter_tsv_blocks(args.signal, 8):
            if isinstance(blk, tsvio.FloatBlock):        # (first line decimal: straight from the float64 tokenizer)
                fb = blk
            else:
                if blk.mostly_integer():
                    out.block(blk)
                    continue
                fb = blk.float_block(8)
                if fb is None:
                    continue
            if fb.clean() and not (args.sig_extract or args.after_stall or out.per_line or out.queued):
                out.rows_f64(fb)                         # the whole chunk as one batch, no Python per read
                continue
            out.flush()
            for fast5, read_id, vals, fl, raw in tsvio.float_block_lines(fb):
                if fl & 8 or (fl & 16 and raw is not None and raw.count(b"\t") < 1):
                    # odd tokens (or not even a readID column): the reference's own parse, exceptions included
                    fast5, read_id, sig = tsvio.parse_motifseq_line(raw.decode())
                else:
                    sig = vals
                if not sig.any():
                    out.note(NO_SIGNAL)
                    continue
                out.add(fast5, read_id, sig)
            out.flush()
    elif args.blow5:
        # [extension] BLOW5: records decoded natively into int16 rows (raw ADC values, as the fast5 branches use)
        fast5 = os.path.basename(args.blow5).encode()
        seen = 0
        try:
            for blk in fastio.iter_blow5_blocks_i16(args.blow5, keep=_KEEP):
                bad = np.flatnonzero(blk.flags & 2)
                for i in bad:
                    sys.stderr.write("MotifSeq: unreadable BLOW5 record {} in {}; skipped\n".format(seen + int(i), args.blow5))
                seen += blk.n
                if bad.size:
                    ok = np.flatnonzero((blk.flags & 2) == 0)
                    blk = fastio.Blow5Block(blk.rows[ok], blk.nsamp[ok], blk.ids[ok], blk.calib[ok], blk.flags[ok])
                w = blk.ids.dtype.itemsize
                st = np.arange(blk.n, dtype=np.int64) * w
                spans = np.stack([st, st + np.char.str_len(blk.ids)], axis=1)
                out.rows(blk.rows, blk.nsamp, ("const", fast5), ("span", blk.ids, spans),
                         lambda i: fast5.decode(), lambda i, b=blk: b.ids[i].decode())
        except ValueError as e:                          # truncated file, unsupported compression: say so, no traceback
            out.drain()
            out.flush()
            sys.stdout.flush()
            sys.stderr.write("MotifSeq: --blow5: {}\n".format(e))
            sys.exit(1)
    elif args.i16:
        # [extension] packed reads: int16 [reads, samples] in a .npy file, memory mapped
        fast5 = os.path.basename(args.i16).encode()
        try:
            blocks = fastio.iter_npy_blocks_i16(args.i16, keep=_KEEP)
            for lo, part in blocks:
                ns = np.full(part.shape[0], part.shape[1], dtype=np.int32)
                out.rows(part, ns, ("const", fast5), ("i32", np.arange(lo, lo + part.shape[0], dtype=np.int32)),
                         lambda i: fast5.decode(), lambda i, lo=lo: str(lo + i))
        except ValueError as e:
            sys.stderr.write("MotifSeq: --i16: {}\n".format(e))
            sys.exit(1)
    else:
        if args.f5f:                                 # MotifSeq.py:165-184: first column = path
            with tsvio.open_text(args.f5f) as fh:
                files = [ln.strip("\n").split("\t")[0] for ln in fh]
        else:
            files = [os.path.join(d, f) for d, _, fs in os.walk(args.f5_path) for f in fs if f.endswith(".fast5")]
        for path in files:
            fast5 = path.split("/")[-1]
            sig, read_id = tsvio.motifseq_process_fast5(path, sys.stderr)          # MotifSeq.py:180,211,327-350
            if not len(sig):
                if args.f5f:
                    out.note("Failed to extract signal: {} {}\n".format(path, fast5))              # MotifSeq.py:182
                else:
                    out.note("main():data not extracted. Moving to next file - {}\n".format(path))  # MotifSeq.py:213
                continue
            out.add(fast5, read_id, np.array(sig, dtype=int))
    out.close()
    _mark("end of main()")
    _STATS[0].finish(args, [args.signal, getattr(args, "blow5", None), getattr(args, "i16", None)] + list(getattr(args, "ind", None) or []))


if __name__ == "__main__":
    main()
