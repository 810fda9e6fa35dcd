"""dRNA_polya: where the adapter and the poly(A) tail of a direct-RNA read lie, by Viterbi through a six-state signal HMM.

    dRNA_polya.py -f reads.blow5 | -s signals.tsv | --i16 FILE.npy  [--preset rna_pa|synth_raw] [--limit N] [--rate]
                  [--model FILE.json] [--segments FILE] [--polya_net]
                  [--refit N --states ADAPTER,POLYA [--em] [--model_out FILE.json] [--fit_only]]
                  [--posterior] [--interval Q]

Output, tab separated, one line per read and no header:
    readID adapter_start adapter_end polya_start polya_end polya_samples score_per_sample
Coordinates are sample indices of the read as given, both ends included (api.polya_segments); a read in which no tail was
found (the best path does not end in TRANSCRIPT) has `.` in every coordinate column and 0 samples.  score_per_sample is
the best path's log score over the samples used, as Python's "{}" writes a float.
--rate appends samples_per_event and polya_events = polya_samples / samples_per_event: samples_per_event is the median
length of the read's events (event detection, rna preset) that start at or after the first TRANSCRIPT sample -- how
many samples one step of the motor takes in this read's own body.  The unit of polya_events is events, not nucleotides:
an event is what the detector cuts, and no calibration to bases is made here.  `.` `.` when there is no tail or no event.
The model sees pA for a BLOW5 file under a pA preset (the record's calibration: (raw + offset) * range / digitisation,
not rounded) and the values as they stand otherwise -- a TSV or a .npy carries no calibration, so the preset has to match
the file's units.  --rate needs raw integer samples (BLOW5, --i16, or a TSV of integers).
A read without samples still has its line -- `.` in every column but the 0 samples -- and one note on stderr; it is not
sent to the device.

The best path itself (api.hmm_segments*; these flags take the state-path route, the others the record-only one):
--model FILE.json   a model description (api.hmm_spec_to_json) in place of the preset's numbers; --preset still says which
                    units the model is in (a pA preset: BLOW5 records are calibrated).
--segments FILE     one line per segment of every read's best path, tab separated:
                        readID index state start end samples mean stdv
                    index counts a read's segments from 0, state is the name from api.POLYA_STATES (the index under
                    --model), start and end are sample indices, both included, mean and stdv (ddof 0) are in the model's
                    units, written as Python's "{}" writes a float.
--polya_net         appends polya_net: the tail's samples without its CLIFF segments (0 when no tail was found).
--refit N --states A,B   Viterbi training before the output: the input is streamed N times, the paths of every batch are
                    pooled, and after each pass the mean and sigma of the Gaussian components of the named states (names
                    or indices) are re-estimated (api.hmm_fit, api.hmm_refit).  --model_out FILE.json gets the fitted
                    description; the usual lines follow under the fitted model unless --fit_only is given.
                    --em trains by Baum-Welch instead (api.hmm_fit_em): soft counts from the posteriors in place of the
                    hard counts of the paths.

How much probability stands behind the coordinates (api.hmm_posterior*; forward-backward over the same model, which must
have the six states of a preset):
--posterior         appends loglik_per_sample (the read's log-likelihood over the samples used), polya_expected (the
                    expected number of samples in POLYA) and p_transcript (the probability that the last sample used is
                    in TRANSCRIPT); `.` `.` `.` for a read without samples or one the model gives probability 0.
--interval Q        appends polya_start_lo polya_start_hi transcript_start_lo transcript_start_hi, from the posterior of
                    every sample: the first sample at which P(state in POLYA, CLIFF, TRANSCRIPT) exceeds Q and 1 - Q, and
                    the same for P(state is TRANSCRIPT) -- the tail starts inside the first pair and ends just before the
                    second (api.hmm_boundary_interval); `.` where the probability never gets there.
Without these flags the output is what it was."""
import argparse
import sys

import numpy as np

from . import api

PA_PRESETS = ("rna_pa",)                                 # presets whose numbers are pA


class _Parser(argparse.ArgumentParser):
    def error(self, message):
        sys.stderr.write("error: %s\n" % message)
        self.print_help()
        sys.exit(2)


def build_parser():
    p = _Parser(description="dRNA_polya (MI355X) - adapter and poly(A) coordinates of direct-RNA reads by a signal HMM")
    src = p.add_mutually_exclusive_group()
    src.add_argument("-f", "--blow5", help="BLOW5 file (uncompressed or zlib records)")
    src.add_argument("-s", "--signal", help="signal TSV written by SquigglePull: pA values, or raw integers with -r (.gz accepted)")
    src.add_argument("--i16", help="packed reads: a .npy file holding an int16 array [reads, samples] (read name = row index)")
    p.add_argument("--preset", default="rna_pa", choices=sorted(api.POLYA_PRESETS), help="model preset (default rna_pa)")
    p.add_argument("--limit", type=int, default=0, help="use only the first N samples of a read (0: all)")
    p.add_argument("--rate", action="store_true", help="append samples_per_event and polya_events (unit: events)")
    p.add_argument("--device", type=int, default=None, help="GPU index (default $SK_DEVICE or 0)")
    p.add_argument("--batch", type=int, default=4096, help="reads per GPU call")
    p.add_argument("--model", help="model description (JSON, api.hmm_spec_to_json) in place of the preset's numbers")
    p.add_argument("--segments", metavar="FILE", help="write one line per segment: readID index state start end samples mean stdv")
    p.add_argument("--polya_net", action="store_true", help="append polya_net: the tail's samples without its CLIFF segments")
    p.add_argument("--refit", type=int, default=0, metavar="N", help="N passes of Viterbi training over the input first")
    p.add_argument("--states", default="", help="--refit: the states to re-estimate, names or indices, comma separated")
    p.add_argument("--model_out", metavar="FILE.json", help="--refit: write the fitted model description here")
    p.add_argument("--fit_only", action="store_true", help="--refit: stop after the model is written")
    p.add_argument("--em", action="store_true", help="--refit: Baum-Welch (soft counts from the posteriors) instead of Viterbi training")
    p.add_argument("--posterior", action="store_true", help="append loglik_per_sample, polya_expected and p_transcript")
    p.add_argument("--interval", type=float, default=None, metavar="Q",
                   help="append the samples at which the tail's start and the transcript's start pass probability Q and 1 - Q")
    return p


def _fmt(v):
    return "." if v < 0 else str(int(v))


def polya_lines(names, records, rates=None, net=None, extra=None):
    """the output lines of a batch; rates: per read samples_per_event (float, <= 0 or NaN: none) when --rate is on;
    net: per read polya_net when --polya_net is on; extra: per read the --posterior / --interval columns"""
    seg = api.polya_segments(records)
    out = []
    for r, rid in enumerate(names):
        s = seg[r]
        n = int(records["n_used"][r])
        cols = [str(rid), _fmt(s["adapter_start"]), _fmt(s["adapter_end"]), _fmt(s["polya_start"]), _fmt(s["polya_end"]),
                str(int(s["polya_samples"])), "{}".format(float(records["score"][r]) / n) if n > 0 else "."]
        if rates is not None:
            spe = float(rates[r])
            if s["found"] and spe > 0:
                cols += ["{}".format(spe), "{}".format(float(s["polya_samples"]) / spe)]
            else:
                cols += [".", "."]
        if net is not None:
            cols.append(str(int(net[r])))
        if extra is not None:
            cols += extra[r]
        out.append("\t".join(cols) + "\n")
    return out


def posterior_columns(post, gammas, posterior, interval):
    """per read the --posterior columns (post: HMM_POST_DTYPE) and the --interval Q columns (gammas: per read [n, 6])"""
    out = []
    for r in range(len(post)):
        cols = []
        ok = int(post["n_used"][r]) > 0 and int(post["flags"][r]) == 0
        if posterior:
            cols += (["{}".format(float(post["loglik"][r]) / int(post["n_used"][r])),
                      "{}".format(float(post["occ"][r][api.POLYA])),
                      "{}".format(float(post["final_post"][r][api.TRANSCRIPT]))] if ok else [".", ".", "."])
        if interval is not None:
            iv = (-1, -1, -1, -1)
            if ok:
                iv = (api.hmm_boundary_interval(gammas[r], (api.POLYA, api.CLIFF, api.TRANSCRIPT), interval, 1.0 - interval) +
                      api.hmm_boundary_interval(gammas[r], (api.TRANSCRIPT,), interval, 1.0 - interval))
            cols += [_fmt(v) for v in iv]
        out.append(cols)
    return out


def polya_net(records, off, seg):
    """per read: the samples of the POLYA segments between polya_start and polya_end (0: no tail found)"""
    ps = api.polya_segments(records)
    out = np.zeros(len(ps), dtype=np.int64)
    for r in np.flatnonzero(ps["found"]):
        g = seg[int(off[r]):int(off[r + 1])]
        inside = (g["state"] == api.POLYA) & (g["start"] >= ps["polya_start"][r]) & (g["start"] <= ps["polya_end"][r])
        out[r] = int(g["length"][inside].sum())
    return out


def segment_lines(names, off, seg, state_names=None, cal=None):
    """the --segments lines of a batch: readID index state start end samples mean stdv; cal: per read (offset, unit) or None"""
    per = np.diff(np.asarray(off, dtype=np.int64))
    mean, stdv = api.hmm_segment_levels(seg, None if cal is None else np.repeat(np.asarray(cal, dtype=np.float64).reshape(-1, 2),
                                                                                per, axis=0))
    out = []
    for r, rid in enumerate(names):
        for i, k in enumerate(range(int(off[r]), int(off[r + 1]))):
            e = seg[k]
            st = int(e["state"])
            out.append("\t".join([str(rid), str(i), state_names[st] if state_names else str(st), str(int(e["start"])),
                                  str(int(e["start"]) + int(e["length"]) - 1), str(int(e["length"])),
                                  "{}".format(float(mean[k])), "{}".format(float(stdv[k]))]) + "\n")
    return out


def samples_per_event(records, off, ev):
    """per read: the median length of its events that start at or after enter[TRANSCRIPT] (NaN: no tail or no such event)"""
    records = np.asarray(records)
    out = np.full(records.shape[0], np.nan)
    for r in range(records.shape[0]):
        t0 = int(records["enter"][r][api.TRANSCRIPT])
        if t0 < 0:
            continue
        e = ev[int(off[r]):int(off[r + 1])]
        ln = e["length"][e["start"] >= t0]
        if ln.size:
            out[r] = float(np.median(ln))
    return out


class _Batcher:
    def __init__(self, args, tool_input, spec=None, seg_out=None):
        self.model = api.polya_model(args.preset) if spec is None else api.hmm_model(*spec)
        self.pa = args.preset in PA_PRESETS
        self.paths = bool(seg_out is not None or args.polya_net)      # the state-path route (api.hmm_segments*)
        self.seg_out, self.net = seg_out, args.polya_net
        self.state_names = api.POLYA_STATES if not args.model else None
        self.limit, self.rate, self.batch, self.input = max(0, args.limit), args.rate, max(1, args.batch), tool_input
        self.posterior, self.interval = args.posterior, args.interval
        if (self.posterior or self.interval is not None) and self.model.nstates != 6:
            raise ValueError("--posterior and --interval need a model of the six states " + ", ".join(api.POLYA_STATES))
        self.names, self.reads, self.cal = [], [], []

    def add(self, rid, sig, cal=None):
        if len(sig) == 0:
            sys.stderr.write("dRNA_polya: no samples in read {} of {}\n".format(rid, self.input))
        self.names.append(rid)
        self.reads.append(sig)
        if cal is not None:
            self.cal.append(cal)
        if len(self.reads) >= self.batch:
            self.flush()

    def flush(self):
        if not self.reads:
            return
        keep = [i for i, r in enumerate(self.reads) if len(r) > 0]
        reads = [self.reads[i] for i in keep]
        rec = np.zeros(len(self.reads), dtype=api.HMM_DTYPE)             # the record of a read without samples ...
        rec["final_state"], rec["enter"] = -1, -1
        rates = np.full(len(self.reads), np.nan) if self.rate else None
        net = None
        if reads and self.paths:
            net = self.flush_paths(keep, reads, rec)
        elif self.paths:
            net = np.zeros(len(self.reads), dtype=np.int64)
        elif reads and self.cal:                         # BLOW5 rows under a pA preset
            buf, lens = api.pack_i16(reads)
            cal = np.array([self.cal[i] for i in keep], dtype=np.float64)
            rec[keep] = api.hmm_viterbi_batch(buf, lens, self.model, cal, self.limit)
        elif reads:
            rec[keep] = api.hmm_viterbi(reads, self.model, self.limit)
        if reads and self.rate:
            try:
                off, ev = api.detect_events(reads, api.det_params("rna"))
            except ValueError:
                raise ValueError("--rate needs raw integer samples (event detection runs on them)") from None
            rates[keep] = samples_per_event(rec[keep], off, ev)
        extra = None
        if self.posterior or self.interval is not None:
            extra = self.flush_posterior(keep, reads)
        sys.stdout.write("".join(polya_lines(self.names, rec, rates, net if self.net else None, extra)))
        self.names, self.reads, self.cal = [], [], []

    def flush_posterior(self, keep, reads):
        """the --posterior / --interval columns of every read of the batch (a read without samples: `.` throughout)"""
        dense = self.interval is not None
        post = np.zeros(len(self.reads), dtype=api.HMM_POST_DTYPE)
        gammas = [None] * len(self.reads)
        if reads and self.cal:                           # BLOW5 rows under a pA preset
            buf, lens = api.pack_i16(reads)
            cal = np.array([self.cal[i] for i in keep], dtype=np.float64)
            p, _c, goff, gamma = api.hmm_posterior_batch(buf, lens, self.model, cal, self.limit, dense=dense)
            g = [gamma[int(goff[k]):int(goff[k + 1])] for k in range(len(reads))] if dense else None
        elif reads:
            p, _c, g = api.hmm_posterior(reads, self.model, self.limit, dense=dense)
        if reads:
            post[keep] = p
            if dense:
                for k, i in enumerate(keep):
                    gammas[i] = g[k]
        return posterior_columns(post, gammas, self.posterior, self.interval)

    def flush_paths(self, keep, reads, rec):
        """the records of the reads with samples through the state-path route, their --segments lines, their polya_net"""
        names = [self.names[i] for i in keep]
        net = np.zeros(len(self.reads), dtype=np.int64)
        if self.cal:                                     # BLOW5 rows under a pA preset
            buf, lens = api.pack_i16(reads)
            cal = np.array([self.cal[i] for i in keep], dtype=np.float64)
            parts = [(list(range(len(reads))),) + api.hmm_segments_batch(buf, lens, self.model, cal, self.limit) + (cal,)]
        else:
            parts = [p + (None,) for p in api._segments_parts(reads, self.model, self.limit)]
        lines = {}
        for idx, prec, off, seg, cal in parts:
            rec[[keep[i] for i in idx]] = prec
            net[[keep[i] for i in idx]] = polya_net(prec, off, seg) if self.model.nstates == 6 else 0
            if self.seg_out is not None:
                for k, i in enumerate(idx):              # (input order: the two feeds of a mixed batch interleave)
                    lines[i] = segment_lines([names[i]], off[k:k + 2] - off[k], seg[int(off[k]):int(off[k + 1])],
                                             self.state_names, None if cal is None else cal[k:k + 1])
        if self.seg_out is not None:
            self.seg_out.write("".join("".join(lines[i]) for i in sorted(lines)))
        return net


def iter_tsv_reads(path):
    """(readID, samples) per line of a SquigglePull TSV: int16 where every value is a raw integer, float64 otherwise"""
    from .tsvio import open_text
    from .detect_cli import START_COL
    with open_text(path) as fh:
        for ln, line in enumerate(fh, 1):
            cols = line.strip("\n").split("\t")
            if len(cols) < 2 or not line.strip():
                continue
            try:
                sig = np.array([float(v) for v in cols[START_COL:] if v != ""], dtype=np.float64)
            except ValueError:
                raise ValueError("line {}: not a line of samples".format(ln)) from None
            if not np.all(np.isfinite(sig)):
                raise ValueError("line {}: a sample is not finite".format(ln))
            b = api.as_int16_exact(sig)
            yield cols[1], sig if b is None else b


def iter_input(args, pa, batch):
    """(readID, samples, calibration pair or None) of every read of the input file, in file order"""
    if args.signal:
        for rid, sig in iter_tsv_reads(args.signal):
            yield rid, sig, None
    elif args.blow5:
        from .blow5 import read_slow5
        for rec in read_slow5(args.blow5):
            cal = None
            if pa:                                       # sk_pa_calib's pair: range cut to two decimals first
                cal = (float(rec["offset"]), float("{0:.2f}".format(rec["range"])) / float(rec["digitisation"]))
            yield rec["read_id"], rec["signal"], cal
    else:
        a = np.load(args.i16, mmap_mode="r")
        if a.ndim != 2 or a.dtype != np.int16:
            raise ValueError("need a 2-D int16 array, got {} {}".format(a.dtype, a.shape))
        for lo in range(0, a.shape[0], batch):
            for i, row in enumerate(np.asarray(a[lo:lo + batch])):
                yield str(lo + i), row, None


def fit_batches(args, pa, batch):
    """the input file as hmm_fit takes it: lists of reads with samples, or (rows, lengths, calibration pairs) under a pA
    preset -- one pass over the file per call"""
    def emit(reads, cals):
        if cals:
            return api.pack_i16(reads) + (np.array(cals, dtype=np.float64),)
        return reads

    def one_pass():
        reads, cals = [], []
        for _rid, sig, cal in iter_input(args, pa, batch):
            if len(sig) == 0:
                continue
            reads.append(sig)
            if cal is not None:
                cals.append(cal)
            if len(reads) >= batch:
                yield emit(reads, cals)
                reads, cals = [], []
        if reads:
            yield emit(reads, cals)
    return one_pass


def parse_states(text, S, named):
    """--states: names of api.POLYA_STATES (a preset's model) or indices below S"""
    out = []
    for tok in [t.strip() for t in text.split(",") if t.strip()]:
        if named and tok.upper() in api.POLYA_STATES:
            out.append(api.POLYA_STATES.index(tok.upper()))
        elif tok.isdigit() and int(tok) < S:
            out.append(int(tok))
        else:
            raise ValueError("--states: no state {!r}".format(tok))
    if not out:
        raise ValueError("--refit needs --states (the states whose emissions are re-estimated)")
    return out


def main(argv=None):
    parser = build_parser()
    argv = sys.argv[1:] if argv is None else argv
    args = parser.parse_args(argv)
    if len(argv) == 0:
        parser.print_help(sys.stderr)
        sys.exit(1)
    if not (args.signal or args.blow5 or args.i16):
        parser.error("one of -f/--blow5, -s/--signal, --i16 is needed")
    if args.limit < 0:
        parser.error("--limit must be >= 0")
    if args.refit < 0:
        parser.error("--refit must be >= 0")
    if (args.model_out or args.fit_only or args.states or args.em) and not args.refit:
        parser.error("--states, --em, --model_out and --fit_only go with --refit N")
    if args.interval is not None and not 0.0 < args.interval < 0.5:
        parser.error("--interval Q needs 0 < Q < 0.5")

    from . import _lib
    _lib.warm_start(args.device, also=())
    tool_input = args.signal or args.blow5 or args.i16
    seg_out = None
    try:
        spec = None
        if args.model:
            with open(args.model) as fh:
                spec = api.hmm_spec_from_json(fh.read())
        if args.refit:
            spec = api.polya_spec(args.preset) if spec is None else spec
            states = parse_states(args.states, len(spec[0]), not args.model)
            fit = api.hmm_fit_em if args.em else api.hmm_fit
            spec, _history = fit(fit_batches(args, args.preset in PA_PRESETS, max(1, args.batch)), spec, states,
                                 args.refit, limit=max(0, args.limit))
            if args.model_out:
                with open(args.model_out, "w") as fh:
                    fh.write(api.hmm_spec_to_json(spec))
        if not (args.refit and args.fit_only):
            if args.segments:
                seg_out = open(args.segments, "w")
            out = _Batcher(args, tool_input, spec, seg_out)
            for rid, sig, cal in iter_input(args, out.pa, out.batch):
                out.add(rid, sig, cal)
            out.flush()
    except (ValueError, EOFError, OSError) as e:
        sys.stdout.flush()
        sys.stderr.write("dRNA_polya: {}: {}\n".format(tool_input, e))
        sys.exit(2)
    finally:
        if seg_out is not None:
            seg_out.close()
    sys.stdout.flush()


if __name__ == "__main__":
    main()
