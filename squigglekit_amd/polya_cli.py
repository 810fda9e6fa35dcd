"""dRNA_polya: where the adapter and the poly(A) tail of a direct-RNA read lie, by Viterbi through a six-state signal HMM.

    dRNA_polya.py -f reads.blow5 | -s signals.tsv | --i16 FILE.npy  [--preset rna_pa|synth_raw] [--limit N] [--rate]

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
sent to the device."""
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
    return p


def _fmt(v):
    return "." if v < 0 else str(int(v))


def polya_lines(names, records, rates=None):
    """the output lines of a batch; rates: per read samples_per_event (float, <= 0 or NaN: none) when --rate is on"""
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
        out.append("\t".join(cols) + "\n")
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
    def __init__(self, args, tool_input):
        self.model = api.polya_model(args.preset)
        self.pa = args.preset in PA_PRESETS
        self.limit, self.rate, self.batch, self.input = max(0, args.limit), args.rate, max(1, args.batch), tool_input
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
        if reads and self.cal:                           # BLOW5 rows under a pA preset
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
        sys.stdout.write("".join(polya_lines(self.names, rec, rates)))
        self.names, self.reads, self.cal = [], [], []


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

    from . import _lib
    _lib.warm_start(args.device, also=())
    out = _Batcher(args, args.signal or args.blow5 or args.i16)
    try:
        if args.signal:
            for rid, sig in iter_tsv_reads(args.signal):
                out.add(rid, sig)
        elif args.blow5:
            from .blow5 import read_slow5
            for rec in read_slow5(args.blow5):
                cal = None
                if out.pa:                               # sk_pa_calib's pair: range cut to two decimals first
                    cal = (float(rec["offset"]), float("{0:.2f}".format(rec["range"])) / float(rec["digitisation"]))
                out.add(rec["read_id"], rec["signal"], cal)
        else:
            a = np.load(args.i16, mmap_mode="r")
            if a.ndim != 2 or a.dtype != np.int16:
                raise ValueError("need a 2-D int16 array, got {} {}".format(a.dtype, a.shape))
            for lo in range(0, a.shape[0], out.batch):
                for i, row in enumerate(np.asarray(a[lo:lo + out.batch])):
                    out.add(str(lo + i), row)
        out.flush()
    except (ValueError, EOFError, OSError) as e:
        sys.stdout.flush()
        sys.stderr.write("dRNA_polya: {}: {}\n".format(args.signal or args.blow5 or args.i16, e))
        sys.exit(2)
    sys.stdout.flush()


if __name__ == "__main__":
    main()
