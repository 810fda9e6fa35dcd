"""detect_events: cut raw reads into events on the GPU and print one line per event.

    detect_events.py -s signals.tsv | --blow5 FILE | --i16 FILE.npy  [--rna] [--w_short N] ... [--pa]

Output: the header line `fast5 readID event start length mean stdv` (tab separated), then one line per event, floats as
Python's "{}" writes them.  mean = sum / length and stdv = sqrt(max(length * sumsq - sum^2, 0)) / length come from the
record's exact integers (api.event_levels / api.event_stdv); with --pa (BLOW5 input: it carries the calibration) both
are in pA.  The detector itself always runs on the raw samples -- its statistic does not change under the calibration.
A TSV holds raw integer samples from column 4 on, as segmenter.py reads it (name = column 0, read id = column 1); a TSV
of decimal (pA) values is refused with exit status 2.  A read without samples prints nothing on stdout and one note on
stderr."""
import argparse
import sys

import numpy as np

from . import api

HEADER = ("fast5", "readID", "event", "start", "length", "mean", "stdv")
START_COL = 4                                            # segmenter.py's rule: data = columns 4 ..


class _Parser(argparse.ArgumentParser):
    def error(self, message):
        sys.stderr.write("error: %s\n" % message)
        self.print_help()
        sys.exit(2)


def build_parser():
    p = _Parser(description="detect_events (MI355X) - cut raw reads into events wherever the current steps")
    src = p.add_mutually_exclusive_group()
    src.add_argument("-s", "--signal", help="signal TSV of raw integer samples written by SquigglePull -r (.gz accepted)")
    src.add_argument("--blow5", help="BLOW5 file (uncompressed or zlib records)")
    src.add_argument("--i16", help="packed reads: a .npy file holding an int16 array [reads, samples] (read name = row index)")
    p.add_argument("--rna", action="store_true", help="the rna preset (7, 14, 2.5, 9.0, 1.0) instead of dna (3, 6, 1.4, 9.0, 0.2)")
    p.add_argument("--w_short", type=int, default=None, help="short window")
    p.add_argument("--w_long", type=int, default=None, help="long window (at most 64)")
    p.add_argument("--th_short", type=float, default=None, help="short threshold")
    p.add_argument("--th_long", type=float, default=None, help="long threshold")
    p.add_argument("--peak_height", type=float, default=None, help="peak height")
    p.add_argument("--pa", action="store_true", help="print mean and stdv in pA (needs --blow5)")
    p.add_argument("--device", type=int, default=None, help="GPU index (default $SK_DEVICE or 0)")
    p.add_argument("--batch", type=int, default=4096, help="reads per GPU call")
    return p


def params_of(args):
    """the sk_det_params of the flags; ValueError names what is wrong with them"""
    over = {k: getattr(args, k) for k in ("w_short", "w_long", "th_short", "th_long", "peak_height")
            if getattr(args, k) is not None}
    p = api.det_params("rna" if args.rna else "dna", **over)
    if not 1 <= p.w_short <= p.w_long <= 64:
        raise ValueError("windows must satisfy 1 <= w_short <= w_long <= 64 (got %d, %d)" % (p.w_short, p.w_long))
    if not (np.isfinite(p.th_short) and np.isfinite(p.th_long)):
        raise ValueError("the thresholds must be finite")
    if not (np.isfinite(p.peak_height) and p.peak_height >= 0):
        raise ValueError("peak_height must be finite and >= 0")
    return p


def event_lines(names, off, rec, calib=None):
    """the output lines of a batch: names[r] = (fast5, readID)"""
    mean, _ = api.event_levels(off, rec, calib)
    sd = api.event_stdv(rec)
    if calib is not None:                                # the calibration is affine: a deviation scales by the raw unit
        calib = np.asarray(calib, dtype=np.float64).reshape(-1, 3)
        unit = np.array([float("{0:.2f}".format(rng)) / dig for dig, _, rng in calib], dtype=np.float64)
        sd = sd * np.repeat(unit, np.diff(off))
    out = []
    for r, (f5, rid) in enumerate(names):
        for k in range(int(off[r]), int(off[r + 1])):
            out.append("{}\t{}\t{}\t{}\t{}\t{}\t{}\n".format(f5, rid, k - int(off[r]), int(rec["start"][k]), int(rec["length"][k]),
                                                           float(mean[k]), float(sd[k])))
    return out


class _Batcher:
    def __init__(self, params, batch, tool_input):
        self.params, self.batch, self.input = params, max(1, batch), tool_input
        self.names, self.reads, self.calib = [], [], []

    def add(self, f5, rid, sig, calib=None):
        if len(sig) == 0:
            sys.stderr.write("detect_events: no samples in read {} of {}\n".format(rid, self.input))
            return
        self.names.append((f5, rid))
        self.reads.append(sig)
        if calib is not None:
            self.calib.append(calib)
        if len(self.reads) >= self.batch:
            self.flush()

    def flush(self):
        if not self.reads:
            return
        off, rec = api.detect_events(self.reads, self.params)
        sys.stdout.write("".join(event_lines(self.names, off, rec, self.calib or None)))
        self.names, self.reads, self.calib = [], [], []


def iter_tsv_reads(path):
    """(fast5, readID, int16 samples) per line of a raw TSV; ValueError for a line of decimal values"""
    from .tsvio import open_text
    with open_text(path) as fh:
        for ln, line in enumerate(fh, 1):
            cols = line.strip("\n").split("\t")
            if len(cols) < 2 or not line.strip():
                continue
            data = [c for c in cols[START_COL:] if c != ""]
            if data and any(ch in data[0] for ch in ".eE"):
                raise ValueError("line {}: decimal values -- event detection takes raw integer samples (write the TSV "
                                 "with SquigglePull -r, or give the BLOW5 file and --pa)".format(ln))
            try:
                sig = np.array([int(v) for v in data], dtype=np.int64)
            except ValueError:
                raise ValueError("line {}: not a line of integer samples".format(ln)) from None
            b = api.as_int16_exact(sig)
            if b is None:
                raise ValueError("line {}: a sample does not fit int16".format(ln))
            yield cols[0], cols[1], b


def main(argv=None):
    parser = build_parser()
    argv = sys.argv[1:] if argv is None else argv
    args = parser.parse_args(argv)
    if len(argv) == 0:
        parser.print_help(sys.stderr)
        sys.exit(1)
    if not (args.signal or args.blow5 or args.i16):
        parser.error("one of -s/--signal, --blow5, --i16 is needed")
    if args.pa and not args.blow5:
        parser.error("--pa needs --blow5 (the calibration comes from its records)")
    try:
        params = params_of(args)
    except ValueError as e:
        parser.error(str(e))

    from . import _lib
    _lib.warm_start(args.device, also=())
    out = _Batcher(params, args.batch, args.signal or args.blow5 or args.i16)
    sys.stdout.write("\t".join(HEADER) + "\n")
    try:
        if args.signal:
            for f5, rid, sig in iter_tsv_reads(args.signal):
                out.add(f5, rid, sig)
        elif args.blow5:
            from .blow5 import read_slow5
            for rec in read_slow5(args.blow5):
                out.add(args.blow5, rec["read_id"], rec["signal"],
                        (rec["digitisation"], rec["offset"], rec["range"]) if args.pa else None)
        else:
            a = np.load(args.i16, mmap_mode="r")
            if a.ndim != 2 or a.dtype != np.int16:
                raise ValueError("need a 2-D int16 array, got {} {}".format(a.dtype, a.shape))
            for lo in range(0, a.shape[0], out.batch):
                for i, row in enumerate(np.asarray(a[lo:lo + out.batch])):
                    out.add(args.i16, str(lo + i), row)
        out.flush()
    except (ValueError, EOFError, OSError) as e:
        sys.stdout.flush()
        sys.stderr.write("detect_events: {}: {}\n".format(args.signal or args.blow5 or args.i16, e))
        sys.exit(2)
    sys.stdout.flush()


if __name__ == "__main__":
    main()
