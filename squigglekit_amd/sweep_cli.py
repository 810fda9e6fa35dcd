"""segmenter_sweep.py: segmenter.py's pipeline for a whole grid of parameter sets in one GPU pass per
(lim_low, lim_hi, std_scale) (api.segment_sweep), one table line per set.

The reads are exactly those segmenter.py hands get_segs -- same inputs, same skips, same [:Num] cut (segmenter_cli);
each of -e -c -w -d -t -l -lim_low -lim_hi -j -b takes a value, a comma list or a:b:s ranges, and --grid FILE adds a
TSV of sets.  The columns are the counts segmenter.py's runs would print: with_segs = lines without -u, stall_ok =
lines with -k -u, gap_ok = lines with -g -u, stall_gap_ok = lines with -k -g -u.
"""
import argparse
import os
import sys
import time
from decimal import Decimal, InvalidOperation

import numpy as np

from . import api, tsvio

FLAGS = (("-e", "--error"), ("-c", "--corrector"), ("-w", "--window"), ("-d", "--seg_dist"), ("-t", "--std_scale"),
         ("-l", "--stall_len"), ("-lim_low", "--lim_low"), ("-lim_hi", "--lim_hi"), ("-j", "--stall_start"),
         ("-b", "--gap_dist"))
COLUMNS = ("reads", "with_segs", "segs", "stall_ok", "gap_ok", "stall_gap_ok")


class _Parser(argparse.ArgumentParser):
    def error(self, message):                      # as segmenter_cli._Parser
        sys.stderr.write("error: %s\n" % message)
        self.print_help()
        sys.exit(2)


def build_parser():
    p = _Parser(description="segmenter parameter sweep (MI355X) - score a grid of segmenter settings in one GPU pass")
    src = p.add_mutually_exclusive_group()
    src.add_argument("-i", "--ind", nargs="+", help="one or more fast5 files")
    src.add_argument("-p", "--f5_path", help="directory searched recursively for fast5 files")
    src.add_argument("-s", "--signal", help="signal TSV written by SquigglePull (.gz accepted)")
    src.add_argument("--blow5", help="BLOW5 file (pA unless --raw_signal)")
    src.add_argument("--i16", help="packed reads: a .npy file holding an int16 array [reads, samples]")
    p.add_argument("--single", action="store_true", help="fast5 files hold one read each")
    p.add_argument("-n", "--Num", type=int, default=0, help="use only the first Num samples; 0 = whole read")
    p.add_argument("--raw_signal", action="store_true", help="fast5 / BLOW5 input: keep raw ADC values (no pA conversion)")
    for (short, long_), key in zip(FLAGS, api.SWEEP_KEYS):
        p.add_argument(short, long_, dest=key, default=str(api.SWEEP_DEFAULTS[key]), metavar="V",
                       help="value, comma list or a:b:s range (default %s)" % api.SWEEP_DEFAULTS[key])
    p.add_argument("--grid", default=None, metavar="FILE",
                   help="TSV of sets: a header naming some of the ten parameters, one set per line; the parameters it "
                        "does not name take the flag values")
    p.add_argument("--records", default=None, metavar="PATH.npy", help="also write the [sets, reads] records")
    p.add_argument("--names", default=None, metavar="PATH.txt", help="also write the read names in record order")
    p.add_argument("--device", type=int, default=None, help="GPU index (default $SK_DEVICE or 0)")
    p.add_argument("--gpus", type=int, default=1, help="shard the reads over this many GPUs of the node")
    p.add_argument("--stats", action="store_true", help="reads, sets and seconds as one line on stderr at the end")
    return p


def _number(text, key):
    d = Decimal(text.strip())
    if key in api._SWEEP_FLOAT:
        return float(d)
    if d != d.to_integral_value():
        raise ValueError("%s takes integers: %r" % (key, text))
    return int(d)


def parse_values(text, key):
    """A flag's values: comma-separated items, each a number or a:b:s (a, a+s, ... up to and including b, computed in
    decimal so that 0.5:1.0:0.1 gives the doubles of the literals).  Raises ValueError on anything else."""
    out = []
    for item in str(text).split(","):
        parts = item.split(":")
        try:
            if len(parts) == 1:
                out.append(_number(parts[0], key))
                continue
            if len(parts) != 3:
                raise ValueError("a range is a:b:s")
            a, b, s = (Decimal(x.strip()) for x in parts)
        except InvalidOperation:
            raise ValueError("-%s: malformed value %r" % (key, item)) from None
        if s == 0 or (b - a) * s < 0:
            raise ValueError("-%s: range %r never reaches its end" % (key, item))
        k, v = 0, a
        while (v <= b) if s > 0 else (v >= b):
            out.append(_number(str(v), key))
            k += 1
            v = a + k * s
    return out


def build_sets(args):
    """The grid of the flags, or -- with --grid -- each line of the file with the flags' grid over the rest."""
    values = {k: parse_values(getattr(args, k), k) for k in api.SWEEP_KEYS}
    if not args.grid:
        return api.sweep_grid(**values)
    sets = []
    with open(args.grid) as fh:
        rows = [ln.rstrip("\n").split("\t") for ln in fh if ln.strip()]
    if not rows:
        raise ValueError("--grid %s: no header" % args.grid)
    head = [h.strip() for h in rows[0]]
    bad = [h for h in head if h not in api.SWEEP_KEYS]
    if bad or len(set(head)) != len(head):
        raise ValueError("--grid %s: the header names unknown or repeated columns: %s" % (args.grid, bad or head))
    for n, row in enumerate(rows[1:], 2):
        if len(row) != len(head):
            raise ValueError("--grid %s: line %d has %d columns, the header %d" % (args.grid, n, len(row), len(head)))
        fixed = {}
        for h, v in zip(head, row):
            try:
                fixed[h] = _number(v, h)
            except (InvalidOperation, ValueError):
                raise ValueError("--grid %s: line %d: malformed %s %r" % (args.grid, n, h, v)) from None
        sets += api.sweep_grid(**dict(values, **fixed))
    return sets


def read_inputs(args):
    """(names, reads): what segmenter.py hands get_segs, in its order (segmenter_cli's readers and skips)."""
    Num = args.Num
    names, reads = [], []
    if args.signal:
        with tsvio.open_text(args.signal) as fh:
            for line in fh:
                name, sig = tsvio.parse_segmenter_line(line)         # segmenter.py:192-201
                if not sig.any():                                     # :203-205
                    continue
                names.append(name)
                reads.append(sig[:Num])
    elif args.blow5:
        from .blow5 import read_blow5, to_pA
        for rec in read_blow5(args.blow5):
            sig = rec["signal"].astype(int)
            if not args.raw_signal:
                sig = to_pA(sig, rec["digitisation"], rec["offset"], rec["range"])
            names.append(rec["read_id"])
            reads.append(sig[:Num])
    elif args.i16:
        rows = np.load(args.i16, mmap_mode="r")
        if rows.dtype != np.int16 or rows.ndim != 2:
            raise ValueError("--i16 %s: not an int16 [reads, samples] array" % args.i16)
        for i in range(rows.shape[0]):
            names.append(str(i))
            reads.append(np.asarray(rows[i, :Num]))
    else:
        if args.f5_path:
            files = [os.path.join(d, f) for d, _, fs in os.walk(args.f5_path) for f in fs if f.endswith(".fast5")]
        else:
            files = list(args.ind)
        for path in files:
            label = os.path.basename(path) if args.f5_path else path
            if args.single:
                sig = tsvio.segmenter_process_fast5(path, args.raw_signal, sys.stderr)
                if not np.asarray(sig).any():
                    continue
                names.append(label)
                reads.append(np.array(sig[:Num], dtype=float))
            else:
                for read, sig in tsvio.read_multi_fast5(path, args.raw_signal).items():
                    names.append(read)
                    reads.append(np.array(sig[:Num], dtype=float))
    return names, reads


def format_table(sets, sums):
    """The sweep table: a header, then per set its ten parameters and its counts."""
    lines = ["\t".join(api.SWEEP_KEYS + COLUMNS + ("seg0_end_mean",))]
    for s, m in zip(sets, sums):
        vals = [str(v) for v in api.sweep_values(s)] + [str(int(m[c])) for c in COLUMNS]
        w = int(m["with_segs"])
        vals.append("%.3f" % (int(m["seg0_end_sum"]) / w) if w else "nan")
        lines.append("\t".join(vals))
    return "\n".join(lines) + "\n"


def main(argv=None):
    parser = build_parser()
    argv = sys.argv[1:] if argv is None else argv
    args = parser.parse_args(argv)
    if not (args.f5_path or args.ind or args.signal or args.blow5 or args.i16):
        parser.error("no input: give one of -s, -p, -i, --blow5, --i16")
    if not args.Num:                                  # segmenter.py:104-105 (drops the last sample)
        args.Num = -1
    try:
        sets = build_sets(args)
    except (ValueError, OSError) as e:
        parser.error(str(e))
    if not sets:
        parser.error("empty grid")
    for k, s in enumerate(sets):
        if s.seg.corrector < 0:
            parser.error("set %d: corrector must be >= 0" % k)
    t0 = time.time()
    from . import _lib
    _lib.warm_start(args.device, also=())
    if args.gpus > 1:
        api.set_devices(range(args.gpus))
    names, reads = read_inputs(args)
    sums, recs = api.segment_sweep(reads, sets, records=args.records is not None)
    sys.stdout.write(format_table(sets, sums))
    sys.stdout.flush()
    if args.records:
        np.save(args.records, recs)
    if args.names:
        with open(args.names, "w") as fh:
            fh.write("".join(n + "\n" for n in names))
    if args.stats:
        sys.stderr.write("segmenter_sweep: %d reads x %d sets in %.3f s\n" % (len(reads), len(sets), time.time() - t0))


if __name__ == "__main__":
    main()
