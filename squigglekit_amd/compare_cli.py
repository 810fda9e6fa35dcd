"""squiggle_compare: two pile-up tables of the same targets, point by point.  Host only: no GPU is touched.

    squiggle_compare.py A.tsv B.tsv [--min_depth N]

A.tsv / B.tsv: tables written by squiggle_map.py --pileup from two samples mapped to the same reference.  They must hold
the same points: a table whose (target, strand, pos) columns differ from the other's is refused.

Output: a header line, then one line per point (tab separated, floats as Python's "{}" writes them, `.` for a value that
does not exist):
    target strand pos depth_a depth_b level_a level_b diff t df d
diff = level_a - level_b; t: Welch's t with the unbiased variances sd^2 * n / (n - 1), n the table's `events`; df: the
Welch-Satterthwaite degrees of freedom; d = diff / sqrt((sd_a^2 + sd_b^2) / 2) (api.pileup_compare states the formulas).
t, df and d are `.` where either sample has fewer than --min_depth events at the point (default 2, and at least 2) or both
variances are zero.  There is no p-value: a normal approximation would mislead at low depth."""
import argparse
import sys

import numpy as np

from .map_cli import PILEUP_HEADER

HEADER = ("target", "strand", "pos", "depth_a", "depth_b", "level_a", "level_b", "diff", "t", "df", "d")


class _Parser(argparse.ArgumentParser):
    def error(self, message):
        sys.stderr.write("error: %s\n" % message)
        self.print_help()
        sys.exit(2)


def build_parser():
    p = _Parser(description="squiggle_compare - compare two squiggle_map --pileup tables point by point (host only)")
    p.add_argument("a", metavar="A.tsv", help="pile-up table of the first sample")
    p.add_argument("b", metavar="B.tsv", help="pile-up table of the second sample, over the same targets")
    p.add_argument("--min_depth", type=int, default=2, help="events a point needs in both samples to be tested (default 2, at least 2)")
    return p


def read_pileup(path):
    """(keys [(target, strand, pos)], pile PILE_DTYPE) of a --pileup table; ValueError for anything else"""
    from .api import PILE_DTYPE
    keys, rows = [], []
    with open(path) as fh:
        head = fh.readline().rstrip("\n").split("\t")
        if tuple(head) != PILEUP_HEADER:
            raise ValueError("not a pile-up table (header)")
        for no, ln in enumerate(fh, 2):
            f = ln.rstrip("\n").split("\t")
            if len(f) != len(PILEUP_HEADER):
                raise ValueError("line {}: {} fields".format(no, len(f)))
            keys.append((f[0], f[1], f[2]))
            try:
                stats = [float("nan") if x == "." else float(x) for x in f[7:13]]
                rows.append(tuple(stats) + (int(f[4]), int(f[5]), int(f[6]), 0))
            except ValueError:
                raise ValueError("line {}: not a number".format(no))
    return keys, np.array(rows, dtype=PILE_DTYPE) if rows else np.zeros(0, dtype=PILE_DTYPE)


def compare_lines(keys, cmp):
    def num(x):
        return "." if x != x else "{}".format(float(x))
    return ["\t".join(list(k) + [str(int(r["depth_a"])), str(int(r["depth_b"]))] +
                      [num(r[c]) for c in ("level_a", "level_b", "diff", "t", "df", "d")]) + "\n" for k, r in zip(keys, cmp)]


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(sys.argv[1:] if argv is None else argv)
    if args.min_depth < 2:
        parser.error("--min_depth must be at least 2")
    tables = []
    for path in (args.a, args.b):
        try:
            tables.append(read_pileup(path))
        except (OSError, ValueError) as e:
            sys.stderr.write("squiggle_compare: {}: {}\n".format(path, e))
            sys.exit(2)
    (ka, pa), (kb, pb) = tables
    if ka != kb:
        at = next((i for i, (x, y) in enumerate(zip(ka, kb)) if x != y), min(len(ka), len(kb)))
        sys.stderr.write("squiggle_compare: the tables do not hold the same points: {} has {} and {} has {}, first "
                         "difference at point line {}\n".format(args.a, len(ka), args.b, len(kb), at + 2))
        sys.exit(2)
    from .api import pileup_compare
    sys.stdout.write("\t".join(HEADER) + "\n")
    sys.stdout.write("".join(compare_lines(ka, pileup_compare(pa, pb, args.min_depth))))


if __name__ == "__main__":
    main()
