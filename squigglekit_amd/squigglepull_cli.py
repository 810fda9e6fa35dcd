"""Drop-in for the reference's SquigglePull.py command line (SquigglePull.py:70-253).

Same flags, help text, stdout (one line per read: file name, read id, [-i columns,] samples), stderr strings and exit
codes.  The files are read the reference's way (os.walk order, its auto-detection rule, its try/except per read); the
part that costs time per sample -- the pA conversion and the text -- is made on the GPU (api.pull_text, csrc/sk_pull.hip)
for many reads per call, in input order.  Additive flag: --blow5 FILE (binary BLOW5, decoded natively; column 0 is the
file's base name), hidden from the help so that the help text stays the reference's.  There is no CPU path.
"""
import argparse
import os
import sys
import time
import traceback

import numpy as np

from . import api, fastio, tsvio

_KEEP = []       # input mappings / page-locked buffers of a finished reader: released with the process
BATCH_READS = 16384
BATCH_SAMPLES = 64 << 20


class MyParser(argparse.ArgumentParser):
    def error(self, message):                      # SquigglePull.py:70-74
        sys.stderr.write('error: %s\n' % message)
        self.print_help()
        sys.exit(2)


def build_parser():
    parser = MyParser(prog="SquigglePull.py",
                      description="SquigglePull - extraction and (optional) conversion to pA of raw signal from Oxford Nanopore fast5 files")
    parser.add_argument("-p", "--path",
                        help="Top directory path of fast5 files")
    parser.add_argument("-t", "--type", action="store", default="auto", choices=["auto", "single", "multi"], help="Specify the type of files provided. Default is autodetection which enables a mix of single and multifast5 files.")
    parser.add_argument("-v", "--verbose", action="store_true",
                        help="Engage higher output verbosity")
    parser.add_argument("-r", "--raw_signal", action="store_true",
                        help="No conversion to pA, raw signal is extracted instead")
    parser.add_argument("-i", "--extra_info", action="store_true",
                        help="Print extra information used for signal conversion and in methylation calling - nanopolish/f5c")
    parser.add_argument("--blow5", help=argparse.SUPPRESS)        # BLOW5 file instead of -p (not in the reference)
    return parser


def _prefix(fast5, d, extra_info):
    """Everything print_data prints before the first sample (SquigglePull.py:247-253), trailing tab included."""
    if extra_info:
        s = '{}\t{}\t{}\t{}\t{}\t{}\t'.format(fast5, d['readID'], d['digitisation'], d['offset'], d['range'],
                                               d['sampling_rate'])
    else:
        s = '{}\t{}\t'.format(fast5, d['readID'])
    return s.encode("utf-8", "surrogateescape")


class _Lines:
    """Reads waiting for one GPU call.  A batch holds one kind of line: pA, or str(int) -- the -r output, and what
    the reference prints for a multi-read entry whose conversion never ran."""

    def __init__(self):
        self.prefixes, self.sigs, self.cals, self.raw, self.samples = [], [], [], None, 0

    def add(self, prefix, sig, cal):
        raw = cal is None
        if self.sigs and raw != self.raw:
            self.flush()
        self.raw = raw
        self.prefixes.append(prefix)
        self.sigs.append(sig)
        self.cals.append(cal if cal is not None else (0.0, 0.0, 0.0))
        self.samples += len(sig)
        if len(self.sigs) >= BATCH_READS or self.samples >= BATCH_SAMPLES:
            self.flush()

    def flush(self):
        if not self.sigs:
            return
        lens = np.array([len(s) for s in self.sigs], dtype=np.int32)
        rows = np.zeros((len(self.sigs), max(1, int(lens.max()))), dtype=np.int16)
        for i, s in enumerate(self.sigs):
            rows[i, :len(s)] = s
        calib = None if self.raw else np.array(self.cals, dtype=np.float64)
        text = api.pull_text(rows, lens, self.prefixes, calib=calib, raw=self.raw)
        self.prefixes, self.sigs, self.cals, self.samples = [], [], [], 0
        fastio.write_stdout(text)


def _signal(ds):
    """The Signal dataset as int16 (the reference's `int(col)` loop, SquigglePull.py:178-179, 211-212)."""
    sig = api.as_int16_exact(ds[()])
    if sig is None:
        raise ValueError("Signal samples do not fit in int16")
    return sig


def _new_read():
    return {'raw': np.zeros(0, dtype=np.int16), 'cal': None, 'readID': '',
            'digitisation': 0.0, 'offset': 0.0, 'range': 0.0, 'sampling_rate': 0.0}


def extract_f5_all(filename, args):
    """SquigglePull.extract_f5_all (SquigglePull.py:130-236) up to the conversion, which is left to the GPU: d['cal']
    = (digitisation, offset, range) when the reference would convert the read, else None.  Exceptions the reference
    does not catch (opening the file, the auto-detection) propagate as they do there."""
    f5_dic = {}
    multi = False
    with tsvio.open_fast5(filename) as hdf:
        if args.type == "auto":
            reads = list(hdf.keys())
            if 'read' not in reads[1]:
                if args.verbose:
                    sys.stderr.write("{} detected as a single fast5 file\n".format(filename))
                multi = False
            else:
                if args.verbose:
                    sys.stderr.write("{} detected as a multi fast5 file\n".format(filename))
                multi = True
        elif args.type == "multi":
            reads = list(hdf.keys())
            multi = True

        if not multi:
            f5_dic = _new_read()
            try:
                c = list(hdf['Raw/Reads'].keys())
                f5_dic['raw'] = _signal(hdf['Raw/Reads/'][c[0]]['Signal'])
                f5_dic['readID'] = hdf['Raw/Reads/'][c[0]].attrs['read_id'].decode()
                digitisation = hdf['UniqueGlobalKey/channel_id'].attrs['digitisation']
                offset = hdf['UniqueGlobalKey/channel_id'].attrs['offset']
                range_ = float("{0:.2f}".format(hdf['UniqueGlobalKey/channel_id'].attrs['range']))
                if not args.raw_signal:
                    f5_dic['cal'] = (digitisation, offset, range_)
                if args.extra_info:
                    f5_dic['digitisation'] = digitisation
                    f5_dic['offset'] = offset
                    f5_dic['range'] = range_
                    f5_dic['sampling_rate'] = hdf['UniqueGlobalKey/channel_id'].attrs['sampling_rate']
            except Exception:
                traceback.print_exc()
                sys.stderr.write("extract_fast5_all():failed to extract raw signal or fastq from {}".format(filename))
                f5_dic = {}
        else:
            for read in reads:
                d = f5_dic[read] = _new_read()
                try:
                    d['raw'] = _signal(hdf[read]['Raw/Signal'])
                    d['readID'] = hdf[read]['Raw'].attrs['read_id'].decode()
                    digitisation = hdf[read]['channel_id'].attrs['digitisation']
                    offset = hdf[read]['channel_id'].attrs['offset']
                    range_ = float("{0:.2f}".format(hdf[read]['channel_id'].attrs['range']))
                    if not args.raw_signal:
                        d['cal'] = (digitisation, offset, range_)
                    if args.extra_info:
                        d['digitisation'] = digitisation
                        d['offset'] = offset
                        d['range'] = range_
                        d['sampling_rate'] = hdf[read]['channel_id'].attrs['sampling_rate']
                except Exception:
                    traceback.print_exc()
                    sys.stderr.write("extract_fast5_all():failed to read readID: {}".format(read))
    return f5_dic, multi


def _walk(args, out):
    for dirpath, dirnames, files in os.walk(args.path):
        for fast5 in files:
            if fast5.endswith('.fast5'):
                fast5_file = os.path.join(dirpath, fast5)
                data, multi = extract_f5_all(fast5_file, args)
                if not data:
                    sys.stderr.write("main():data not extracted from {}. Moving to next file.".format(fast5_file))
                    continue
                for d in ([data] if not multi else data.values()):
                    out.add(_prefix(fast5, d, args.extra_info), d['raw'], d['cal'])


def _write(text):
    """fastio.write_stdout for a memoryview as well (a captured stdout without a byte layer takes text)."""
    fastio.write_stdout(text if getattr(sys.stdout, "buffer", None) is not None else bytes(text))


def _blow5(args):
    """--blow5: records decoded natively into int16 rows (fastio.iter_blow5_blocks_i16, one block ahead on its own
    thread); block k's GPU call runs on a worker thread while block k - 1's text is written and block k + 1 decoded."""
    from concurrent.futures import ThreadPoolExecutor
    name = os.path.basename(args.blow5).encode("utf-8", "surrogateescape")
    rates = None
    if args.extra_info:                                  # (the native decoder does not return the sampling rate)
        from .blow5 import read_blow5
        rates = (rec["sampling_rate"] for rec in read_blow5(args.blow5))
    bufs = [None, None, None]

    def gpu(k, blk, prefixes):
        b = bufs[k % 3]
        need = int(sum(len(p) for p in prefixes)) + 8 * int(blk.nsamp.sum()) + blk.n + 1
        if b is None or b.nbytes < need:
            try:                                         # page-locked: the text comes back by DMA
                b = api.pinned_empty((need + need // 4,), np.uint8)
            except Exception:                            # noqa: BLE001 -- no pinned memory: ordinary pages
                b = np.empty(need + need // 4, dtype=np.uint8)
            bufs[k % 3] = b
        return api.pull_text(blk.rows, blk.nsamp, prefixes, calib=blk.calib, raw=args.raw_signal, out=b)

    seen = 0
    pending = None
    with ThreadPoolExecutor(1) as ex:
        try:
            for k, blk in enumerate(fastio.iter_blow5_blocks_i16(args.blow5, keep=_KEEP)):
                rate = [next(rates) for _ in range(blk.n)] if rates is not None else None
                ok = np.flatnonzero((blk.flags & 2) == 0)
                for i in np.flatnonzero(blk.flags & 2):
                    sys.stderr.write("SquigglePull: unreadable BLOW5 record {} in {}; skipped\n".format(seen + int(i), args.blow5))
                seen += blk.n
                if ok.size != blk.n:
                    blk = fastio.Blow5Block(blk.rows[ok], blk.nsamp[ok], blk.ids[ok], blk.calib[ok], blk.flags[ok])
                    rate = [rate[i] for i in ok] if rate is not None else None
                if rates is not None:
                    prefixes = [_prefix(name.decode("utf-8", "surrogateescape"),
                                        {'readID': rid.decode(), 'digitisation': cal[0], 'offset': cal[1],
                                         'range': float("{0:.2f}".format(cal[2])), 'sampling_rate': sr}, True)
                                for rid, cal, sr in zip(blk.ids, blk.calib.tolist(), rate)]
                else:
                    prefixes = [b"%s\t%s\t" % (name, rid) for rid in blk.ids]
                fut = ex.submit(gpu, k, blk, prefixes)
                if pending is not None:
                    _write(pending.result())
                pending = fut
        except ValueError as e:                          # truncated file, unsupported compression: say so, no traceback
            if pending is not None:
                _write(pending.result())
            sys.stderr.write("SquigglePull: --blow5: {}\n".format(e))
            sys.exit(1)
        if pending is not None:
            _write(pending.result())


def main(argv=None):
    parser = build_parser()
    argv = sys.argv[1:] if argv is None else argv
    args = parser.parse_args(argv)
    if len(argv) == 0:                              # SquigglePull.py:97-99
        parser.print_help(sys.stderr)
        sys.exit(1)
    if args.verbose:
        sys.stderr.write("Verbose mode on. Starting timer.\n")
        start_time = time.time()
    del _KEEP[:]
    if args.blow5:
        _blow5(args)
    else:
        if not os.path.isdir(args.path):
            sys.stderr.write("The provided path {} is not an existing directory.\n".format(args.path))
            sys.exit(1)
        out = _Lines()
        try:
            _walk(args, out)
        except BaseException:
            out.flush()                             # the lines the reference had printed before it stopped
            raise
        out.flush()
    if args.verbose:
        end_time = time.time() - start_time
        sys.stderr.write("Time taken: {}\n".format(end_time))


if __name__ == "__main__":
    main()
