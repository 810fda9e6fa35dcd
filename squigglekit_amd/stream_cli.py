"""MotifSeq_stream -- replay a file of raw reads as if it arrived live, chunk by chunk, through a MotifSeq session.

`--channels S` reads are in flight at a time, each in a slot of one session (api.MotifStream); every round pushes the
next `--chunk C` samples of each.  After each push a read is decided: accepted when a motif's Z-score (MotifSeq.py's
distance model: mean = slope * L + intercept, sd = mean * std_const) is at or below --accept_Z, rejected when no motif
accepts and `--give_up` kept samples have gone by, and otherwise it goes on; a read that runs out of samples is flushed
(decision `end`).  A decided read frees its slot for the next one.  One line per read and motif: MotifSeq.py's twelve
columns computed from the record at the moment of decision, then decision, chunks, samples_seen.

Input is raw integer samples only -- a session calibrates on raw values: --blow5, --i16, or a SquigglePull -r TSV (-s).
"""
import argparse
import os
import sys

import numpy as np

from . import _lib, api, tsvio
from .motifseq_cli import HEADER, DistanceModel, load_models

STREAM_HEADER = HEADER + ["decision", "chunks", "samples_seen"]


class _Parser(argparse.ArgumentParser):
    def error(self, message):
        self.print_usage(sys.stderr)
        sys.stderr.write("MotifSeq_stream: error: {}\n".format(message))
        sys.exit(2)


def build_parser():
    p = _Parser(prog="MotifSeq_stream", description="MotifSeq on reads that arrive chunk by chunk (replay of a file)")
    src = p.add_mutually_exclusive_group()
    src.add_argument("-s", "--signal", help="raw-integer signal TSV written by SquigglePull -r (.gz accepted)")
    src.add_argument("--blow5", help="BLOW5 file (stored or zlib records): raw ADC values")
    src.add_argument("--i16", help="packed reads: a .npy file holding an int16 array [reads, samples]")
    mod = p.add_mutually_exclusive_group()
    mod.add_argument("-i", "--fasta_input", help="fasta of motifs, turned into squiggles with scrappy")
    mod.add_argument("-m", "--model", help="pre-computed motif signal: scrappie squiggle text or name/len/x/values TSV")
    p.add_argument("--scrappie_model", default="squiggle_r94")
    p.add_argument("-l", "--scale", default="medmad", choices=["zscale", "medmad"])
    p.add_argument("-scale_hi", "--scale_hi", type=int, default=1200, help="samples >= this are dropped")
    p.add_argument("-scale_low", "--scale_low", type=int, default=0, help="samples <= this are dropped")
    p.add_argument("--slope", type=float, default=2.90, help="[experimental] distance model slope")
    p.add_argument("--intercept", type=float, default=-9.6, help="[experimental] distance model intercept")
    p.add_argument("--std_const", type=float, default=0.08468, help="[experimental] distance model stdev factor")
    p.add_argument("--chunk", type=int, default=2000, metavar="C", help="samples per push and read (0.4 s at 5 kHz)")
    p.add_argument("--calib", type=int, default=2000, metavar="W", help="kept samples a read calibrates on")
    p.add_argument("--channels", type=int, default=512, metavar="S", help="reads in flight at a time")
    p.add_argument("--accept_Z", type=float, default=None, metavar="Z", help="accept a read when a motif scores at or below Z")
    p.add_argument("--give_up", type=int, default=None, metavar="N", help="reject a read no motif accepted after N kept samples")
    p.add_argument("--device", type=int, default=None, help="GPU index (default $SK_DEVICE or 0)")
    p.add_argument("--strict-compat", action="store_true", help=argparse.SUPPRESS)      # (load_models looks at it)
    return p


def check_args(parser, a):
    if a.chunk < 1:
        parser.error("--chunk must be at least 1, got {}".format(a.chunk))
    if not 1 <= a.calib <= _lib.SK_STREAM_MAX_CALIB:
        parser.error("--calib must be in 1 .. {}, got {}".format(_lib.SK_STREAM_MAX_CALIB, a.calib))
    if not 1 <= a.channels <= _lib.SK_STREAM_MAX_SLOTS:
        parser.error("--channels must be in 1 .. {}, got {}".format(_lib.SK_STREAM_MAX_SLOTS, a.channels))
    if a.give_up is not None and a.give_up < 1:
        parser.error("--give_up must be at least 1, got {}".format(a.give_up))


def iter_reads(parser, a):
    """(fast5, readID, int16 samples) of every read of the input"""
    if a.blow5:
        from .blow5 import read_blow5
        name = os.path.basename(a.blow5)
        for rec in read_blow5(a.blow5):
            yield name, rec["read_id"], np.ascontiguousarray(rec["signal"], dtype=np.int16)
    elif a.i16:
        rows = np.load(a.i16, mmap_mode="r")
        if rows.dtype != np.int16 or rows.ndim != 2:
            parser.error("--i16 takes an int16 array [reads, samples]")
        name = os.path.basename(a.i16)
        for r in range(rows.shape[0]):
            yield name, str(r), np.ascontiguousarray(rows[r])
    else:
        with tsvio.open_text(a.signal) as fh:
            for line in fh:
                if not line.strip():
                    continue
                fast5, read_id, sig = tsvio.parse_motifseq_line(line)
                raw = api.as_int16_exact(sig)
                if raw is None:
                    parser.error("-s {}: read {} holds values that are not raw integers (pA?): a session calibrates on "
                                 "raw samples -- write the TSV with SquigglePull -r, or use --blow5 / --i16"
                                 .format(a.signal, read_id))
                yield fast5, read_id, raw


def lines_of(a, meta, rec, order, lens, decision):
    """The K lines of one decided read from its records rec [K]; None (and a note on stderr) for a read without a search"""
    fast5, read_id = meta
    flags = int(rec[0]["flags"])
    if flags & _lib.SK_FLAG_EMPTY:
        sys.stderr.write("MotifSeq_stream: no sample of {} survived the outlier limits; skipped\n".format(read_id))
        return None
    if flags & _lib.SK_FLAG_DEGENERATE:
        sys.stderr.write("MotifSeq_stream: the MAD of the calibration samples of {} is 0; skipped\n".format(read_id))
        return None
    out = []
    model = DistanceModel(a, lens)
    for k, name in enumerate(order):
        dist, start, end = float(rec[k]["dist"]), int(rec[k]["start"]), int(rec[k]["end"])
        z, p_value, hit_p = model.score(dist, k)
        row = [fast5, read_id, name, start, end, end - start, dist, model.mean[k], model.stdev[k], z, p_value, hit_p, decision,
               int(rec[k]["chunks"]), int(rec[k]["seen"])]
        out.append("\t".join("{}".format(v) for v in row))
    return out


def main(argv=None):
    parser = build_parser()
    argv = sys.argv[1:] if argv is None else argv
    a = parser.parse_args(argv)
    if len(argv) == 0:
        parser.print_help(sys.stderr)
        sys.exit(1)
    check_args(parser, a)
    if not (a.signal or a.blow5 or a.i16):
        parser.error("no input: one of -s, --blow5, --i16")
    models, order, lens = load_models(a)
    if not order:
        parser.error("no motif: -m or -i")
    reads = iter_reads(parser, a)
    first = next(reads, None)                        # (a refused input says so before the device is looked at)
    print("\t".join(STREAM_HEADER))
    if first is None:
        return
    motifs = [np.asarray(models[name], dtype=np.float64) for name in order]
    means = np.array([(a.slope * n) + a.intercept for n in lens], dtype=np.float64)
    sds = means * a.std_const
    accept_z = -np.inf if a.accept_Z is None else a.accept_Z
    give_up = np.iinfo(np.int32).max if a.give_up is None else a.give_up
    _lib.init(a.device)
    S = a.channels
    free, flight = list(range(S - 1, -1, -1)), {}    # slot -> [meta, samples, position]
    pending = first
    with api.MotifStream(motifs, S, a.scale, a.scale_low, a.scale_hi, calib=a.calib) as ms:
        while pending is not None or flight:
            fresh = []
            while pending is not None and free:
                s = free.pop()
                flight[s] = [(pending[0], pending[1]), pending[2], 0]
                fresh.append(s)
                pending = next(reads, None)
            if fresh:
                ms.reset(fresh)
            slots = sorted(flight)
            chunks = []
            for s in slots:
                _, sig, pos = flight[s]
                chunks.append(sig[pos:pos + a.chunk])
                flight[s][2] = pos + len(chunks[-1])
            rec = ms.push(slots, chunks)
            dec = api.stream_decide(rec, means, sds, accept_z, give_up)
            done, ended = [], []
            for i, s in enumerate(slots):
                if (dec[:, i] == 1).any():
                    done.append((s, rec[:, i], "accept"))
                elif (dec[:, i] == -1).all():
                    done.append((s, rec[:, i], "reject"))
                elif flight[s][2] >= len(flight[s][1]):
                    ended.append(s)
            if ended:
                frec = ms.flush(ended)
                done += [(s, frec[:, i], "end") for i, s in enumerate(ended)]
            for s, r, decision in sorted(done, key=lambda d: d[0]):
                text = lines_of(a, flight[s][0], r, order, lens, decision)
                if text:
                    print("\n".join(text))
                del flight[s]
                free.append(s)


if __name__ == "__main__":
    main()
