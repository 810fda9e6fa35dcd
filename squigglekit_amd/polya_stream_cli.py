"""dRNA_polya_stream -- replay a file of direct-RNA reads as if it arrived live, chunk by chunk, through an HMM session.

    dRNA_polya_stream.py -f reads.blow5 | -s signals.tsv | --i16 FILE.npy  [--preset rna_pa|synth_raw] [--model FILE.json]
                         [--sample_chunk N] [--channels S] [--min_body N] [--min_margin X] [--give_up N] [--device D]
                         [--min_post P] [--min_rate R]

`--channels S` reads are in flight at a time, each in a slot of one session (api.HmmStream) under dRNA_polya.py's
six-state model; every round pushes the next `--sample_chunk N` samples of each.  After each push a read is decided
(api.polya_decide): accepted when its best path ends in TRANSCRIPT, has been there for at least --min_body samples and
TRANSCRIPT's score leads every other state's by at least --min_margin; rejected when it is not accepted and --give_up
samples have gone by (0: never); otherwise it goes on, and a read that runs out of samples is decided `end`.  A decided
read frees its slot for the next one.  The decision is a heuristic: the entry into TRANSCRIPT can still move while POLYA
stays competitive, which is what the margin is for.

--min_post P        decide by probability instead (api.polya_decide_post): the session is opened filtered
                    (api.HmmStream(filter=True)) and a read is accepted when its best path ends in TRANSCRIPT, has been
                    there for --min_body samples and P(TRANSCRIPT at the newest sample | the samples so far) >= P;
                    --min_margin is then ignored.  Every line gets two more columns, loglik_per_sample and p_transcript,
                    written as dRNA_polya.py --posterior writes them (`.` for a read without samples or one the model
                    gives probability 0) -- for a read that ran to its `end` they are that tool's columns of the same
                    read.  What is probabilistic is that the transcript has begun; where still comes from the best path.
--min_rate R        with --min_post: also reject a read of at least --min_body samples whose loglik per sample is below R
                    (a read the model fits badly).  Alone it turns --min_post's columns and rule on with P = 0.

Output, tab separated, one line per read at the moment of its decision and no header:
    readID adapter_start adapter_end polya_start polya_end polya_samples score_per_sample decision pushes samples_seen
The first seven columns are dRNA_polya.py's, computed from the record at that moment -- for a read that ran to its `end`
they are dRNA_polya.py's line of the same read, byte for byte.  Lines come in the order the decisions fall, slot by slot
within a round.

The model sees pA for a BLOW5 file under a pA preset (the record's calibration goes to the slot with its reset) and the
values as they stand otherwise: integer reads go through the int16 feed, pA text through the float64 one."""
import argparse
import sys

import numpy as np

from . import _lib, api
from .polya_cli import PA_PRESETS, iter_input, polya_lines


class _Parser(argparse.ArgumentParser):
    def error(self, message):
        self.print_usage(sys.stderr)
        sys.stderr.write("dRNA_polya_stream: error: {}\n".format(message))
        sys.exit(2)


def build_parser():
    p = _Parser(prog="dRNA_polya_stream", description="adapter and poly(A) coordinates of direct-RNA reads that arrive chunk "
                                                      "by chunk (replay of a file)")
    src = p.add_mutually_exclusive_group()
    src.add_argument("-f", "--blow5", help="BLOW5 file (uncompressed or zlib records)")
    src.add_argument("-s", "--signal", help="signal TSV written by SquigglePull: pA values, or raw integers with -r (.gz accepted)")
    src.add_argument("--i16", help="packed reads: a .npy file holding an int16 array [reads, samples] (read name = row index)")
    p.add_argument("--preset", default="rna_pa", choices=sorted(api.POLYA_PRESETS), help="model preset (default rna_pa)")
    p.add_argument("--model", help="model description (JSON, api.hmm_spec_to_json) in place of the preset's numbers")
    p.add_argument("--device", type=int, default=None, help="GPU index (default $SK_DEVICE or 0)")
    p.add_argument("--sample_chunk", type=int, default=2000, metavar="N", help="samples per push and read (0.4 s at 5 kHz)")
    p.add_argument("--channels", type=int, default=512, metavar="S", help="reads in flight at a time")
    p.add_argument("--min_body", type=int, default=2000, metavar="N", help="accept: samples the path has been in TRANSCRIPT")
    p.add_argument("--min_margin", type=float, default=20.0, metavar="X",
                   help="accept: TRANSCRIPT's lead over every other state (ignored with --min_post / --min_rate)")
    p.add_argument("--give_up", type=int, default=0, metavar="N", help="reject a read not accepted after N samples (0: never)")
    p.add_argument("--min_post", type=float, default=None, metavar="P",
                   help="accept by P(TRANSCRIPT | samples so far) >= P in place of --min_margin; adds loglik_per_sample and "
                        "p_transcript columns")
    p.add_argument("--min_rate", type=float, default=None, metavar="R",
                   help="with --min_post: reject a read of --min_body samples or more whose loglik per sample is below R")
    return p


def filter_columns(filt):
    """loglik_per_sample and p_transcript of one filter (HMMS_FILT_DTYPE [1]), as dRNA_polya.py --posterior writes them"""
    n = int(filt["n_used"][0])
    if n <= 0 or int(filt["flags"][0]) != 0:
        return [".", "."]
    return ["{}".format(float(filt["loglik"][0]) / n), "{}".format(float(filt["post"][0][api.TRANSCRIPT]))]


def decided_line(rid, rec, decision, filt=None):
    """the line of one decided read from its record (HMMS_DTYPE [1]) and, in a filtered run, its filter"""
    cols = [polya_lines([rid], rec)[0].rstrip("\n"), decision, str(int(rec["pushes"][0])), str(int(rec["n_used"][0]))]
    if filt is not None:
        cols += filter_columns(filt)
    return "\t".join(cols) + "\n"


def main(argv=None):
    parser = build_parser()
    argv = sys.argv[1:] if argv is None else argv
    a = parser.parse_args(argv)
    if len(argv) == 0:
        parser.print_help(sys.stderr)
        sys.exit(1)
    if not (a.signal or a.blow5 or a.i16):
        parser.error("one of -f/--blow5, -s/--signal, --i16 is needed")
    if a.sample_chunk < 1:
        parser.error("--sample_chunk must be at least 1, got {}".format(a.sample_chunk))
    if not 1 <= a.channels <= _lib.SK_HMMS_MAX_SLOTS:
        parser.error("--channels must be in 1 .. {}, got {}".format(_lib.SK_HMMS_MAX_SLOTS, a.channels))
    if a.min_body < 0 or a.give_up < 0:
        parser.error("--min_body and --give_up must be >= 0")
    filtered = a.min_post is not None or a.min_rate is not None
    if filtered and not 0.0 <= (a.min_post or 0.0) <= 1.0:
        parser.error("--min_post must be in [0, 1], got {}".format(a.min_post))
    tool_input = a.signal or a.blow5 or a.i16
    _lib.warm_start(a.device, also=())
    try:
        spec = None
        if a.model:
            with open(a.model) as fh:
                spec = api.hmm_spec_from_json(fh.read())
        model = api.polya_model(a.preset) if spec is None else api.hmm_model(*spec)
        if model.nstates != 6:
            raise ValueError("the decision reads the six states of api.POLYA_STATES; the model has {}".format(model.nstates))
        reads = iter_input(a, a.preset in PA_PRESETS, 4096)
        pending = next(reads, None)
        if pending is None:
            return
        S = a.channels
        free, flight = list(range(S - 1, -1, -1)), {}        # slot -> [readID, samples, position, is int16]
        with api.HmmStream(model, S, filter=filtered) as hs:
            while pending is not None or flight:
                fresh, cals = [], []
                while pending is not None and free:
                    rid, sig, cal = pending
                    if len(sig) == 0:
                        sys.stderr.write("dRNA_polya_stream: no samples in read {} of {}\n".format(rid, tool_input))
                    s = free.pop()
                    sig = np.asarray(sig)
                    flight[s] = [rid, sig, 0, sig.dtype == np.int16]
                    fresh.append(s)
                    cals.append((0.0, 1.0) if cal is None else cal)
                    pending = next(reads, None)
                if fresh:
                    hs.reset(fresh, np.array(cals, dtype=np.float64))
                rec, filt = {}, {}
                for ints in (True, False):                   # raw integers through the int16 feed, pA text through the float64 one
                    slots = [s for s in sorted(flight) if flight[s][3] == ints]
                    if not slots:
                        continue
                    chunks = []
                    for s in slots:
                        _, sig, pos, _ = flight[s]
                        chunks.append(sig[pos:pos + a.sample_chunk])
                        flight[s][2] = pos + len(chunks[-1])
                    out = hs.push(slots, chunks) if ints else hs.push_values(slots, chunks)
                    fout = hs.filter(slots) if filtered else None
                    for i, s in enumerate(slots):
                        rec[s] = out[i:i + 1]
                        if filtered:
                            filt[s] = fout[i:i + 1]
                text = []
                for s in sorted(rec):
                    if filtered:
                        dec = int(api.polya_decide_post(rec[s], filt[s], a.min_body, a.min_post or 0.0, a.give_up, a.min_rate)[0])
                    else:
                        dec = int(api.polya_decide(rec[s], a.min_body, a.min_margin, a.give_up)[0])
                    ended = flight[s][2] >= len(flight[s][1])
                    if dec == 0 and not ended:
                        continue
                    text.append(decided_line(flight[s][0], rec[s], "accept" if dec == 1 else "reject" if dec == -1 else "end",
                                             filt.get(s)))
                    del flight[s]
                    free.append(s)
                sys.stdout.write("".join(text))
    except (ValueError, EOFError, OSError) as e:
        sys.stdout.flush()
        sys.stderr.write("dRNA_polya_stream: {}: {}\n".format(tool_input, e))
        sys.exit(2)
    sys.stdout.flush()


if __name__ == "__main__":
    main()
