#!/usr/bin/env python3
"""Goldens for the SquigglePull drop-in (run where the reference checkout is, as tools/gen_golden.py).

    python tools/gen_golden_pull.py

Runs the reference's own SquigglePull.main() with `h5py` stood in by squigglekit_amd.hdf5min (h5py is not installable
here) on temporary trees holding tests/golden/example_test.fast5 (a single-read file), tests/golden/multi_two_reads.fast5
(two reads) and tests/golden/multi_partial.fast5 (laid out here by tools/hdf5_write_min.py: one complete read, one
without its channel_id group, one whose channel_id lacks sampling_rate -- the reference prints partial lines for them).
Captures stdout, stderr and the exit code of each run; an exception the reference does not catch is recorded as Python
reports it (traceback on stderr, exit 1).  A long stdout is stored as its length, SHA-256 and first / last 4 KiB.
Paths are masked as <TMP>, the -v timer as <t>.  Outputs only -- no reference source is stored."""
import contextlib
import gzip
import hashlib
import io
import json
import os
import re
import shutil
import sys
import tempfile
import traceback
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from squigglekit_amd import hdf5min                       # noqa: E402
from gen_golden import REF                                # noqa: E402

EDGE = 4096
LONG = 16384


def stored(text):
    """A run's stdout as kept in the golden: the text itself, or its digest when it is long."""
    if len(text) <= LONG:
        return {"text": text}
    b = text.encode("utf-8", "surrogateescape")
    return {"bytes": len(b), "sha256": hashlib.sha256(b).hexdigest(), "head": b[:EDGE].decode(), "tail": b[-EDGE:].decode()}


def run_main(mod, argv):
    out, err = io.StringIO(), io.StringIO()
    old = sys.argv
    sys.argv = argv
    code = 0
    try:
        with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
            try:
                mod.main()
            except SystemExit as e:
                code = e.code if isinstance(e.code, int) else 1
            except Exception:                                # uncaught in the reference: Python prints it, exit 1
                traceback.print_exc()
                code = 1
    finally:
        sys.argv = old
    return out.getvalue(), err.getvalue(), code


def partial_fixture(path):
    """Three reads cut from the example read; the second has no channel_id, the third no sampling_rate."""
    from hdf5_write_min import write_hdf5
    with hdf5min.File(os.path.join(GOLD, "example_test.fast5")) as f:
        name = list(f["Raw/Reads"].keys())[0]
        sig = f["Raw/Reads"][name]["Signal"][()]
        ch = {k: float(v) for k, v in f["UniqueGlobalKey/channel_id"].attrs.items()
              if k in ("digitisation", "offset", "range", "sampling_rate")}
    chan = {"@" + k: v for k, v in ch.items()}
    no_rate = {k: v for k, v in chan.items() if k != "@sampling_rate"}
    ids = ["0a1b2c3d-aaaa-4bbb-8ccc-0000000000%02d" % i for i in (11, 12, 13)]
    tree = {"read_" + ids[0]: {"Raw": {"@read_id": ids[0].encode(), "Signal": np.ascontiguousarray(sig[100:1100])},
                               "channel_id": dict(chan, **{"@offset": -3.5})},
            "read_" + ids[1]: {"Raw": {"@read_id": ids[1].encode(), "Signal": np.ascontiguousarray(sig[2000:2600])}},
            "read_" + ids[2]: {"Raw": {"@read_id": ids[2].encode(), "Signal": np.ascontiguousarray(sig[5000:5700])},
                               "channel_id": no_rate}}
    write_hdf5(path, tree)


def main():
    h5 = types.ModuleType("h5py")
    h5.File = lambda path, mode="r": hdf5min.File(path)
    sys.modules["h5py"] = h5
    sys.path.insert(0, REF)
    import SquigglePull as ref
    ref.h5py = h5
    partial_fixture(os.path.join(GOLD, "multi_partial.fast5"))
    tmp = tempfile.mkdtemp()
    layout = {"reads/example_test.fast5": "example_test.fast5",                 # (one file per directory: os.walk
              "reads/m/multi_two_reads.fast5": "multi_two_reads.fast5",          #  order is then the same everywhere)
              "reads/m/p/multi_partial.fast5": "multi_partial.fast5",
              "single/example_test.fast5": "example_test.fast5",
              "multi/multi_two_reads.fast5": "multi_two_reads.fast5"}
    for dst, src in layout.items():
        os.makedirs(os.path.dirname(os.path.join(tmp, dst)), exist_ok=True)
        shutil.copyfile(os.path.join(GOLD, src), os.path.join(tmp, dst))
    os.makedirs(os.path.join(tmp, "bad"))
    with open(os.path.join(tmp, "bad", "broken.fast5"), "wb") as fh:
        fh.write(b"this is not an HDF5 file\n" * 40)
    with open(os.path.join(tmp, "bad", "notes.txt"), "w") as fh:
        fh.write("not a fast5\n")
    t = "<TMP>"
    argvs = [["-p", t + "/reads"], ["-p", t + "/reads", "-r"], ["-p", t + "/reads", "-i"], ["-p", t + "/reads", "-r", "-i"],
             ["-p", t + "/single", "-t", "single"], ["-p", t + "/multi", "-t", "multi"], ["-p", t + "/single", "-t", "multi"],
             ["-p", t + "/multi", "-t", "single", "-i"], ["-p", t + "/single", "-v"], ["-p", t + "/bad"],
             ["-p", t + "/missing"], ["-r"], [], ["--bogus"], ["-p", t + "/reads", "-t", "both"]]
    runs = []
    for argv in argvs:
        so, se, code = run_main(ref, ["SquigglePull.py"] + [a.replace(t, tmp) for a in argv])
        so, se = so.replace(tmp, t), re.sub(r"Time taken: \S+\n", "Time taken: <t>\n", se.replace(tmp, t))   # (-v's timer)
        runs.append({"argv": argv, "stdout": stored(so), "stderr": se, "exit": code})
        print(argv, "->", len(so), "bytes,", repr(so[:70]), "| exit", code, "| stderr tail:", repr(se[-100:]))
    shutil.rmtree(tmp)
    with gzip.GzipFile(os.path.join(GOLD, "squigglepull_cli.json.gz"), "wb", mtime=0) as gz:
        gz.write(json.dumps({"generator": "tools/gen_golden_pull.py: the reference's SquigglePull.py main(); h5py stood in "
                                          "by squigglekit_amd.hdf5min",
                             "layout": layout, "runs": runs}, indent=1, sort_keys=True).encode())


if __name__ == "__main__":
    main()
