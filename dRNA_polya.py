#!/usr/bin/env python3
"""dRNA_polya.py -- adapter and poly(A) tail coordinates of direct-RNA reads by a signal HMM on the MI355X.
Thin launcher; the tool lives in squigglekit_amd/polya_cli.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from squigglekit_amd import _warm  # noqa: E402
_warm.start()                      # the GPU context comes up while numpy and the tool are being imported
from squigglekit_amd.polya_cli import main  # noqa: E402

if __name__ == "__main__":
    main()
    _warm.fast_exit(0)             # (sys.exit inside main() leaves the ordinary way)
