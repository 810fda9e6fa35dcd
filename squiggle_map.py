#!/usr/bin/env python3
"""squiggle_map.py -- map the event levels of each read's first samples to reference squiggles by DTW on the MI355X.
Thin launcher; the tool lives in squigglekit_amd/map_cli.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from squigglekit_amd import _warm  # noqa: E402
_warm.start()                      # the GPU context comes up while numpy and the tool are being imported
from squigglekit_amd.map_cli import main  # noqa: E402

if __name__ == "__main__":
    main()
    _warm.fast_exit(0)             # (sys.exit inside main() leaves the ordinary way)
