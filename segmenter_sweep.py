#!/usr/bin/env python3
"""segmenter_sweep.py -- a grid of segmenter.py settings scored over the same reads in one GPU pass.
Thin launcher; the tool lives in squigglekit_amd/sweep_cli.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from squigglekit_amd.sweep_cli import main  # noqa: E402

if __name__ == "__main__":
    main()
