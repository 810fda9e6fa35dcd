#!/usr/bin/env python3
"""squiggle_compare.py -- compare two squiggle_map.py --pileup tables point by point (host only, no GPU).
Thin launcher; the tool lives in squigglekit_amd/compare_cli.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from squigglekit_amd.compare_cli import main  # noqa: E402

if __name__ == "__main__":
    main()
