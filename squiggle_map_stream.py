#!/usr/bin/env python3
"""squiggle_map_stream.py -- map each read's event levels to reference squiggles as they arrive: replays a file through a
mapping session on the MI355X.  Thin launcher; the tool lives in squigglekit_amd/mapstream_cli.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from squigglekit_amd.mapstream_cli import main  # noqa: E402

if __name__ == "__main__":
    main()
