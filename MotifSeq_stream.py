#!/usr/bin/env python3
"""MotifSeq_stream.py -- MotifSeq on reads that arrive chunk by chunk: replays a file through a MotifSeq session.
Thin launcher; the tool lives in squigglekit_amd/stream_cli.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from squigglekit_amd.stream_cli import main  # noqa: E402

if __name__ == "__main__":
    main()
