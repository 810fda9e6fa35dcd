#!/usr/bin/env python3
"""dRNA_polya_stream.py -- adapter and poly(A) coordinates of direct-RNA reads that arrive chunk by chunk: replays a file
through an HMM session.  Thin launcher; the tool lives in squigglekit_amd/polya_stream_cli.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from squigglekit_amd.polya_stream_cli import main  # noqa: E402

if __name__ == "__main__":
    main()
