#!/usr/bin/env python3
"""Blends the tiles ``city_receiver.py`` decoded from a ``city_sender.py --yuv-fit tile`` run back into whole frames (the
reference has no counterpart: it only sees frames of the model's size); the implementation is evc_amd/stitch.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evc_amd  # noqa: E402,F401
from evc_amd.stitch import main  # noqa: E402

if __name__ == "__main__":
    main()
