#!/usr/bin/env python3
"""Receiver for the job streams of ``city_sender.py --policy psnr|lpips --bitstream-dir DIR`` (the reference has none: its
generator runs inside the sender); the implementation is evc_amd/receiver.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evc_amd  # noqa: E402,F401
from evc_amd.receiver import main  # noqa: E402

if __name__ == "__main__":
    main()
