"""Time the two kernels of csrc/yuv.hip on one clip (default 30 frames of 128x128, 8 bits): HIP events around back-to-back
launches after a warm-up, several windows, with the bytes each launch moves beside the time.

    python tools/yuv_time.py [--frames 30] [--size 128] [--bits 8] [--launches 2000] [--windows 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import evc_amd  # noqa: E402,F401
from evc_amd import lib as L  # noqa: E402


def window(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches       # microseconds per launch


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frames", type=int, default=30)
    p.add_argument("--size", type=int, default=128)
    p.add_argument("--bits", type=int, default=8)
    p.add_argument("--launches", type=int, default=2000)
    p.add_argument("--windows", type=int, default=5)
    a = p.parse_args()
    L.hip_lib()
    T, S = a.frames, a.size
    samples = T * L.yuv420_frame_bytes(S, S, a.bits)
    x = torch.rand((T, 3, S, S), device="cuda")
    events = torch.zeros(1, dtype=torch.int32, device="cuda")
    buf = L.rgb_to_yuv420(x, events, a.bits)
    out_f = torch.empty((T, 3, S, S), device="cuda")
    out_u = torch.empty((T, 3, S, S), device="cuda", dtype=torch.uint8)
    cases = {
        "rgb_to_yuv420": (lambda: L.rgb_to_yuv420(x, events, a.bits, buf=buf), x.numel() * 4 + samples),
        "yuv420_to_rgb bicubic float32": (lambda: L.yuv420_to_rgb(buf, T, S, S, a.bits, "bicubic", out=out_f), samples + out_f.numel() * 4),
        "yuv420_to_rgb bicubic uint8": (lambda: L.yuv420_to_rgb(buf, T, S, S, a.bits, "bicubic", dtype=torch.uint8, out=out_u),
                                        samples + out_u.numel()),
        "yuv420_to_rgb nearest float32": (lambda: L.yuv420_to_rgb(buf, T, S, S, a.bits, "nearest", out=out_f), samples + out_f.numel() * 4),
    }
    for name, (fn, nbytes) in cases.items():
        window(fn, 200)                             # warm-up: code object load, clocks
        us = sorted(window(fn, a.launches) for _ in range(a.windows))
        print(json.dumps({"kernel": name, "frames": T, "size": S, "bits": a.bits, "bytes": nbytes, "us_per_launch_median": round(us[len(us) // 2], 3),
                          "us_min": round(us[0], 3), "us_max": round(us[-1], 3), "GB_per_s": round(nbytes / us[len(us) // 2] / 1e3, 1),
                          "launches_per_window": a.launches}), flush=True)
    assert int(events.item()) == 0


if __name__ == "__main__":
    main()
