"""Time the two kernels of csrc/tile.hip on one clip of whole frames (default: 30 frames of 352x288 and of 1920x1080, tiles of
128 overlapping by 16): HIP events around back-to-back launches after a warm-up, several windows, with the bytes each launch
moves -- counted from the shapes -- beside the time.  The gather reads every source byte a tile holds and writes it once; the
blend reads every tile value and writes every pixel once.

    python tools/tile_time.py [--frames 30] [--sizes 352x288 1920x1080] [--size 128] [--overlap 16] [--launches 200] [--windows 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import evc_amd  # noqa: E402,F401
from evc_amd import lib as L  # noqa: E402
from evc_amd import video_io as V  # noqa: E402


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
    p.add_argument("--sizes", type=str, nargs="+", default=["352x288", "1920x1080"], help="WxH of the source frames")
    p.add_argument("--size", type=int, default=128, help="tile size")
    p.add_argument("--overlap", type=int, default=16)
    p.add_argument("--launches", type=int, default=200)
    p.add_argument("--windows", type=int, default=5)
    a = p.parse_args()
    L.hip_lib()
    T, S = a.frames, a.size
    for wh in a.sizes:
        W, H = (int(v) for v in wh.lower().split("x"))
        oy, ox = V.tile_grid(H, W, S, a.overlap)
        tiles = len(oy) * len(ox)
        x = torch.randint(0, 256, (T, 3, H, W), dtype=torch.uint8, device="cuda")
        t = L.tile_gather_u8(x, S, oy, ox).float() / 255.0
        tile_values, pixels = tiles * T * 3 * S * S, T * 3 * H * W
        # the blend reads a tile's values only where they lie inside the frame (an axis shorter than S)
        read_values = T * 3 * sum(min(S, H - y0) for y0 in oy) * sum(min(S, W - x0) for x0 in ox)
        cases = {
            "tile_gather_u8": (lambda: L.tile_gather_u8(x, S, oy, ox), 2 * tile_values),
            "tile_blend": (lambda: L.tile_blend(t, H, W, oy, ox), 4 * (read_values + pixels)),
        }
        for name, (fn, nbytes) in cases.items():
            window(fn, 20)                              # warm-up: code object load, clocks, the allocator's blocks
            us = sorted(window(fn, a.launches) for _ in range(a.windows))
            print(json.dumps({"kernel": name, "frames": T, "width": W, "height": H, "tiles": f"{len(oy)}x{len(ox)}", "size": S,
                              "overlap": a.overlap, "bytes": nbytes, "us_per_launch_median": round(us[len(us) // 2], 3),
                              "us_min": round(us[0], 3), "us_max": round(us[-1], 3),
                              "GB_per_s": round(nbytes / us[len(us) // 2] / 1e3, 1), "launches_per_window": a.launches}), flush=True)


if __name__ == "__main__":
    main()
