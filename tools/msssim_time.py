"""Time MS-SSIM (csrc/msssim.hip) on one 30-frame clip (90 planes) at 352x288 and at 1920x1080, next to SSIM (csrc/ssim.hip) on
the same device tensors: HIP events around back-to-back calls after a warm-up, several windows.  A call is the library entry
with its workspace allocation (``lib.msssim_levels``: four pool launches, one tile launch over all levels, one finishing
launch; ``lib.ssim_planes``: two launches).  The bytes of a call are counted from the shapes: both inputs read once, the two
float64 pyramids written once and read twice (by the next pool launch and by the tile launch; the last level once), two
doubles per tile written and read.  No time is gated; the ratio to SSIM on the same box is the figure to keep.

    python tools/msssim_time.py [--launches 800] [--windows 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import evc_amd  # noqa: E402,F401
from evc_amd import lib as L, msssim as M, ssim as S  # noqa: E402


def window(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches       # microseconds per call


def pyramid(H, W, levels):
    sizes = [(H, W)]
    for _ in range(levels - 1):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    return sizes


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--launches", type=int, default=800)
    p.add_argument("--windows", type=int, default=5)
    a = p.parse_args()
    so = L.hip_lib()
    taps = torch.from_numpy(S.gaussian_taps()).cuda()
    levels, planes = len(M.WEIGHTS), 90
    for name, (H, W) in (("352x288", (288, 352)), ("1920x1080", (1080, 1920))):
        x = torch.rand((planes, H, W), device="cuda")
        y = (x + 0.05 * torch.randn_like(x)).clamp_(0, 1)
        out_ms = torch.empty((planes, levels, 2), dtype=torch.float64, device="cuda")
        out_s = torch.empty(planes, dtype=torch.float64, device="cuda")
        sizes = pyramid(H, W, levels)
        inputs = 2 * x.numel() * 4
        pyr = 2 * planes * 8 * (sum(h * w for h, w in sizes[1:]) + 2 * sum(h * w for h, w in sizes[1:-1]) + sizes[-1][0] * sizes[-1][1])
        partial_ms = so.evc_msssim_workspace_bytes(planes, H, W, levels) - 2 * planes * 8 * sum(h * w for h, w in sizes[1:])
        nbytes = {"evc_msssim_levels_f32": 2 * inputs + pyr + 2 * partial_ms + out_ms.numel() * 8,      # level 0 is read by the pool and by the tiles
                  "evc_ssim_planes_f32": inputs + 2 * so.evc_ssim_workspace_bytes(planes, H, W) + planes * 8}
        cases = {"evc_msssim_levels_f32": lambda: L.msssim_levels(x, y, levels, taps, S.C1, S.C2, out=out_ms),
                 "evc_ssim_planes_f32": lambda: L.ssim_planes(x, y, taps, S.C1, S.C2, out=out_s)}
        launches = max(20, a.launches if H * W < 1 << 20 else a.launches // 4)
        med = {}
        for kernel, fn in cases.items():
            window(fn, max(3, launches // 10))                      # warm-up: code object load, clocks, allocator
            us = sorted(window(fn, launches) for _ in range(a.windows))
            med[kernel] = us[len(us) // 2]
            print(json.dumps({"case": name, "kernel": kernel, "planes": planes, "H": H, "W": W, "bytes": nbytes[kernel],
                              "us_per_call_median": round(med[kernel], 2), "us_min": round(us[0], 2), "us_max": round(us[-1], 2),
                              "GB_per_s": round(nbytes[kernel] / med[kernel] / 1e3, 1), "calls_per_window": launches}), flush=True)
        torch.cuda.synchronize()
        diff = float((out_ms[:, 0, 0] - out_s).abs().max())
        value = float(M.combine(out_ms.cpu().numpy()).mean())
        print(json.dumps({"case": name, "msssim_over_ssim": round(med["evc_msssim_levels_f32"] / med["evc_ssim_planes_f32"], 3),
                          "max_abs_diff_level0_vs_ssim": diff, "ms_ssim_mean": round(value, 6)}), flush=True)


if __name__ == "__main__":
    main()
