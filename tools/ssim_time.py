"""Time the SSIM kernel of csrc/ssim.hip on one clip (30 frames of 128x128 = 90 planes) and on a 32-job batch (2 880 planes):
HIP events around back-to-back launches after a warm-up, several windows, with the bytes each call moves counted from the
shapes (both inputs read once, one double per tile written and read, one double per plane written).  Beside it the time of
the same metric restated with torch float64 conv2d on the same device, and the largest difference between the two.

    python tools/ssim_time.py [--size 128] [--launches 500] [--windows 5]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import evc_amd  # noqa: E402,F401
from evc_amd import lib as L, ssim as S  # noqa: E402


def window(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches       # microseconds per call


def torch_f64(a, b, k2d):
    """The metric with torch: five float64 conv2d over the widened planes, the map, its mean.  a, b: (N, H, W) float32."""
    x1, x2 = a.double()[:, None], b.double()[:, None]
    f = lambda t: F.conv2d(t, k2d)      # noqa: E731
    mu1, mu2 = f(x1), f(x2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = f(x1 * x1) - mu1_sq, f(x2 * x2) - mu2_sq, f(x1 * x2) - mu1_mu2
    m = ((2 * mu1_mu2 + S.C1) * (2 * s12 + S.C2)) / ((mu1_sq + mu2_sq + S.C1) * (s1 + s2 + S.C2))
    return m.mean(dim=(1, 2, 3))


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--size", type=int, default=128)
    p.add_argument("--launches", type=int, default=500)
    p.add_argument("--windows", type=int, default=5)
    a = p.parse_args()
    so = L.hip_lib()
    taps = torch.from_numpy(S.gaussian_taps()).cuda()
    k2d = torch.outer(taps, taps)[None, None]
    for name, planes in (("one clip (30 frames x 3)", 90), ("32 jobs (32 x 30 frames x 3)", 2880)):
        x = torch.rand((planes, a.size, a.size), device="cuda")
        y = (x + 0.05 * torch.randn_like(x)).clamp_(0, 1)
        out = torch.empty(planes, dtype=torch.float64, device="cuda")
        ws_bytes = so.evc_ssim_workspace_bytes(planes, a.size, a.size)
        nbytes = 2 * x.numel() * 4 + 2 * ws_bytes + planes * 8
        cases = {"evc_ssim_planes_f32": (lambda: L.ssim_planes(x, y, taps, S.C1, S.C2, out=out), max(50, a.launches)),
                 "torch float64 conv2d": (lambda: torch_f64(x, y, k2d), max(5, a.launches // 25))}
        try:
            diff = float((L.ssim_planes(x, y, taps, S.C1, S.C2) - torch_f64(x, y, k2d)).abs().max())
        except RuntimeError as e:           # a torch build without a float64 convolution on this device: time the kernel alone
            print(json.dumps({"case": name, "kernel": "torch float64 conv2d", "error": str(e).splitlines()[0]}), flush=True)
            diff = None
            del cases["torch float64 conv2d"]
        for kernel, (fn, launches) in cases.items():
            window(fn, max(3, launches // 10))                      # warm-up: code object load, clocks, allocator
            us = sorted(window(fn, launches) for _ in range(a.windows))
            print(json.dumps({"case": name, "kernel": kernel, "planes": planes, "size": a.size, "bytes": nbytes,
                              "us_per_call_median": round(us[len(us) // 2], 3), "us_min": round(us[0], 3), "us_max": round(us[-1], 3),
                              "GB_per_s": round(nbytes / us[len(us) // 2] / 1e3, 1), "calls_per_window": launches,
                              "max_abs_diff_kernel_vs_torch": diff}), flush=True)


if __name__ == "__main__":
    main()
