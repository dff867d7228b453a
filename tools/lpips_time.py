"""Time the LPIPS family of evc_amd/lpips.py (csrc/lpips.hip) on one 30-frame 128x128 clip: each network (alex, vgg, squeeze) as
distances and as the spatial mean the benchmark reports, on seeded stand-in backbones (the timing does not depend on the weight
values).  And the head alone: ``evc_lpips_map_f32`` + ``evc_lpips_map_mean_f32`` against the one-workgroup-per-pair
``evc_lpips_layer_f32`` on the same tensors, at N = 30 with (HW, C) = (128^2, 64) -- VGG's first tap -- and (31^2, 64) -- AlexNet's.
HIP events around back-to-back calls after a warm-up, several windows, the two heads alternating; bytes counted from the shapes
(both feature tensors read once; the map written and read once by the new head).

    python tools/lpips_time.py [--frames 30] [--size 128] [--launches 200] [--windows 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import evc_amd  # noqa: E402,F401
from evc_amd import lib as L  # noqa: E402
from evc_amd.lpips import NETS, Lpips, LpipsAlex  # noqa: E402
import lpips_ref as R  # noqa: E402  (the seeded stand-in state dicts)


def window(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches       # microseconds per call


def report(case, kernel, us, launches, **more):
    us = sorted(us)
    print(json.dumps(dict(case=case, kernel=kernel, us_per_call_median=round(us[len(us) // 2], 2), us_min=round(us[0], 2),
                          us_max=round(us[-1], 2), calls_per_window=launches, **more)), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frames", type=int, default=30)
    p.add_argument("--size", type=int, default=128)
    p.add_argument("--launches", type=int, default=200)
    p.add_argument("--windows", type=int, default=5)
    a = p.parse_args()
    L.hip_lib()
    N = a.frames

    # ---- the head alone, old and new alternating in one process ----
    for HW, C in ((a.size * a.size, 64), (31 * 31, 64)):
        f0 = torch.relu(torch.randn((N, HW, 1, C), device="cuda"))
        f1 = torch.relu(f0 + 0.1 * torch.randn_like(f0))
        w = torch.rand(C, device="cuda") / C
        d_old, d_new = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
        m = torch.empty((N, HW, 1), device="cuda")
        old = lambda: L.lpips_layer(f0, f1, w, d_old, False)                                          # noqa: E731
        new = lambda: L.lpips_map_mean(L.lpips_map(f0, f1, w, out=m), d_new, False)                   # noqa: E731
        only_map = lambda: L.lpips_map(f0, f1, w, out=m)                                              # noqa: E731
        old(), new()
        diff = float(((d_old - d_new).abs() / d_old).max())
        launches = max(20, a.launches if HW < 4096 else a.launches // 2)
        times = {"old": [], "new": [], "map": []}
        for fn in (old, new, only_map):
            window(fn, max(3, launches // 10))
        for _ in range(a.windows):
            times["old"].append(window(old, launches))
            times["new"].append(window(new, launches))
            times["map"].append(window(only_map, launches))
        nbytes = 2 * N * HW * C * 4
        case = f"head N={N} HW={HW} C={C}"
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        report(case, "evc_lpips_layer_f32", times["old"], launches, bytes=nbytes, GB_per_s=round(nbytes / med["old"] / 1e3, 1))
        report(case, "evc_lpips_map_f32 + evc_lpips_map_mean_f32", times["new"], launches, bytes=nbytes + 2 * N * HW * 4,
               GB_per_s=round((nbytes + 2 * N * HW * 4) / med["new"] / 1e3, 1), old_over_new=round(med["old"] / med["new"], 2),
               max_rel_diff_old_vs_new=diff)
        report(case, "evc_lpips_map_f32", times["map"], launches, bytes=nbytes + N * HW * 4,
               GB_per_s=round((nbytes + N * HW * 4) / med["map"] / 1e3, 1))

    # ---- the networks on one clip ----
    g = torch.Generator().manual_seed(1)
    x = torch.rand((N, 3, a.size, a.size), generator=g).cuda()
    y = (x + 0.1 * torch.randn(x.shape, generator=g).cuda()).clamp(0, 1)
    for net_name in NETS:
        sd = R.seeded_state_dict(net_name, 7)
        net = Lpips(net_name, sd)
        cases = {"distance": lambda: net(x, y), "spatial mean (normalize=True)": lambda: net.spatial_mean(x, y)}
        if net_name == "alex":
            older = LpipsAlex(sd)
            cases["LpipsAlex distance (evc_lpips_layer_f32 head)"] = lambda: older(x, y)
        launches = max(5, a.launches // 20)
        for fn in cases.values():
            window(fn, 2)
        times = {k: [] for k in cases}
        for _ in range(a.windows):
            for k, fn in cases.items():
                times[k].append(window(fn, launches))
        for k, v in times.items():
            report(f"{net_name} {N} frames {a.size}x{a.size}", k, v, launches, mean_value=float(np.mean(cases[k]().cpu().numpy())))


if __name__ == "__main__":
    main()
