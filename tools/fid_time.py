"""Time the FID feature network of evc_amd/fid.py (csrc/inception.hip + the convolutions) and the two set kernels of precision /
recall, on seeded stand-in weights (the timing does not depend on the weight values).

Per batch size: ms per frame of ``InceptionV3.forward`` on 128x128 frames, the FLOP count of the forward taken from the layer
shapes (``fid.flops_per_image``: 2 FLOP per MAC of every convolution at 299 x 299; the pools, the resize and the im2col copies
are not counted) and the TFLOP/s that gives.  Then ``evc_knn_radius_f32`` and ``evc_manifold_hits_f32`` at n = m = 30 and
2 000 rows of 2 048 features, with the bytes an ideal pass would read (each set once) and the fp64 FLOP they execute
(3 per feature pair: subtract, multiply, add).  HIP events around back-to-back calls after a warm-up, several windows.

    python tools/fid_time.py [--batches 1 8 30] [--size 128] [--launches 5] [--windows 5]
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
from evc_amd import fid, lib as L  # noqa: E402
import fid_recipe as R  # noqa: E402  (the seeded stand-in state dict)


def window(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches       # milliseconds per call


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--batches", type=int, nargs="+", default=[1, 8, 30])
    p.add_argument("--size", type=int, default=128)
    p.add_argument("--launches", type=int, default=5)
    p.add_argument("--windows", type=int, default=5)
    a = p.parse_args()
    L.hip_lib()
    flops = fid.flops_per_image()
    print(json.dumps(dict(case="forward", flops_per_frame=flops, convolutions=len(fid.conv_specs()),
                          arithmetic={L.ARITH_F32: "f32", L.ARITH_BF16X6: "bf16x6"}.get(L.default_arith()))), flush=True)
    net = fid.InceptionV3(R.seeded_state_dict(), max_images=max(a.batches))
    g = torch.Generator().manual_seed(1)
    for B in a.batches:
        x = torch.rand((B, 3, a.size, a.size), generator=g).cuda()
        fn = lambda: net.forward(x)                                               # noqa: E731
        window(fn, 2)
        ms = sorted(window(fn, a.launches) for _ in range(a.windows))
        med = ms[len(ms) // 2]
        print(json.dumps(dict(case=f"forward B={B} {a.size}x{a.size}", ms_per_forward_median=round(med, 3), ms_min=round(ms[0], 3),
                              ms_max=round(ms[-1], 3), ms_per_frame=round(med / B, 3), flops=flops * B,
                              tflops=round(flops * B / med / 1e9, 2), forwards_per_window=a.launches)), flush=True)
    d = 2048
    for n in (30, 2000):
        rng = np.random.default_rng(n)
        real = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).cuda()
        gen = torch.from_numpy((0.9 * rng.standard_normal((n, d)) + 0.1).astype(np.float32)).cuda()
        r2 = L.knn_radius(real, 3)
        cases = {"evc_knn_radius_f32 k=3": lambda: L.knn_radius(real, 3), "evc_manifold_hits_f32": lambda: L.manifold_hits(gen, real, r2)}
        launches = max(a.launches, 200 if n <= 100 else 5)
        for name, fn in cases.items():
            window(fn, 2)
            ms = sorted(window(fn, launches) for _ in range(a.windows))
            med = ms[len(ms) // 2]
            nbytes = (1 if "knn" in name else 2) * n * d * 4
            print(json.dumps(dict(case=f"n = m = {n}, d = {d}", kernel=name, us_per_call_median=round(med * 1e3, 2),
                                  us_min=round(ms[0] * 1e3, 2), us_max=round(ms[-1] * 1e3, 2), calls_per_window=launches,
                                  ideal_bytes=nbytes, fp64_flops=3.0 * n * n * d,
                                  fp64_gflops=round(3.0 * n * n * d / med / 1e6, 1))), flush=True)
        p_r = fid.precision_recall(real.cpu().numpy(), gen.cpu().numpy(), k=3)
        print(json.dumps(dict(case=f"n = m = {n}, d = {d}", precision=p_r[0], recall=p_r[1])), flush=True)


if __name__ == "__main__":
    main()
