"""Time the two kernels of csrc/resample.hip on one 30-frame clip, 1920x1080 -> 128 and 352x288 -> 128 (centre crop, lanczos):
HIP events around back-to-back launches after a warm-up, several windows, with the bytes each launch has to move beside the
time -- the crop read once and the result written once; the pair counts its intermediate once each way.  Where Pillow is
installed the same clip is also resized on the host cores (one thread per core this process may use), as the baseline.

    python tools/resize_time.py [--frames 30] [--size 128] [--filter lanczos] [--launches 200] [--windows 5] [--no-pillow]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import evc_amd  # noqa: E402,F401
from evc_amd import lib as L, video_io as V  # noqa: E402


def window(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches       # microseconds per launch


def pillow_seconds(x, box, size, name, threads):
    from PIL import Image
    filters = {"lanczos": Image.LANCZOS, "bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR, "hamming": Image.HAMMING, "box": Image.BOX}
    r0, c0, h, w = box
    images = [Image.fromarray(np.ascontiguousarray(f[:, r0:r0 + h, c0:c0 + w].transpose(1, 2, 0))) for f in x]
    best = None
    with ThreadPoolExecutor(threads) as ex:
        for _ in range(3):
            t = time.perf_counter()
            out = list(ex.map(lambda im: im.resize((size, size), filters[name]), images))
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
    return best, np.stack([np.asarray(o) for o in out]).transpose(0, 3, 1, 2)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frames", type=int, default=30)
    p.add_argument("--size", type=int, default=128)
    p.add_argument("--filter", default="lanczos", choices=sorted(L.RESAMPLE_FILTERS))
    p.add_argument("--launches", type=int, default=200)
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--no-pillow", action="store_true")
    a = p.parse_args()
    so = L.hip_lib()
    T, S = a.frames, a.size
    for H, W in ((1080, 1920), (288, 352)):
        x = torch.from_numpy(np.random.default_rng(H).integers(0, 256, (T, 3, H, W), dtype=np.uint8)).cuda()
        r0, c0, h, w = box = V.center_box(H, W)
        bh, kh, ksh = L._resample_device_tables(w, S, a.filter, x.device)
        bv, kv, ksv = L._resample_device_tables(h, S, a.filter, x.device)
        mid = torch.empty((T, 3, h, S), dtype=torch.uint8, device="cuda")
        out = torch.empty((T, 3, S, S), dtype=torch.uint8, device="cuda")
        src = x.data_ptr() + r0 * W + c0

        def hpass():
            L._check(so.evc_resample_h_u8(src, 3 * T, h, w, H * W, W, L.ptr(bh), L.ptr(kh), ksh, S, L.ptr(mid), L.stream_ptr()), "h")

        def vpass():
            L._check(so.evc_resample_v_u8(mid.data_ptr(), 3 * T, h, S, h * S, S, L.ptr(bv), L.ptr(kv), ksv, S, L.ptr(out), L.stream_ptr()), "v")
        crop, inter, res = 3 * T * h * w, mid.numel(), out.numel()
        cases = {"horizontal": (hpass, crop + inter), "vertical": (vpass, inter + res),
                 "pair (lib.resample_u8)": (lambda: L.resample_u8(x, S, S, a.filter, box=box), crop + 2 * inter + res)}
        for name, (fn, nbytes) in cases.items():
            window(fn, 20)                              # warm-up: code object load, clocks
            us = sorted(window(fn, a.launches) for _ in range(a.windows))
            print(json.dumps({"kernel": name, "source": f"{W}x{H}", "crop": f"{w}x{h}", "size": S, "filter": a.filter, "frames": T,
                              "ksize": [ksh, ksv], "bytes": nbytes, "us_per_launch_median": round(us[len(us) // 2], 2), "us_min": round(us[0], 2),
                              "us_max": round(us[-1], 2), "GB_per_s": round(nbytes / us[len(us) // 2] / 1e3, 1),
                              "launches_per_window": a.launches}), flush=True)
        if not a.no_pillow:
            try:
                import PIL
            except ImportError:
                print(json.dumps({"pillow": "not installed"}), flush=True)
                continue
            threads = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
            threads = max(1, min(threads, int(os.environ.get("OMP_NUM_THREADS", threads)), T))
            sec, ref = pillow_seconds(x.cpu().numpy(), box, S, a.filter, threads)
            same = bool(np.array_equal(L.resample_u8(x, S, S, a.filter, box=box).cpu().numpy(), ref))
            print(json.dumps({"pillow": PIL.__version__, "source": f"{W}x{H}", "threads": threads, "ms_per_clip_best_of_3": round(sec * 1e3, 2),
                              "same_bytes_as_the_gpu": same}), flush=True)


if __name__ == "__main__":
    main()
