#!/usr/bin/env python3
"""Generate tests/golden/yuv_transform.npz by running the REFERENCE's own colour transforms in float64 on the CPU.

Runs only where the reference is present (its root is the first argument, default /root/reference).  Nothing from the
reference is copied: this script imports benchmark/transform.py (torch only) and evaluates

    ycbcr2rgb(yuv_420_to_444((y, u, v), mode).true_divide(maxv))        benchmark/fvd_utils/bench_uvg.py:479
    yuv_444_to_420(rgb2ycbcr(rgb)), then rint(clamp(v * maxv, 0, maxv))

on seeded inputs, and stores inputs and results only.

Shapes (H x W): 2x2 (chroma 1x1: every tap clamps onto one sample), 12x16, 18x34 (no multiple of any vector width), 32x48; two
frames each; bit depths 8 and 10; nearest, bilinear, bicubic.

Stored, per shape HxW and bit depth b:
    yuv_{y,u,v}_HxW_b         seeded random samples in 0 .. 2^b - 1 (uint16)
    rgb_<mode>_HxW_b          the float64 result r as q = rint((r + OFFSET) / GRID), OFFSET = 1.5, GRID = 2^-22, in three byte
                              planes (3, N, 3, H, W): q = b[0] + 256 b[1] + 65536 b[2].  Every result lies in -1.5 .. 2.5, so q
                              fits 24 bits; float64 itself would not fit the fixture's size limit.  The rounding, at most
                              GRID / 2 = 1.2e-7, is taken off the 2e-6 bar by the GPU test
    rgbk_<clip>_HxW           RGB inputs as uint8 codes k, clip = random | smooth; the input is float32(k) / float32(255)
    code_{y,u,v}_<clip>_HxW_b the 4:2:0 sample codes (uint16)
    band_{y,u,v}_<clip>_HxW_b True where the float64 pre-rounding value is within DELTA = maxv * 1e-6 code units of a rounding tie
The uint8 form of the first transform is rint(clamp(rgb * 255, 0, 255)) of the stored result (the GRID rounding is 3.1e-5 code
units, which the test takes off that form's DELTA), so it is not stored twice.  The script asserts, for every case it stores, that at
most 1 % of the samples lie in the tie band, and that tests/yuv_ref.py computes what the reference computes.

    python tests/golden/make_yuv_golden.py [reference root]
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import yuv_ref as YR  # noqa: E402

SHAPES = [(2, 2), (12, 16), (18, 34), (32, 48)]
FRAMES = 2
BITS = (8, 10)
MODES = ("nearest", "bilinear", "bicubic")
GRID = 2.0 ** -22
OFFSET = 1.5
BAND_LIMIT = 0.01


def load_reference(root):
    spec = importlib.util.spec_from_file_location("ref_transform", os.path.join(root, "benchmark", "transform.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def check_band(name, bands):
    n = sum(b.size for b in bands)
    k = sum(int(b.sum()) for b in bands)
    assert k <= BAND_LIMIT * n, f"{name}: {k} of {n} samples within the tie band (> 1 %)"
    return k / n


def main():
    T = load_reference(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
    rng = np.random.default_rng(20240607)
    out, worst_ref, worst_band = {}, 0.0, 0.0
    for H, W in SHAPES:
        tag = f"{H}x{W}"
        for bits in BITS:
            maxv = 2 ** bits - 1
            y = rng.integers(0, maxv + 1, (FRAMES, H, W)).astype(np.uint16)
            u = rng.integers(0, maxv + 1, (FRAMES, H // 2, W // 2)).astype(np.uint16)
            v = rng.integers(0, maxv + 1, (FRAMES, H // 2, W // 2)).astype(np.uint16)
            out[f"yuv_y_{tag}_{bits}"], out[f"yuv_u_{tag}_{bits}"], out[f"yuv_v_{tag}_{bits}"] = y, u, v
            planes = tuple(torch.from_numpy(p.astype(np.float64)).unsqueeze(1) for p in (y, u, v))
            for mode in MODES:
                rgb = T.ycbcr2rgb(T.yuv_420_to_444(planes, mode=mode).true_divide(maxv)).numpy()
                assert rgb.dtype == np.float64 and rgb.shape == (FRAMES, 3, H, W)
                worst_ref = max(worst_ref, float(np.abs(rgb - YR.yuv420_to_rgb(y, u, v, bits, mode)).max()))
                q = np.rint((rgb + OFFSET) / GRID).astype(np.int64)
                assert q.min() >= 0 and q.max() < 2 ** 24
                out[f"rgb_{mode}_{tag}_{bits}"] = np.stack([(q >> s) & 255 for s in (0, 8, 16)]).astype(np.uint8)
                _, pre = YR.rgb_u8(q * GRID - OFFSET)
                worst_band = max(worst_band, check_band(f"rgb_{mode}_{tag}_{bits} (uint8 form)", [YR.tie_band(pre, 255e-6)]))
        clips = {"random": rng.integers(0, 256, (FRAMES, 3, H, W)).astype(np.uint8),
                 "smooth": np.rint(YR.smooth_clip(FRAMES, H, W, seed=H * W).astype(np.float64) * 255).astype(np.uint8)}
        for clip, k in clips.items():
            out[f"rgbk_{clip}_{tag}"] = k
            x = torch.from_numpy((k.astype(np.float32) / np.float32(255)).astype(np.float64))
            ycc = T.yuv_444_to_420(T.rgb2ycbcr(x))
            for bits in BITS:
                maxv = 2 ** bits - 1
                (ry, ru, rv), _ = YR.rgb_to_yuv420(x.numpy(), bits)
                bands = []
                for name, p, mine in zip("yuv", ycc, (ry, ru, rv)):
                    pre = (p[:, 0] * maxv).clamp(0, maxv)
                    code = pre.round().numpy().astype(np.int64)            # torch.round: half to even
                    band = YR.tie_band(pre.numpy(), maxv * 1e-6)
                    assert (np.abs(code - mine) <= band).all(), "tests/yuv_ref.py disagrees with the reference away from ties"
                    out[f"code_{name}_{clip}_{tag}_{bits}"] = code.astype(np.uint16)
                    out[f"band_{name}_{clip}_{tag}_{bits}"] = band
                    bands.append(band)
                worst_band = max(worst_band, check_band(f"codes {clip} {tag} {bits}-bit", bands))
    assert worst_ref < 1e-13, worst_ref
    path = os.path.join(HERE, "yuv_transform.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 400 * 1024, size
    print(f"wrote {path}: {len(out)} arrays, {size} bytes; restatement vs reference (float64): {worst_ref:.2e}; "
          f"largest tie-band share of a case: {100 * worst_band:.3f} %")


if __name__ == "__main__":
    main()
