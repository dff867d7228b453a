"""Writes tests/golden/resize_pillow.npz: seeded uint8 frames and what Pillow makes of them -- the reference's read_video
(benchmark/fvd_utils/bench_uvg.py:577-598): centre crop, then PIL.Image.resize(..., filter).  Needs Pillow; the version that
wrote the file is recorded in it (``pillow_version``).

    python tests/golden/make_resize_golden.py

Keys: in_<case>_<kind> (N, 3, H, W) uint8, out_<case>_<kind>_<filter> (N, 3, out_h, out_w) uint8, size_<case> (out_h, out_w).
Every case comes as random bytes (``bytes``) and as random 0 / 255 (``binary``: both clip ends occur in Pillow's output).
"""
import os

import numpy as np
import PIL
from PIL import Image

ALL = ("lanczos", "bicubic", "bilinear", "hamming", "box")
# case -> (frames, H, W, out_h, out_w, filters)
CASES = {
    "a": (2, 33, 47, 16, 16, ALL),                        # odd sizes: crop 32x32 at (0, 7), unaligned head
    "b": (2, 24, 40, 32, 32, ("lanczos", "bicubic")),     # up-scaling, fs = 1
    "c": (1, 136, 240, 128, 128, ("lanczos",)),           # scale 1.0625, ksize 9, many clamped xmin
    "d": (1, 270, 480, 16, 16, ("lanczos", "box")),       # scale 16.875, ksize 103: the long tap loop
    "e": (1, 128, 160, 128, 128, ("lanczos",)),           # crop only: both passes skipped
    "f": (2, 40, 40, 20, 12, ("lanczos",)),               # both passes, different tables per axis
    "g": (1, 128, 128, 128, 128, ("lanczos",)),           # identity
}
KINDS = ("bytes", "binary")
PIL_FILTERS = {"lanczos": Image.LANCZOS, "bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR, "hamming": Image.HAMMING,
               "box": Image.BOX}


def center_crop(image):
    h, w, _ = image.shape
    m = min(h, w)
    return image[h // 2 - m // 2:h // 2 + m // 2, w // 2 - m // 2:w // 2 + m // 2, :]


def frames_of(case, kind):
    n, H, W = CASES[case][:3]
    rng = np.random.default_rng([ord(case), KINDS.index(kind)])
    x = rng.integers(0, 256, (n, 3, H, W), dtype=np.uint8)
    return x if kind == "bytes" else np.where(x < 128, 0, 255).astype(np.uint8)


def pillow_fit(x, out_h, out_w, filter):
    out = [np.array(Image.fromarray(np.ascontiguousarray(center_crop(f.transpose(1, 2, 0)))).resize((out_w, out_h), PIL_FILTERS[filter]))
           for f in x]
    return np.stack(out).transpose(0, 3, 1, 2)


def main():
    blob = {"pillow_version": np.array(PIL.__version__)}
    for case, (_, _, _, oh, ow, filters) in CASES.items():
        blob[f"size_{case}"] = np.array([oh, ow], dtype=np.int32)
        for kind in KINDS:
            x = frames_of(case, kind)
            blob[f"in_{case}_{kind}"] = x
            for f in filters:
                blob[f"out_{case}_{kind}_{f}"] = np.ascontiguousarray(pillow_fit(x, oh, ow, f))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "resize_pillow.npz")
    np.savez_compressed(path, **blob)
    outs = np.concatenate([v.ravel() for k, v in blob.items() if k.startswith("out_") and "_binary_" in k])
    print(f"{path}: {os.path.getsize(path)} bytes, Pillow {PIL.__version__}; outputs of the 0/255 inputs: "
          f"{(outs == 0).mean():.1%} zeros, {(outs == 255).mean():.1%} 255")


if __name__ == "__main__":
    main()
