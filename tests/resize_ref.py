"""numpy restatement of Pillow's 8-bit resize (PIL.Image.resize on 8 bits per channel) and of the reference's centre crop
(benchmark/fvd_utils/bench_uvg.py:577-598), as DESIGN.md section 8c states them: the checker of csrc/resample.hip.

Coefficients per axis, in Python floats, in this order of operations:
    scale = n_in / n_out; fs = max(scale, 1); support = filter_support * fs; ksize = int(ceil(support)) * 2 + 1
    per output xx: c = (xx + 0.5) * scale; xmin = max(int(c - support + 0.5), 0); n = min(int(c + support + 0.5), n_in) - xmin
                   w[x] = filter((x + xmin - c + 0.5) / fs), x < n; ww = the sum left to right; w[x] /= ww when ww != 0
    k[x] = int(w[x] * 2^22 + 0.5) for w[x] >= 0, else int(w[x] * 2^22 - 0.5)        (both truncate toward zero)
One pass: clamp((2^21 + sum_x src[xmin + x] * k[x]) >> 22, 0, 255) in int32, arithmetic shift.  Horizontal first, skipped when
n_out == n_in, rounded to uint8, then vertical, skipped likewise; with both skipped the output is a copy.
"""
import math

import numpy as np

PRECISION = 22
ALL = ("lanczos", "bicubic", "bilinear", "hamming", "box")
# case -> (frames, H, W, out_h, out_w, filters): the table of tests/golden/make_resize_golden.py
CASES = {
    "a": (2, 33, 47, 16, 16, ALL),
    "b": (2, 24, 40, 32, 32, ("lanczos", "bicubic")),
    "c": (1, 136, 240, 128, 128, ("lanczos",)),
    "d": (1, 270, 480, 16, 16, ("lanczos", "box")),
    "e": (1, 128, 160, 128, 128, ("lanczos",)),
    "f": (2, 40, 40, 20, 12, ("lanczos",)),
    "g": (1, 128, 128, 128, 128, ("lanczos",)),
}
KINDS = ("bytes", "binary")
FIXTURES = [(c, k, f) for c, v in CASES.items() for k in KINDS for f in v[5]]


def _sinc(v):
    return 1.0 if v == 0.0 else math.sin(math.pi * v) / (math.pi * v)


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x *= math.pi
    return math.sin(x) / x * (0.54 + 0.46 * math.cos(x))


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


FILTERS = {"lanczos": (_lanczos, 3.0), "bicubic": (_bicubic, 2.0), "bilinear": (_bilinear, 1.0), "hamming": (_hamming, 1.0),
           "box": (_box, 0.5)}


def tables(n_in, n_out, filter="lanczos"):
    """-> (bounds (n_out, 2) int32, coeffs (n_out, ksize) int32, zero past n, ksize)."""
    fn, fsupport = FILTERS[filter] if isinstance(filter, str) else filter
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fsupport * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    coeffs = np.zeros((n_out, ksize), dtype=np.int64)
    for xx in range(n_out):
        c = (xx + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        n = min(int(c + support + 0.5), n_in) - xmin
        w = [fn((x + xmin - c + 0.5) / fs) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, n)
        for x, v in enumerate(w):
            coeffs[xx, x] = int(v * (1 << PRECISION) + 0.5) if v >= 0 else int(v * (1 << PRECISION) - 0.5)
    return bounds, coeffs.astype(np.int32), ksize


def one_pass(src, bounds, coeffs, axis):
    """src: (..., rows, cols) uint8, filtered along ``axis`` (-1 or -2) -> uint8.  The sums are formed in int64 and must fit
    int32 (asserted): Pillow's accumulator is an int."""
    s = np.moveaxis(src.astype(np.int64), axis, -1)
    out = np.empty(s.shape[:-1] + (len(bounds),), dtype=np.uint8)
    for i, (xmin, n) in enumerate(bounds):
        acc = (1 << (PRECISION - 1)) + (s[..., xmin:xmin + n] * coeffs[i, :n].astype(np.int64)).sum(-1)
        assert np.abs(acc).max(initial=0) < 2 ** 31
        out[..., i] = np.clip(acc >> PRECISION, 0, 255)
    return np.moveaxis(out, -1, axis)


def resize(x, out_h, out_w, filter="lanczos"):
    """x: (..., H, W) uint8 -> (..., out_h, out_w) uint8."""
    H, W = x.shape[-2:]
    if out_w != W:
        b, k, _ = tables(W, out_w, filter)
        x = one_pass(x, b, k, -1)
    if out_h != H:
        b, k, _ = tables(H, out_h, filter)
        x = one_pass(x, b, k, -2)
    return np.array(x, dtype=np.uint8)


def center_box(H, W):
    """-> (r0, c0, h, w): rows H//2 - m//2 .. H//2 + m//2 and the same in columns, m = min(H, W); an odd m gives m - 1."""
    m = min(H, W)
    return H // 2 - m // 2, W // 2 - m // 2, 2 * (m // 2), 2 * (m // 2)


def crop(x, box):
    r0, c0, h, w = box
    return x[..., r0:r0 + h, c0:c0 + w]


def fit_box(x, out_h, out_w, filter="lanczos"):
    """centre crop + resize: what the reference's read_video does to a frame (there out_h = out_w = image_size)."""
    return resize(np.ascontiguousarray(crop(x, center_box(*x.shape[-2:]))), out_h, out_w, filter)
