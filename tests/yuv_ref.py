"""CPU restatement, in float64 numpy, of the colour conventions of csrc/yuv.hip, written from their
definition and not from the kernel; tests/test_yuv_host.py checks it against tests/golden/yuv_transform.npz, which the
reference's own functions produced.

    yuv420_to_rgb   up-sample the raw chroma samples x2, divide by maxv = 2^bits - 1, BT.709 full-range YCbCr -> RGB
    rgb_to_yuv420   RGB -> YCbCr, chroma = mean of each 2x2 block, sample = rint(clamp(v * maxv, 0, maxv)) (half to even)

Up-sampling by 2 with align_corners=False puts output i at source position (i + 0.5) / 2 - 0.5 = i/2 - 0.25: output 2c lies
3/4 of the way from sample c-1 to sample c, output 2c+1 a quarter past sample c.  Every mode is then a 4-tap filter over
samples c-2 .. c+1 (even outputs) or, mirrored, c-1 .. c+2 (odd outputs), with indices clamped to the plane:
nearest takes floor(i / 2) = c; bilinear weighs the two neighbours 1/4 : 3/4; bicubic is the cubic convolution kernel with
A = -0.75 evaluated at the distances 1.75, 0.75, 0.25, 1.25.
"""
import numpy as np

KR, KG, KB = 0.2126, 0.7152, 0.0722
FRAME_MARK = b"FRAME\n"


def cubic(x, a=-0.75):
    x = abs(x)
    if x <= 1:
        return ((a + 2) * x - (a + 3)) * x * x + 1
    return (((x - 5) * x + 8) * x - 4) * a


TAPS = {"nearest": (0.0, 0.0, 1.0, 0.0), "bilinear": (0.0, 0.25, 0.75, 0.0),
        "bicubic": (cubic(1.75), cubic(0.75), cubic(0.25), cubic(1.25))}


def upsample2_axis(p, mode, axis):
    """p: float64 array; doubles ``axis``."""
    w = TAPS[mode]
    n = p.shape[axis]
    c = np.arange(n)
    take = lambda i: np.take(p, np.clip(i, 0, n - 1), axis=axis)   # noqa: E731
    even = sum(w[k] * take(c - 2 + k) for k in range(4))
    odd = sum(w[3 - k] * take(c - 1 + k) for k in range(4))
    out = np.stack([even, odd], axis=axis + 1 if axis >= 0 else axis)
    shape = list(p.shape)
    shape[axis] = 2 * n
    return out.reshape(shape)


def upsample2(p, mode):
    """(..., h, w) -> (..., 2h, 2w)."""
    p = np.asarray(p, dtype=np.float64)
    return upsample2_axis(upsample2_axis(p, mode, p.ndim - 1), mode, p.ndim - 2)


def yuv420_to_rgb(y, u, v, bits=8, mode="bicubic"):
    """y: (N, H, W), u, v: (N, H/2, W/2) integer samples -> (N, 3, H, W) float64, unclamped."""
    maxv = float(2 ** bits - 1)
    Y = np.asarray(y, dtype=np.float64) / maxv
    cb = upsample2(u, mode) / maxv - 0.5
    cr = upsample2(v, mode) / maxv - 0.5
    r = Y + (2 - 2 * KR) * cr
    b = Y + (2 - 2 * KB) * cb
    g = (Y - KR * r - KB * b) / KG
    return np.stack([r, g, b], axis=1)


def ycbcr420(rgb):
    """rgb: (N, 3, H, W) -> (y (N, H, W), cb, cr (N, H/2, W/2)) float64 in [0, 1] units, before scaling and rounding."""
    rgb = np.asarray(rgb, dtype=np.float64)
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    y = KR * r + KG * g + KB * b
    cb = 0.5 * (b - y) / (1 - KB) + 0.5
    cr = 0.5 * (r - y) / (1 - KR) + 0.5
    pool = lambda p: p.reshape(p.shape[0], p.shape[1] // 2, 2, p.shape[2] // 2, 2).mean(axis=(2, 4))   # noqa: E731
    return y, pool(cb), pool(cr)


def to_codes(v, maxv):
    """rint(clamp(v * maxv, 0, maxv)), ties to even -> (codes int64, pre-rounding values)."""
    pre = np.clip(np.asarray(v, dtype=np.float64) * maxv, 0, maxv)
    return np.rint(pre).astype(np.int64), pre


def tie_band(pre, delta):
    """True where a pre-rounding value lies within ``delta`` of a rounding tie (k + 0.5)."""
    return np.abs(np.abs(pre - np.floor(pre) - 0.5)) <= delta


def rgb_to_yuv420(rgb, bits=8):
    """-> ((y, u, v) codes, (y, u, v) pre-rounding values)."""
    maxv = float(2 ** bits - 1)
    pairs = [to_codes(p, maxv) for p in ycbcr420(rgb)]
    return tuple(c for c, _ in pairs), tuple(p for _, p in pairs)


def rgb_u8(rgb):
    """The uint8 form: rint(clamp(rgb * 255, 0, 255)) -> (codes, pre-rounding values)."""
    return to_codes(rgb, 255.0)


# ---- buffers ----------------------------------------------------------------------------------------------------------

def frame_buffer(y, u, v, bits=8, lead=b"", marker=b""):
    """Planes of N frames -> (bytes, first, stride): ``lead``, then per frame ``marker`` + Y + U + V -- a Y4M file is
    lead = header line, marker = FRAME_MARK; a raw file has neither."""
    dt = np.dtype("<u2") if bits > 8 else np.dtype(np.uint8)
    frames = [marker + b"".join(np.ascontiguousarray(p[n], dtype=dt).tobytes() for p in (y, u, v)) for n in range(len(y))]
    return lead + b"".join(frames), len(lead) + len(marker), len(frames[0])


def split_buffer(buf, N, H, W, bits=8, first=0, stride=None):
    """The inverse: bytes -> (y, u, v) integer planes of N frames."""
    dt = np.dtype("<u2") if bits > 8 else np.dtype(np.uint8)
    fb = H * W * dt.itemsize * 3 // 2
    stride = fb if stride is None else stride
    ys, us, vs = [], [], []
    for n in range(N):
        s = np.frombuffer(bytes(buf[first + n * stride:first + n * stride + fb]), dtype=dt).astype(np.int64)
        ys.append(s[:H * W].reshape(H, W))
        us.append(s[H * W:H * W * 5 // 4].reshape(H // 2, W // 2))
        vs.append(s[H * W * 5 // 4:].reshape(H // 2, W // 2))
    return np.stack(ys), np.stack(us), np.stack(vs)


def smooth_clip(N, H, W, seed=0):
    """A smooth seeded RGB clip in [0, 1], float32 (N, 3, H, W): a few low-frequency waves per channel, drifting over frames."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H) / max(H, 1), np.arange(W) / max(W, 1), indexing="ij")
    out = np.zeros((N, 3, H, W))
    for c in range(3):
        for _ in range(3):
            fy, fx, ph, dr = rng.uniform(0.3, 2.5), rng.uniform(0.3, 2.5), rng.uniform(0, 6.28), rng.uniform(0.1, 0.6)
            for n in range(N):
                out[n, c] += np.sin(6.283185307179586 * (fy * yy + fx * xx) + ph + dr * n)
    return (0.5 + out / 6.5).clip(0, 1).astype(np.float32)
