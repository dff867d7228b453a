"""numpy restatement of the whole-frame tiling (DESIGN.md section 8c "Whole frames"): the grid of video_io.tile_axis /
tile_grid, the gather of evc_tile_gather_u8 and the blend of evc_tile_blend_f32.  The reference has no counterpart, so this
file is the yardstick, and the definitions are such that the kernels reproduce it bit for bit.

The blend is float32 in the order the kernel takes: per output pixel, the tiles that cover it in ascending tile index,
acc = acc + float32(t(ly) t(lx)) * v with the product rounded before the sum (numpy evaluates the two array operations one
after the other, so nothing is fused), the weights summed as integers, one float32 division at the end.  A tile adds to the
pixels it covers and to no others, so a pixel no further tile covers keeps its value exactly."""
import numpy as np

# (H, W, O, S) of tests/test_gpu_tile.py, with what each one exercises
GEOMETRIES = [
    (40, 70, 8, 32),         # general case, unaligned column origins 0, 19, 38
    (33, 32, 8, 32),         # odd height, row origins 0, 1; a single column
    (20, 50, 0, 32),         # an axis shorter than S: edge replication in the gather, ignored by the blend
    (64, 96, 0, 32),         # abutting tiles, every pixel covered once
    (61, 35, 4, 32),         # a pixel covered by three tiles along the rows; odd width: no 16-byte path
    (144, 160, 16, 128),     # the command-line test's own grid
]
# further paths of the kernels: S = 2 is no multiple of 16 (the gather's byte kernel) and smaller than a thread's 4 pixels (a
# group spans two tiles); 1026 column origins are more than a blend workgroup stages in LDS; a row takes three workgroups
EXTRA_GEOMETRIES = [
    (2, 2052, 0, 2),
    (5, 1031, 2, 6),         # the same with an odd width, overlap and a short last workgroup of single pixels
]


def axis(L, S, O):
    """Origins of the tiles of one axis: [0] for L <= S, else n = ceil((L - O) / (S - O)) origins (k (L - S)) // (n - 1)."""
    assert L >= 1 and S >= 1 and 0 <= 2 * O <= S
    if L <= S:
        return [0]
    P = S - O
    n = -(-(L - O) // P)
    return [(k * (L - S)) // (n - 1) for k in range(n)]


def grid(H, W, S, O):
    return axis(H, S, O), axis(W, S, O)


def tent(S):
    i = np.arange(S, dtype=np.int64)
    return np.minimum(i + 1, S - i)


def gather(x, S, oy, ox):
    """x: (N, C, H, W) -> (ny * nx, N, C, S, S): tile ty * nx + tx holds x[n][c][min(oy[ty] + y, H - 1)][min(ox[tx] + x, W - 1)]."""
    N, C, H, W = x.shape
    out = np.empty((len(oy) * len(ox), N, C, S, S), dtype=x.dtype)
    for a, y0 in enumerate(oy):
        rows = np.minimum(np.arange(y0, y0 + S), H - 1)
        for b, x0 in enumerate(ox):
            cols = np.minimum(np.arange(x0, x0 + S), W - 1)
            out[a * len(ox) + b] = x[:, :, rows][:, :, :, cols]
    return out


def blend(tiles, H, W, oy, ox):
    """tiles: (ny * nx, N, C, S, S) float32 -> (N, C, H, W) float32."""
    tiles = np.asarray(tiles)
    assert tiles.dtype == np.float32 and tiles.shape[0] == len(oy) * len(ox)
    _, N, C, S, _ = tiles.shape
    t = tent(S)
    acc = np.zeros((N, C, H, W), dtype=np.float32)
    den = np.zeros((H, W), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for a, y0 in enumerate(oy):
            for b, x0 in enumerate(ox):
                h, w = min(S, H - y0), min(S, W - x0)           # the padding samples of a short axis take no part
                weight = t[:h, None] * t[None, :w]              # integers
                prod = weight.astype(np.float32) * tiles[a * len(ox) + b][:, :, :h, :w]      # rounded to float32
                acc[:, :, y0:y0 + h, x0:x0 + w] = acc[:, :, y0:y0 + h, x0:x0 + w] + prod     # then the sum is rounded
                den[y0:y0 + h, x0:x0 + w] += weight
        assert den.min() > 0, "the origins leave a pixel uncovered"
        return acc / den.astype(np.float32)


def cover_counts(L, S, origins):
    """How many tiles cover each sample of an axis."""
    n = np.zeros(L, dtype=np.int64)
    for o in origins:
        n[o:min(o + S, L)] += 1
    return n
