"""Float64 yardstick of MS-SSIM, restated from the definition of ``pytorch_msssim.ms_ssim`` (the library is not installed
here): data_range 1, win_size 11, win_sigma 1.5, K = (0.01, 0.03), on float32 inputs widened to float64.  Per level the maps
    cs = (2 s12 + C2) / (s1 + s2 + C2),   ssim = ((2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1)) * cs,   s = E[.] - mu mu
over the valid region of the Gaussian window and their means; between levels ``avg_pool2d(kernel 2, stride 2, padding =
size % 2)`` of both planes; the value prod_{l < L-1} relu(cs_l)^w_l * relu(ssim_{L-1})^w_{L-1}; a frame's value is the mean of
its channels'.

Two independent forms: "full" filters with the 121-tap ``scipy.signal.correlate2d`` and pools with torch's own
``F.avg_pool2d``; "separable" filters 11 taps along rows, then columns, and pools by hand over a plane with one zero row /
column put in front of an odd axis.  They differ by summation order only."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import ssim_ref as S

C1, C2 = S.C1, S.C2
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
KINDS, content = S.KINDS, S.content

SHAPES5 = [(161, 161), (162, 177), (176, 208), (271, 165)]      # the smallest legal frame (161 -> 81 -> 41 -> 21 -> 11: a 1x1 last
                                                                # map), odd sizes at every level, several tiles per level
SMALL = [(1, (11, 12)), (2, (21, 23)), (3, (41, 45))]           # (levels, shape), with the first L standard weights


def pool_torch(x):
    H, W = x.shape
    return F.avg_pool2d(torch.from_numpy(np.ascontiguousarray(x))[None, None], kernel_size=2, padding=(H % 2, W % 2))[0, 0].numpy()


def pool_zero_pad(x):
    """One zero row / column in front of an odd axis, then 0.25 * ((x00 + x01) + (x10 + x11)): (n + 1) // 2 outputs."""
    H, W = x.shape
    p = np.zeros((H + H % 2, W + W % 2), dtype=np.float64)
    p[H % 2:, W % 2:] = x
    return 0.25 * ((p[0::2, 0::2] + p[0::2, 1::2]) + (p[1::2, 0::2] + p[1::2, 1::2]))


FORMS = {"full": (S.filter_full, pool_torch), "separable": (S.filter_separable, pool_zero_pad)}


def level_means(x, y, filt, c1=C1, c2=C2):
    """One level of one pair of float64 planes -> (mean of the SSIM map, mean of the cs map)."""
    k = S.taps()
    mu1, mu2 = filt(x, k), filt(y, k)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 ** 2, mu2 ** 2, mu1 * mu2
    sigma1_sq = filt(x * x, k) - mu1_sq
    sigma2_sq = filt(y * y, k) - mu2_sq
    sigma12 = filt(x * y, k) - mu1_mu2
    cs_map = (2 * sigma12 + c2) / (sigma1_sq + sigma2_sq + c2)
    ssim_map = ((2 * mu1_mu2 + c1) / (mu1_sq + mu2_sq + c1)) * cs_map
    return ssim_map.mean(), cs_map.mean()


def levels_plane(x, y, levels, form="full"):
    """-> (levels, 2) float64 for one pair of 2-D planes."""
    filt, pool = FORMS[form]
    x, y = np.asarray(x).astype(np.float64), np.asarray(y).astype(np.float64)
    assert min(x.shape) > 10 * 2 ** (levels - 1)
    out = np.empty((levels, 2), dtype=np.float64)
    for l in range(levels):
        out[l] = level_means(x, y, filt)
        if l < levels - 1:
            x, y = pool(x), pool(y)
    return out


def ms_ssim_levels(a, b, levels=5, form="full"):
    """(..., H, W) -> (..., levels, 2) float64."""
    a, b = np.asarray(a), np.asarray(b)
    lead = a.shape[:-2]
    fa, fb = a.reshape((-1,) + a.shape[-2:]), b.reshape((-1,) + b.shape[-2:])
    with np.errstate(invalid="ignore"):      # inf - inf in a plane that holds an infinity: NaN, as the formula says
        return np.array([levels_plane(x, y, levels, form) for x, y in zip(fa, fb)], dtype=np.float64).reshape(lead + (levels, 2))


def factors(levels):
    """(..., L, 2) -> (..., L): cs of the levels before the last, ssim of the last -- what the value raises to the weights."""
    levels = np.asarray(levels)
    return np.concatenate([levels[..., :-1, 1], levels[..., -1:, 0]], axis=-1)


def combine(levels, weights=WEIGHTS):
    f = np.maximum(factors(levels), 0.0)     # relu; np.maximum hands a NaN on
    return np.prod(f ** np.asarray(weights[:f.shape[-1]], dtype=np.float64), axis=-1)


def ms_ssim_planes(a, b, weights=WEIGHTS, form="full"):
    return combine(ms_ssim_levels(a, b, len(weights), form), weights)


def ms_ssim_frames(pred, gt, weights=WEIGHTS, form="full"):
    """(n, C, H, W) -> (n,): the mean of the channels' values."""
    return ms_ssim_planes(pred, gt, weights, form).mean(axis=-1)


@functools.lru_cache(maxsize=None)
def case(kind, shape, levels=5, planes=3):
    """-> (a, b, yardstick levels (planes, levels, 2)) of the seeded content; computed once and shared: leave them unchanged."""
    a, b = content(kind, shape, planes)
    ref = ms_ssim_levels(a, b, levels)
    ref.setflags(write=False)            # (a and b go to torch.from_numpy as they are, which wants them writable)
    return a, b, ref
