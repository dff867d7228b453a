"""MS-SSIM as ``pytorch_msssim.ms_ssim`` defines it and CompressAI and ELIC evaluate it: data_range 1, the 11-tap Gaussian window
(sigma 1.5) over the valid region, K = (0.01, 0.03), five levels weighted (0.0448, 0.2856, 0.3001, 0.2363, 0.1333), between
levels ``avg_pool2d(kernel 2, stride 2, padding = size % 2)``; all in float64 on the float32 inputs, widened, as ssim.py.  The
pyramid and both maps of every level are one call of the fused float64 kernels (csrc/msssim.hip), which returns per plane and
level the means of the SSIM map and of its contrast-structure factor; the product of their powers is taken here, on the host:
ten numbers per plane.  DESIGN.md section 8g.

A reported value only: no decision rule reads it.
"""
import numpy as np
import torch

from .ssim import C1, C2, WINDOW, _as_planes, _device_taps, channel_mean

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MAX_LEVELS = 8


def min_side(levels=len(WEIGHTS)):
    """The shorter side of a frame must be larger than this: (win_size - 1) * 2^(levels - 1), 160 for five levels."""
    return (WINDOW - 1) * 2 ** (levels - 1)


def check_shapes(a_shape, b_shape, levels=len(WEIGHTS)):
    """What ``ms_ssim_levels`` refuses, before anything touches the device."""
    if not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f"MS-SSIM takes 1 .. {MAX_LEVELS} levels, got {levels}")
    if tuple(a_shape) != tuple(b_shape):
        raise ValueError(f"Input images must have the same dimensions: {tuple(a_shape)} and {tuple(b_shape)}")
    if len(a_shape) < 2 or min(a_shape[-2:]) <= min_side(levels):
        raise ValueError(f"MS-SSIM over {levels} level(s) needs planes whose shorter side is larger than {min_side(levels)} "
                         f"({WINDOW - 1} * 2^{levels - 1}: the last level must hold a window; nothing is padded), got {tuple(a_shape)}")


def ms_ssim_levels(a, b, levels=len(WEIGHTS), c1=C1, c2=C2, device=None):
    """a, b: (..., H, W) float32 tensors or arrays in [0, 1] -> float64 numpy array (..., levels, 2): per pair of planes and per
    pyramid level the mean of the SSIM map and the mean of the cs map, one call for all planes."""
    check_shapes(a.shape, b.shape, levels)
    lead = tuple(a.shape[:-2])
    H, W = a.shape[-2:]
    n = int(np.prod(lead, dtype=np.int64))
    if n == 0:
        return np.empty(lead + (levels, 2), dtype=np.float64)
    if n > 0x7fffffff:
        raise ValueError(f"{n} planes in one call: split the batch")
    from . import lib as L
    if device is None:
        on_dev = [t.device for t in (a, b) if torch.is_tensor(t) and t.is_cuda]
        device = on_dev[0] if on_dev else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    with torch.cuda.device(device):
        ta = _as_planes(a, device).view(n, H, W)
        tb = _as_planes(b, device).view(n, H, W)
        out = L.msssim_levels(ta, tb, levels, _device_taps(device), c1, c2)
    return out.cpu().numpy().reshape(lead + (levels, 2))


def combine(levels, weights=WEIGHTS):
    """(..., L, 2) level means -> (...): prod_{l < L-1} relu(cs_l)^w_l * relu(ssim_{L-1})^w_{L-1}.  relu keeps a NaN; a negative
    factor gives exactly 0."""
    v = np.asarray(levels, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    if v.ndim < 2 or v.shape[-1] != 2 or v.shape[-2] != len(w):
        raise ValueError(f"level means of shape (..., {len(w)}, 2) expected for {len(w)} weights, got {v.shape}")
    f = np.concatenate([v[..., :-1, 1], v[..., -1:, 0]], axis=-1)
    f = np.where(f < 0, 0.0, f)              # NaN < 0 is False: kept
    return np.prod(f ** w, axis=-1)


def ms_ssim_planes(a, b, weights=WEIGHTS, c1=C1, c2=C2):
    """a, b: (..., H, W) -> float64 (...): ``ms_ssim`` of every pair of planes."""
    return combine(ms_ssim_levels(a, b, len(weights), c1, c2), weights)


def ms_ssim_frames(pred, gt, weights=WEIGHTS, c1=C1, c2=C2):
    """pred, gt: (n, C, H, W), C in {1, 3} -> (n,) float64: ``ms_ssim(pred, gt, data_range=1, size_average=False)``, the mean
    of the channels' values."""
    if len(pred.shape) != 4 or pred.shape[1] not in (1, 3):
        raise ValueError(f"Wrong input image dimensions: {tuple(pred.shape)} (expected (n, 1 or 3, H, W))")
    return channel_mean(ms_ssim_planes(pred, gt, weights, c1, c2))


def to_db(v):
    """-10 log10(1 - v), the scale MS-SSIM is plotted on; inf at 1."""
    with np.errstate(divide="ignore"):
        return -10.0 * np.log10(1.0 - np.asarray(v, dtype=np.float64))


def size_message(H, W, levels=len(WEIGHTS)):
    """Why frames of H x W have no MS-SSIM and where whole frames come from; None when they have one."""
    if min(H, W) > min_side(levels):
        return None
    return (f"--ms-ssim: the frames are {W}x{H}, and {levels} levels need a shorter side > {min_side(levels)} (10 * 2^{levels - 1}; "
            f"nothing is padded).  Whole frames come from city_sender.py --yuv-fit joint, or from --yuv-fit tile and "
            f"city_stitch.py --ms-ssim")
