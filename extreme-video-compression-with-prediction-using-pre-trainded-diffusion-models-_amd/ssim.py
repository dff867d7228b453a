"""SSIM as the reference's metric helpers define it (fvd_utils/calculate_ssim.py, copied under benchmark/fvd_utils/): the
11x11 Gaussian window (sigma 1.5) over the valid region, C1 = 0.01^2, C2 = 0.03^2, inputs in [0, 1], all in float64.  The
planes go through one launch of the fused float64 window kernel (csrc/ssim.hip); the host computes the taps, shapes the
batch and assembles the reference's result dict.

A reported value only: no decision rule reads it (``policy.load_metric("ssim")`` stays refused).
"""
import numpy as np
import torch

WINDOW, SIGMA = 11, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2

_taps_cache = {}


def gaussian_taps(size=WINDOW, sigma=SIGMA):
    """cv2.getGaussianKernel(size, sigma) for sigma > 0: exp(-(i - (size-1)/2)^2 / (2 sigma^2)) over its sum, float64."""
    i = np.arange(size, dtype=np.float64) - (size - 1) / 2
    k = np.exp(-(i * i) / (2.0 * sigma * sigma))
    return k / k.sum()


def _device_taps(device):
    key = (device.type, device.index)
    if key not in _taps_cache:
        _taps_cache[key] = torch.from_numpy(gaussian_taps()).to(device)
    return _taps_cache[key]


def _as_planes(x, device):
    """-> float32 tensor on the device (uploaded when it is on the host)."""
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    if t.dtype != torch.float32:
        raise ValueError(f"SSIM takes float32 planes in [0, 1], got {t.dtype}")
    return t.to(device).contiguous()


def check_shapes(a_shape, b_shape):
    """What ``ssim_planes`` refuses, before anything touches the device."""
    if tuple(a_shape) != tuple(b_shape):
        raise ValueError(f"Input images must have the same dimensions: {tuple(a_shape)} and {tuple(b_shape)}")
    if len(a_shape) < 2 or a_shape[-2] < WINDOW or a_shape[-1] < WINDOW:
        raise ValueError(f"SSIM needs planes of at least {WINDOW}x{WINDOW} (the window's valid region), got {tuple(a_shape)}")


def ssim_planes(a, b, c1=C1, c2=C2, device=None):
    """a, b: (..., H, W) float32 tensors or arrays in [0, 1] -> float64 numpy array of the leading shape: ``ssim(img1, img2)``
    of calculate_ssim.py:6-23 for every pair of planes, one launch for all of them."""
    check_shapes(a.shape, b.shape)
    lead = tuple(a.shape[:-2])
    H, W = a.shape[-2:]
    n = int(np.prod(lead, dtype=np.int64))
    if n == 0:
        return np.empty(lead, dtype=np.float64)
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
        out = L.ssim_planes(ta, tb, _device_taps(device), c1, c2)
    return out.cpu().numpy().reshape(lead)


def ssim_frames(pred, gt, c1=C1, c2=C2):
    """pred, gt: (n, C, H, W), C in {1, 3} -> (n,) float64: ``calculate_ssim_function`` (calculate_ssim.py:26-42) per frame,
    the mean of the channels' values."""
    if len(pred.shape) != 4 or pred.shape[1] not in (1, 3):
        raise ValueError(f"Wrong input image dimensions: {tuple(pred.shape)} (expected (n, 1 or 3, H, W))")
    return channel_mean(ssim_planes(pred, gt, c1, c2))


def channel_mean(values):
    """(..., C) plane values -> (...): np.array(ssims).mean() of calculate_ssim.py:38."""
    return np.asarray(values, dtype=np.float64).mean(axis=-1)


def ssim_result(values, calculate_per_frame, calculate_final, video_shape):
    """The dict ``calculate_ssim`` returns (calculate_ssim.py:79-100) from the (videos, frames) array of per-frame values;
    ``video_shape``: (T, C, H, W) of one video."""
    v = np.asarray(values, dtype=np.float64)
    ssim, ssim_std = {}, {}
    for t in range(calculate_per_frame, v.shape[1] + 1, calculate_per_frame):
        ssim[f"avg[:{t}]"] = np.mean(v[:, :t])
        ssim_std[f"std[:{t}]"] = np.std(v[:, :t])
    if calculate_final:
        ssim["final"] = np.mean(v)
        ssim_std["final"] = np.std(v)
    return {"ssim": ssim, "ssim_std": ssim_std, "ssim_per_frame": calculate_per_frame,
            "ssim_video_setting": tuple(video_shape), "ssim_video_setting_name": "time, channel, heigth, width"}


def calculate_ssim(videos1, videos2, calculate_per_frame, calculate_final, c1=C1, c2=C2):
    """videos: (B, T, C, H, W) in [0, 1] -> the reference's result dict; every plane of every video in one launch."""
    if tuple(videos1.shape) != tuple(videos2.shape) or len(videos1.shape) != 5:
        raise ValueError(f"videos must be two (B, T, C, H, W) arrays of one shape: {tuple(videos1.shape)}, {tuple(videos2.shape)}")
    if videos1.shape[2] not in (1, 3):
        raise ValueError(f"Wrong input image dimensions: {tuple(videos1.shape)} (C must be 1 or 3)")
    values = channel_mean(ssim_planes(videos1, videos2, c1, c2))
    return ssim_result(values, calculate_per_frame, calculate_final, videos1.shape[1:])
