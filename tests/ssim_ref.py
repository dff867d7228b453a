"""Float64 yardstick of SSIM, restated from the formula of the reference's fvd_utils/calculate_ssim.py:6-42 (cv2 is not
available here, so the reference itself cannot be run): inputs in [0, 1], C1 = 0.01^2, C2 = 0.03^2, the window
exp(-(i-5)^2 / (2 1.5^2)) over its sum applied as the 2-D outer product, the valid region only, the map's mean.

Two independent forms of the filter: (a) ``scipy.signal.correlate2d`` with the 121-tap outer product, literally what
``filter2D(...)[5:-5, 5:-5]`` yields; (b) separable, 11 taps along rows and then along columns.  They differ by summation
order only."""
import numpy as np

C1, C2 = 0.01 ** 2, 0.03 ** 2


def taps(size=11, sigma=1.5):
    i = np.arange(size, dtype=np.float64) - (size - 1) / 2
    k = np.exp(-(i ** 2) / (2 * sigma ** 2))
    return k / k.sum()


def filter_full(x, k):
    from scipy.signal import correlate2d
    return correlate2d(x, np.outer(k, k), mode="valid")


def filter_separable(x, k):
    n = len(k)
    rows = sum(k[j] * x[:, j:x.shape[1] - n + 1 + j] for j in range(n))
    return sum(k[j] * rows[j:rows.shape[0] - n + 1 + j, :] for j in range(n))


def ssim_plane(img1, img2, filt=filter_full, c1=C1, c2=C2):
    """calculate_ssim.py:6-23 for one pair of 2-D planes."""
    img1, img2 = np.asarray(img1).astype(np.float64), np.asarray(img2).astype(np.float64)
    k = taps()
    mu1, mu2 = filt(img1, k), filt(img2, k)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 ** 2, mu2 ** 2, mu1 * mu2
    sigma1_sq = filt(img1 ** 2, k) - mu1_sq
    sigma2_sq = filt(img2 ** 2, k) - mu2_sq
    sigma12 = filt(img1 * img2, k) - mu1_mu2
    ssim_map = ((2 * mu1_mu2 + c1) * (2 * sigma12 + c2)) / ((mu1_sq + mu2_sq + c1) * (sigma1_sq + sigma2_sq + c2))
    return ssim_map.mean()


def ssim_planes(a, b, filt=filter_full):
    """(..., H, W) -> float64 array of the leading shape."""
    a, b = np.asarray(a), np.asarray(b)
    lead = a.shape[:-2]
    fa, fb = a.reshape((-1,) + a.shape[-2:]), b.reshape((-1,) + b.shape[-2:])
    with np.errstate(invalid="ignore"):      # inf - inf in a plane that holds an infinity: NaN, as the formula says
        return np.array([ssim_plane(x, y, filt) for x, y in zip(fa, fb)], dtype=np.float64).reshape(lead)


def calculate_ssim(videos1, videos2, calculate_per_frame, calculate_final):
    """calculate_ssim.py:47-100 on (B, T, C, H, W) arrays."""
    v = ssim_planes(videos1, videos2).mean(axis=-1)
    ssim, ssim_std = {}, {}
    for t in range(calculate_per_frame, v.shape[1] + 1, calculate_per_frame):
        ssim[f"avg[:{t}]"] = np.mean(v[:, :t])
        ssim_std[f"std[:{t}]"] = np.std(v[:, :t])
    if calculate_final:
        ssim["final"] = np.mean(v)
        ssim_std["final"] = np.std(v)
    return {"ssim": ssim, "ssim_std": ssim_std, "ssim_per_frame": calculate_per_frame,
            "ssim_video_setting": tuple(np.asarray(videos1).shape[1:]), "ssim_video_setting_name": "time, channel, heigth, width"}


# ---- the seeded content kinds and shapes the host and GPU tests share -------------------------------------------------------

SHAPES = [(11, 11), (12, 17), (34, 70), (128, 128)]
KINDS = ["noise", "noisy_copy", "nearly_flat", "quantised_identical"]


def content(kind, shape, planes=3, seed=0):
    """-> (a, b): float32 (planes, H, W) in [0, 1]."""
    rng = np.random.default_rng([seed, KINDS.index(kind), shape[0], shape[1]])
    full = (planes,) + tuple(shape)
    if kind == "noise":
        a, b = rng.random(full), rng.random(full)
    elif kind == "noisy_copy":
        a = rng.random(full)
        b = np.clip(a + 0.02 * rng.standard_normal(full), 0.0, 1.0)
    elif kind == "nearly_flat":
        a, b = 0.7 + 1e-4 * (2 * rng.random(full) - 1), 0.7 + 1e-4 * (2 * rng.random(full) - 1)
    else:
        a = np.round(rng.random(full) * 255) / 255
        b = a.copy()
    return a.astype(np.float32), b.astype(np.float32)
