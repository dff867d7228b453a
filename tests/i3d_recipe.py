"""Seeded InceptionI3d(400) weights, the golden clips and a torch CPU restatement of the network, shared by
tests/golden/make_i3d_golden.py (which runs the reference module on them) and the FVD tests.

The restatement follows models/fvd/pytorch_i3d.py and models/fvd/fvd.py (preprocess_single) literally -- unfolded BatchNorm,
F.pad with TensorFlow-"same" amounts, NCTHW -- and is written independently of evc_amd.fvd so that it checks that module."""
import math

import numpy as np
import torch
import torch.nn.functional as F

# (name, Ci, Co, k, stride) of the stem units; Inception widths (b0, b1a, b1b, b2a, b2b, b3b)
STEM = (("Conv3d_1a_7x7", 3, 64, 7, 2), ("Conv3d_2b_1x1", 64, 64, 1, 1), ("Conv3d_2c_3x3", 64, 192, 3, 1))
MIXED = (("Mixed_3b", 192, (64, 96, 128, 16, 32, 32)), ("Mixed_3c", 256, (128, 128, 192, 32, 96, 64)),
         ("Mixed_4b", 480, (192, 96, 208, 16, 48, 64)), ("Mixed_4c", 512, (160, 112, 224, 24, 64, 64)),
         ("Mixed_4d", 512, (128, 128, 256, 24, 64, 64)), ("Mixed_4e", 512, (112, 144, 288, 32, 64, 64)),
         ("Mixed_4f", 528, (256, 160, 320, 32, 128, 128)), ("Mixed_5b", 832, (256, 160, 320, 32, 128, 128)),
         ("Mixed_5c", 832, (384, 192, 384, 48, 128, 128)))
POOLS = {"MaxPool3d_2a_3x3": ((1, 3, 3), (1, 2, 2)), "MaxPool3d_3a_3x3": ((1, 3, 3), (1, 2, 2)),
         "MaxPool3d_4a_3x3": ((3, 3, 3), (2, 2, 2)), "MaxPool3d_5a_2x2": ((2, 2, 2), (2, 2, 2))}
END_POINTS = ("Conv3d_1a_7x7", "MaxPool3d_2a_3x3", "Conv3d_2b_1x1", "Conv3d_2c_3x3", "MaxPool3d_3a_3x3", "Mixed_3b",
              "Mixed_3c", "MaxPool3d_4a_3x3", "Mixed_4b", "Mixed_4c", "Mixed_4d", "Mixed_4e", "Mixed_4f", "MaxPool3d_5a_2x2",
              "Mixed_5b", "Mixed_5c")
WEIGHT_SEED = 2024
# golden clips: (seed, T, H, W) -- five 30-frame 128^2 clips and one 16-frame non-square clip (T' = 2 at the head, a crop)
CLIPS = ((11, 30, 128, 128), (12, 30, 128, 128), (13, 30, 128, 128), (14, 30, 128, 128), (15, 30, 128, 128),
         (16, 16, 96, 128))


def units():
    """[(key prefix, Ci, Co, k, stride, has_bn)] of every Unit3D, in the reference module's names."""
    out = [(n, ci, co, k, (s, s, s), True) for n, ci, co, k, s in STEM]
    for name, ci, (c0, c1a, c1b, c2a, c2b, c3) in MIXED:
        out += [(f"{name}.b0", ci, c0, 1, (1, 1, 1), True), (f"{name}.b1a", ci, c1a, 1, (1, 1, 1), True),
                (f"{name}.b1b", c1a, c1b, 3, (1, 1, 1), True), (f"{name}.b2a", ci, c2a, 1, (1, 1, 1), True),
                (f"{name}.b2b", c2a, c2b, 3, (1, 1, 1), True), (f"{name}.b3b", ci, c3, 1, (1, 1, 1), True)]
    out.append(("logits", 1024, 400, 1, (1, 1, 1), False))
    return out


def seeded_state_dict(seed=WEIGHT_SEED):
    """Every parameter and BatchNorm buffer of InceptionI3d(400) from one default_rng: He-scaled weights, gamma in [0.8, 1.2],
    beta and running mean ~ N(0, 0.1) (non-zero), running variance in [0.5, 1.5] (positive, not 1)."""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, ci, co, k, _, bn in units():
        fan_in = ci * k ** 3
        sd[f"{name}.conv3d.weight"] = rng.standard_normal((co, ci, k, k, k)) * math.sqrt(2.0 / fan_in)
        if bn:
            sd[f"{name}.bn.weight"] = rng.uniform(0.8, 1.2, co)
            sd[f"{name}.bn.bias"] = rng.normal(0.0, 0.1, co)
            sd[f"{name}.bn.running_mean"] = rng.normal(0.0, 0.1, co)
            sd[f"{name}.bn.running_var"] = rng.uniform(0.5, 1.5, co)
        else:
            sd[f"{name}.conv3d.weight"] *= math.sqrt(0.5)
            sd[f"{name}.conv3d.bias"] = rng.normal(0.0, 0.1, co)
    return {k: torch.from_numpy(v.astype(np.float32)) for k, v in sd.items()}


def clip(seed, T, H, W):
    """(T, 3, H, W) float32 in [0, 1]: uniform noise of a per-clip contrast and offset, so that clips differ in their features."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.2, 1.0)
    c = rng.uniform(0.0, 1.0 - a)
    return torch.from_numpy((c + a * rng.random((T, 3, H, W))).astype(np.float32))


def compute_pad(size, k, s):
    return max(k - s, 0) if size % s == 0 else max(k - size % s, 0)


def same_pad_args(shape_thw, kernel, stride):
    """F.pad argument (w_f, w_b, h_f, h_b, t_f, t_b) of the TensorFlow-"same" padding."""
    out = []
    for size, k, s in reversed(list(zip(shape_thw, kernel, stride))):
        p = compute_pad(size, k, s)
        out += [p // 2, p - p // 2]
    return tuple(out)


def preprocess(video, resolution=224):
    """preprocess_single: video (C, T, H, W) in [0, 1]."""
    c, t, h, w = video.shape
    scale = resolution / min(h, w)
    size = (resolution, math.ceil(w * scale)) if h < w else (math.ceil(h * scale), resolution)
    video = F.interpolate(video, size=size, mode="bilinear", align_corners=False)
    h0, w0 = (video.shape[2] - resolution) // 2, (video.shape[3] - resolution) // 2
    return ((video[:, :, h0:h0 + resolution, w0:w0 + resolution] - 0.5) * 2).contiguous()


def _unit(sd, name, x, k, stride, bn=True):
    x = F.pad(x, same_pad_args(x.shape[2:], (k,) * 3, stride))
    x = F.conv3d(x, sd[f"{name}.conv3d.weight"], sd.get(f"{name}.conv3d.bias"), stride)
    if not bn:
        return x
    x = F.batch_norm(x, sd[f"{name}.bn.running_mean"], sd[f"{name}.bn.running_var"], sd[f"{name}.bn.weight"],
                     sd[f"{name}.bn.bias"], False, 0.0, 1e-5)
    return F.relu(x)


def _pool(x, kernel, stride):
    return F.max_pool3d(F.pad(x, same_pad_args(x.shape[2:], kernel, stride)), kernel, stride)


def forward(sd, clips):
    """clips: (B, T, 3, H, W) in [0, 1] -> ((B, 400) logits, {end point: (B, C, T', H', W')}), torch CPU fp32."""
    sd = {k: v.float() for k, v in sd.items()}
    x = torch.stack([preprocess(v.permute(1, 0, 2, 3)) for v in clips])
    eps = {}
    stems = {n: (k, s) for n, _, _, k, s in STEM}
    widths = {n: w for n, _, w in MIXED}
    with torch.no_grad():
        for ep in END_POINTS:
            if ep in stems:
                k, s = stems[ep]
                x = _unit(sd, ep, x, k, (s, s, s))
            elif ep in POOLS:
                x = _pool(x, *POOLS[ep])
            else:
                b0 = _unit(sd, f"{ep}.b0", x, 1, (1, 1, 1))
                b1 = _unit(sd, f"{ep}.b1b", _unit(sd, f"{ep}.b1a", x, 1, (1, 1, 1)), 3, (1, 1, 1))
                b2 = _unit(sd, f"{ep}.b2b", _unit(sd, f"{ep}.b2a", x, 1, (1, 1, 1)), 3, (1, 1, 1))
                b3 = _unit(sd, f"{ep}.b3b", _pool(x, (3, 3, 3), (1, 1, 1)), 1, (1, 1, 1))
                assert b0.shape[1] == widths[ep][0]
                x = torch.cat([b0, b1, b2, b3], 1)
            eps[ep] = x
        x = F.avg_pool3d(x, (2, 7, 7), (1, 1, 1))
        x = _unit(sd, "logits", x, 1, (1, 1, 1), bn=False)
        logits = x.squeeze(3).squeeze(3).mean(2)
    return logits, eps


def checksums(t):
    """A few numbers that pin an end point: sum, sum of |x|, max."""
    t = t.double()
    return np.array([float(t.sum()), float(t.abs().sum()), float(t.max())])
