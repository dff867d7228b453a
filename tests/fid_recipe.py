"""Seeded weights of pytorch-fid's Inception-v3, a torch CPU restatement of the network and float64 references of the two set
metrics, shared by tests/golden/make_fid_golden.py and the FID tests.

The restatement follows the reference's evaluation/inception.py (the four blocks, the resize to 299 x 299, 2x - 1, the patched
FIDInceptionA / C / E_1 / E_2 forwards) and torchvision's Inception3 module structure, through torch.nn.functional only
(unfolded BatchNorm, NCHW), in float32 or float64.  It is written independently of evc_amd.fid so that it checks that module."""
import math

import numpy as np
import torch
import torch.nn.functional as F

WEIGHT_SEED = 2025
BN_EPS = 1e-3
MIXED_NAMES = ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a",
               "Mixed_7b", "Mixed_7c")
BLOCKS = ("block0", "block1", "block2", "block3")
END_POINTS = BLOCKS + MIXED_NAMES


def _a(ci, pf):
    return [("branch1x1", ci, 64, 1, 1), ("branch5x5_1", ci, 48, 1, 1), ("branch5x5_2", 48, 64, 5, 5),
            ("branch3x3dbl_1", ci, 64, 1, 1), ("branch3x3dbl_2", 64, 96, 3, 3), ("branch3x3dbl_3", 96, 96, 3, 3),
            ("branch_pool", ci, pf, 1, 1)]


def _c(c7):
    return [("branch1x1", 768, 192, 1, 1), ("branch7x7_1", 768, c7, 1, 1), ("branch7x7_2", c7, c7, 1, 7), ("branch7x7_3", c7, 192, 7, 1),
            ("branch7x7dbl_1", 768, c7, 1, 1), ("branch7x7dbl_2", c7, c7, 7, 1), ("branch7x7dbl_3", c7, c7, 1, 7),
            ("branch7x7dbl_4", c7, c7, 7, 1), ("branch7x7dbl_5", c7, 192, 1, 7), ("branch_pool", 768, 192, 1, 1)]


def _e(ci):
    return [("branch1x1", ci, 320, 1, 1), ("branch3x3_1", ci, 384, 1, 1), ("branch3x3_2a", 384, 384, 1, 3),
            ("branch3x3_2b", 384, 384, 3, 1), ("branch3x3dbl_1", ci, 448, 1, 1), ("branch3x3dbl_2", 448, 384, 3, 3),
            ("branch3x3dbl_3a", 384, 384, 1, 3), ("branch3x3dbl_3b", 384, 384, 3, 1), ("branch_pool", ci, 192, 1, 1)]


def units():
    """[(key prefix, Ci, Co, KH, KW)] of every BasicConv2d the four blocks use, in torchvision's names."""
    out = [("Conv2d_1a_3x3", 3, 32, 3, 3), ("Conv2d_2a_3x3", 32, 32, 3, 3), ("Conv2d_2b_3x3", 32, 64, 3, 3),
           ("Conv2d_3b_1x1", 64, 80, 1, 1), ("Conv2d_4a_3x3", 80, 192, 3, 3)]
    mixed = {"Mixed_5b": _a(192, 32), "Mixed_5c": _a(256, 64), "Mixed_5d": _a(288, 64),
             "Mixed_6a": [("branch3x3", 288, 384, 3, 3), ("branch3x3dbl_1", 288, 64, 1, 1), ("branch3x3dbl_2", 64, 96, 3, 3),
                          ("branch3x3dbl_3", 96, 96, 3, 3)],
             "Mixed_6b": _c(128), "Mixed_6c": _c(160), "Mixed_6d": _c(160), "Mixed_6e": _c(192),
             "Mixed_7a": [("branch3x3_1", 768, 192, 1, 1), ("branch3x3_2", 192, 320, 3, 3), ("branch7x7x3_1", 768, 192, 1, 1),
                          ("branch7x7x3_2", 192, 192, 1, 7), ("branch7x7x3_3", 192, 192, 7, 1), ("branch7x7x3_4", 192, 192, 3, 3)],
             "Mixed_7b": _e(1280), "Mixed_7c": _e(2048)}
    for name in MIXED_NAMES:
        out += [(f"{name}.{n}", ci, co, kh, kw) for n, ci, co, kh, kw in mixed[name]]
    return out


def seeded_state_dict(seed=WEIGHT_SEED):
    """Every convolution weight and BatchNorm buffer of the four blocks from one default_rng: He-scaled weights, gamma in
    [0.8, 1.2], beta and running mean ~ N(0, 0.1), running variance in [0.5, 1.5]; plus the keys of pytorch-fid's file that the
    feature network does not use (a small ``fc`` and the BatchNorm counters)."""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, ci, co, kh, kw in units():
        sd[f"{name}.conv.weight"] = rng.standard_normal((co, ci, kh, kw)) * math.sqrt(2.0 / (ci * kh * kw))
        sd[f"{name}.bn.weight"] = rng.uniform(0.8, 1.2, co)
        sd[f"{name}.bn.bias"] = rng.normal(0.0, 0.1, co)
        sd[f"{name}.bn.running_mean"] = rng.normal(0.0, 0.1, co)
        sd[f"{name}.bn.running_var"] = rng.uniform(0.5, 1.5, co)
    out = {k: torch.from_numpy(v.astype(np.float32)) for k, v in sd.items()}
    for name, *_ in units():
        out[f"{name}.bn.num_batches_tracked"] = torch.tensor(0)
    out["fc.weight"], out["fc.bias"] = torch.zeros((8, 2048)), torch.zeros(8)
    return out


def images(seed, n, h, w):
    """(n, 3, h, w) float32 in [0, 1]: smooth low-frequency content plus noise, a per-image contrast and offset."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        a = rng.uniform(0.3, 1.0)
        c = rng.uniform(0.0, 1.0 - a)
        low = torch.from_numpy(rng.random((1, 3, 8, 8)))
        smooth = F.interpolate(low, size=(h, w), mode="bilinear", align_corners=True)[0].numpy()
        out.append(c + a * (0.5 * smooth + 0.5 * rng.random((3, h, w))))
    return torch.from_numpy(np.stack(out).astype(np.float32))


def _bc(sd, name, x, stride=1, padding=0):
    x = F.conv2d(x, sd[f"{name}.conv.weight"], None, stride, padding)
    x = F.batch_norm(x, sd[f"{name}.bn.running_mean"], sd[f"{name}.bn.running_var"], sd[f"{name}.bn.weight"],
                     sd[f"{name}.bn.bias"], False, 0.0, BN_EPS)
    return F.relu(x)


def _avg(x):
    return F.avg_pool2d(x, kernel_size=3, stride=1, padding=1, count_include_pad=False)


def _inception_a(sd, n, x):
    b1 = _bc(sd, f"{n}.branch1x1", x)
    b5 = _bc(sd, f"{n}.branch5x5_2", _bc(sd, f"{n}.branch5x5_1", x), padding=2)
    b3 = _bc(sd, f"{n}.branch3x3dbl_1", x)
    b3 = _bc(sd, f"{n}.branch3x3dbl_3", _bc(sd, f"{n}.branch3x3dbl_2", b3, padding=1), padding=1)
    return torch.cat([b1, b5, b3, _bc(sd, f"{n}.branch_pool", _avg(x))], 1)


def _inception_b(sd, n, x):
    b3 = _bc(sd, f"{n}.branch3x3", x, stride=2)
    bd = _bc(sd, f"{n}.branch3x3dbl_2", _bc(sd, f"{n}.branch3x3dbl_1", x), padding=1)
    bd = _bc(sd, f"{n}.branch3x3dbl_3", bd, stride=2)
    return torch.cat([b3, bd, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


def _inception_c(sd, n, x):
    b1 = _bc(sd, f"{n}.branch1x1", x)
    b7 = _bc(sd, f"{n}.branch7x7_1", x)
    b7 = _bc(sd, f"{n}.branch7x7_2", b7, padding=(0, 3))
    b7 = _bc(sd, f"{n}.branch7x7_3", b7, padding=(3, 0))
    bd = _bc(sd, f"{n}.branch7x7dbl_1", x)
    bd = _bc(sd, f"{n}.branch7x7dbl_2", bd, padding=(3, 0))
    bd = _bc(sd, f"{n}.branch7x7dbl_3", bd, padding=(0, 3))
    bd = _bc(sd, f"{n}.branch7x7dbl_4", bd, padding=(3, 0))
    bd = _bc(sd, f"{n}.branch7x7dbl_5", bd, padding=(0, 3))
    return torch.cat([b1, b7, bd, _bc(sd, f"{n}.branch_pool", _avg(x))], 1)


def _inception_d(sd, n, x):
    b3 = _bc(sd, f"{n}.branch3x3_2", _bc(sd, f"{n}.branch3x3_1", x), stride=2)
    b7 = _bc(sd, f"{n}.branch7x7x3_1", x)
    b7 = _bc(sd, f"{n}.branch7x7x3_2", b7, padding=(0, 3))
    b7 = _bc(sd, f"{n}.branch7x7x3_3", b7, padding=(3, 0))
    b7 = _bc(sd, f"{n}.branch7x7x3_4", b7, stride=2)
    return torch.cat([b3, b7, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


def _inception_e(sd, n, x, pool):
    b1 = _bc(sd, f"{n}.branch1x1", x)
    b3 = _bc(sd, f"{n}.branch3x3_1", x)
    b3 = torch.cat([_bc(sd, f"{n}.branch3x3_2a", b3, padding=(0, 1)), _bc(sd, f"{n}.branch3x3_2b", b3, padding=(1, 0))], 1)
    bd = _bc(sd, f"{n}.branch3x3dbl_2", _bc(sd, f"{n}.branch3x3dbl_1", x), padding=1)
    bd = torch.cat([_bc(sd, f"{n}.branch3x3dbl_3a", bd, padding=(0, 1)), _bc(sd, f"{n}.branch3x3dbl_3b", bd, padding=(1, 0))], 1)
    return torch.cat([b1, b3, bd, _bc(sd, f"{n}.branch_pool", pool(x))], 1)


def preprocess(x):
    """inception.py:146-153: bilinear resize to 299 x 299, align_corners=False, then 2x - 1."""
    return 2 * F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False) - 1


def forward(sd, x, dtype=torch.float32, last="block3"):
    """x: (N, 3, H, W) in [0, 1] -> {end point: tensor}: block0..block2 and every Mixed_* as (N, C, H', W'), block3 as (N, 2048);
    torch CPU in ``dtype``.  ``last="block0"`` stops after the first block."""
    sd = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}
    eps = {}
    with torch.no_grad():
        x = preprocess(x.to(dtype))
        x = _bc(sd, "Conv2d_1a_3x3", x, stride=2)
        x = _bc(sd, "Conv2d_2a_3x3", x)
        x = _bc(sd, "Conv2d_2b_3x3", x, padding=1)
        x = eps["block0"] = F.max_pool2d(x, kernel_size=3, stride=2)
        if last == "block0":
            return eps
        x = _bc(sd, "Conv2d_3b_1x1", x)
        x = _bc(sd, "Conv2d_4a_3x3", x)
        x = eps["block1"] = F.max_pool2d(x, kernel_size=3, stride=2)
        for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
            x = eps[n] = _inception_a(sd, n, x)
        x = eps["Mixed_6a"] = _inception_b(sd, "Mixed_6a", x)
        for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            x = eps[n] = _inception_c(sd, n, x)
        eps["block2"] = x
        x = eps["Mixed_7a"] = _inception_d(sd, "Mixed_7a", x)
        x = eps["Mixed_7b"] = _inception_e(sd, "Mixed_7b", x, _avg)
        x = eps["Mixed_7c"] = _inception_e(sd, "Mixed_7c", x, lambda t: F.max_pool2d(t, kernel_size=3, stride=1, padding=1))
        eps["block3"] = F.adaptive_avg_pool2d(x, (1, 1)).flatten(1)
    return eps


# ---- fid_ref: the two set metrics in numpy / scipy float64 --------------------------------------------------------------
def frechet_distance_sqrtm(feats_a, feats_b, eps=1e-6):
    """The Frechet distance in the reference's form: |mu_a - mu_b|^2 + Tr(S_a) + Tr(S_b) - 2 Tr(sqrtm(S_a S_b)), the matrix
    square root by scipy, eps on the diagonals when the product is singular."""
    from scipy import linalg
    a, b = np.asarray(feats_a, dtype=np.float64), np.asarray(feats_b, dtype=np.float64)
    mu_a, mu_b = a.mean(axis=0), b.mean(axis=0)
    s_a, s_b = np.atleast_2d(np.cov(a, rowvar=False)), np.atleast_2d(np.cov(b, rowvar=False))
    root, _ = linalg.sqrtm(s_a.dot(s_b), disp=False)
    if not np.isfinite(root).all():
        off = np.eye(s_a.shape[0]) * eps
        root = linalg.sqrtm((s_a + off).dot(s_b + off))
    root = np.real(root)
    diff = mu_a - mu_b
    return float(diff.dot(diff) + np.trace(s_a) + np.trace(s_b) - 2 * np.trace(root))


def frechet_distance_eig(feats_a, feats_b):
    """The same quantity from the eigenvalues of the Gram matrix M M^T, M = A_c B_c^T / sqrt((n - 1)(m - 1)): Tr sqrt(S_a S_b) is
    the sum of their square roots.  Float64; holds when the covariances are rank deficient."""
    a, b = np.asarray(feats_a, dtype=np.float64), np.asarray(feats_b, dtype=np.float64)
    ac, bc = a - a.mean(axis=0), b - b.mean(axis=0)
    m = ac.dot(bc.T) / math.sqrt((len(a) - 1.0) * (len(b) - 1.0))
    ev = np.clip(np.linalg.eigvalsh(m.dot(m.T)), 0.0, None)
    diff = a.mean(axis=0) - b.mean(axis=0)
    return float(diff.dot(diff) + np.square(ac).sum() / (len(a) - 1) + np.square(bc).sum() / (len(b) - 1) - 2 * np.sqrt(ev).sum())


def dist2(a, b):
    """(n, m) squared distances by direct differences, float64."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.square(a[:, None, :] - b[None, :, :]).sum(-1)


def knn_radius2(x, k):
    """Squared distance of every row to its (k + 1)-th nearest row, itself included: kthvalue(k + 1) of the self distances."""
    return np.sort(dist2(x, x), axis=1)[:, k]


def precision_recall(real, gen, k=3):
    """Precision / recall of pr.py by direct-difference distances, float64, squared values compared."""
    d = dist2(gen, real)
    precision = (d <= knn_radius2(real, k)[None, :]).any(axis=1).mean()
    recall = (d.T <= knn_radius2(gen, k)[None, :]).any(axis=1).mean()
    return float(precision), float(recall)


def min_gap(real, gen, k=3):
    """The smallest relative gap |dist - radius| / radius over every comparison precision / recall make (distances, not
    squares, as the reference compares them), float64."""
    d = np.sqrt(dist2(gen, real))
    rr, rg = np.sqrt(knn_radius2(real, k)), np.sqrt(knn_radius2(gen, k))
    return float(min((np.abs(d - rr[None, :]) / rr[None, :]).min(), (np.abs(d.T - rg[None, :]) / rg[None, :]).min()))


# seeded feature sets of the golden: (seed, n, m, d, shift, k); real = N(0, 1), generated = 0.9 N(0, 1) + shift
PR_SETS = ((7, 40, 30, 64, 0.6, 3), (7, 5, 4, 16, 0.3, 3))
GAP_BAR = 1e-3


def feature_sets(seed, n, m, d, shift):
    rng = np.random.default_rng(seed)
    real = rng.standard_normal((n, d)).astype(np.float32)
    gen = (0.9 * rng.standard_normal((m, d)) + shift).astype(np.float32)
    return real, gen
