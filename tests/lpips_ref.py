"""LPIPS v0.1 with the VGG16, SqueezeNet 1.1 and AlexNet backbones, restated on torch CPU (test infrastructure only).

Written from the definitions, not from a run of the packages (neither ``lpips`` nor ``torchvision`` is importable here):

* ``torchvision.models.vgg16().features``: 3x3 pad-1 convolutions at 0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28, each with
  ReLU, ``MaxPool2d(2, 2)`` at 4, 9, 16, 23; lpips taps the ReLUs of 2, 7, 14, 21, 28 (64, 128, 256, 512, 512 channels);
* ``torchvision.models.squeezenet1_1().features``: 0 = ``Conv2d(3, 64, 3, stride=2)``, ReLU (tap), ``MaxPool2d(3, 2,
  ceil_mode=True)`` at 2, 5, 8, ``Fire`` at 3, 4, 6, 7, 9, 10, 11, 12 = 1x1 ``squeeze`` + ReLU, then ``expand1x1`` || ``expand3x3``
  (pad 1), each with ReLU, concatenated; lpips taps 1, 4, 7, 9, 10, 11, 12 (64, 128, 256, 384, 384, 512, 512 channels);
* AlexNet: ``oracle/lpips.py``;
* the head: ScalingLayer, ``x / (|x|_2 + 1e-10)`` over channels, squared difference, bias-free 1x1 ``lin`` layer, then the spatial
  mean (``distance``) or ``F.interpolate(size=(H, W), mode="bilinear", align_corners=False)`` (``spatial_map``), summed over taps.

Backbone weights are seeded stand-ins in torchvision's key names (He-scaled normal weights, small biases): the trained
checkpoints are not available.  The linear layers are the trained ones when ``lin`` (tests/golden/lpips_<net>_lin.npz) is given.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import lpips as OL

SHIFT, SCALE = OL.SHIFT, OL.SCALE
NETS = ("alex", "vgg", "squeeze")
CHANNELS = {"alex": OL.CHANNELS, "vgg": (64, 128, 256, 512, 512), "squeeze": (64, 128, 256, 384, 384, 512, 512)}
VGG = ((0, 3, 64), (2, 64, 64), "P", (5, 64, 128), (7, 128, 128), "P", (10, 128, 256), (12, 256, 256), (14, 256, 256), "P",
       (17, 256, 512), (19, 512, 512), (21, 512, 512), "P", (24, 512, 512), (26, 512, 512), (28, 512, 512))
VGG_TAPS = (2, 7, 14, 21, 28)
FIRES = ((3, 64, 16, 64), (4, 128, 16, 64), "P", (6, 128, 32, 128), (7, 256, 32, 128), "P", (9, 256, 48, 192), (10, 384, 48, 192),
         (11, 384, 64, 256), (12, 512, 64, 256))
FIRE_TAPS = (4, 7, 9, 10, 11, 12)
# where a saved lpips.LPIPS module keeps features[idx]: net.slice<K>.<idx>
SLICES = {"alex": {0: 1, 3: 2, 6: 3, 8: 4, 10: 5},
          "vgg": {0: 1, 2: 1, 5: 2, 7: 2, 10: 3, 12: 3, 14: 3, 17: 4, 19: 4, 21: 4, 24: 5, 26: 5, 28: 5},
          "squeeze": {0: 1, 3: 2, 4: 2, 6: 3, 7: 3, 9: 4, 10: 5, 11: 6, 12: 7}}


def _conv_weights(rng, sd, name, co, ci, k):
    sd[f"{name}.weight"] = torch.from_numpy((rng.standard_normal((co, ci, k, k)) * np.sqrt(2.0 / (ci * k * k))).astype(np.float32))
    sd[f"{name}.bias"] = torch.from_numpy((0.05 * rng.standard_normal(co)).astype(np.float32))


def seeded_state_dict(net, seed, lin=None):
    """Stand-in backbone in torchvision's key names + ``lin{k}.model.1.weight`` (trained when ``lin`` holds lin0.., else
    non-negative stand-ins)."""
    if net == "alex":
        return OL.seeded_state_dict(seed, lin)
    rng = np.random.default_rng(seed)
    sd = {}
    if net == "vgg":
        for e in VGG:
            if e != "P":
                _conv_weights(rng, sd, f"features.{e[0]}", e[2], e[1], 3)
    else:
        _conv_weights(rng, sd, "features.0", 64, 3, 3)
        for e in FIRES:
            if e != "P":
                idx, ci, sq, ex = e
                _conv_weights(rng, sd, f"features.{idx}.squeeze", sq, ci, 1)
                _conv_weights(rng, sd, f"features.{idx}.expand1x1", ex, sq, 1)
                _conv_weights(rng, sd, f"features.{idx}.expand3x3", ex, sq, 3)
    for i, c in enumerate(CHANNELS[net]):
        w = np.abs(rng.standard_normal((1, c, 1, 1))).astype(np.float32) / c
        if lin is not None:
            w = np.asarray(lin[f"lin{i}"], dtype=np.float32).reshape(1, c, 1, 1)
        sd[f"lin{i}.model.1.weight"] = torch.from_numpy(w.copy())
    return sd


def as_saved_module(net, sd):
    """The same weights under the key names of a saved ``lpips.LPIPS`` module: ``net.slice<K>.<idx>...`` and ``lins.<k>.``."""
    out = {}
    for k, v in sd.items():
        if k.startswith("features."):
            idx = int(k.split(".")[1])
            out[f"net.slice{SLICES[net][idx]}." + k[len("features."):]] = v
        else:
            out["lins." + k[3:]] = v
    return out


def features(net, sd, x):
    """The ReLU taps (NCHW) of the scaled input, x: (N, 3, H, W); the dtype of x decides the arithmetic."""
    if net == "alex":
        return OL.features(sd, x)
    g = lambda name: (sd[name + ".weight"].to(x.dtype), sd[name + ".bias"].to(x.dtype))  # noqa: E731
    h = (x - torch.tensor(SHIFT, dtype=x.dtype).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=x.dtype).view(1, 3, 1, 1)
    taps = []
    if net == "vgg":
        for e in VGG:
            if e == "P":
                h = F.max_pool2d(h, 2, 2)
                continue
            h = F.relu(F.conv2d(h, *g(f"features.{e[0]}"), padding=1))
            if e[0] in VGG_TAPS:
                taps.append(h)
        return taps
    h = F.relu(F.conv2d(h, *g("features.0"), stride=2))
    taps.append(h)
    h = F.max_pool2d(h, 3, 2, ceil_mode=True)
    for e in FIRES:
        if e == "P":
            h = F.max_pool2d(h, 3, 2, ceil_mode=True)
            continue
        s = F.relu(F.conv2d(h, *g(f"features.{e[0]}.squeeze")))
        h = torch.cat([F.relu(F.conv2d(s, *g(f"features.{e[0]}.expand1x1"))),
                       F.relu(F.conv2d(s, *g(f"features.{e[0]}.expand3x3"), padding=1))], 1)
        if e[0] in FIRE_TAPS:
            taps.append(h)
    return taps


def layer_map(a, b, lin_w):
    """One tap's per-pixel distance, (N, 1, h, w)."""
    na = a / (a.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    nb = b / (b.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    return F.conv2d((na - nb).pow(2), lin_w.to(a.dtype).reshape(1, -1, 1, 1))


def maps(net, sd, x0, x1):
    return [layer_map(a, b, sd[f"lin{i}.model.1.weight"]) for i, (a, b) in enumerate(zip(features(net, sd, x0), features(net, sd, x1)))]


def distance(net, sd, x0, x1):
    """lpips.LPIPS(net=net).forward(x0, x1) -> (N,)."""
    return sum(m.mean((1, 2, 3)) for m in maps(net, sd, x0, x1))


def spatial_map(net, sd, x0, x1):
    """lpips.LPIPS(net=net, spatial=True).forward(x0, x1) -> (N, H, W)."""
    size = tuple(x0.shape[-2:])
    return sum(F.interpolate(m, size=size, mode="bilinear", align_corners=False) for m in maps(net, sd, x0, x1))[:, 0]


def pairs(seed, n, h, w):
    """The inputs the tolerances were measured on: a = rand, b = clamp(a + 0.1 randn, 0, 1), in [0, 1]."""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand((n, 3, h, w), generator=g)
    b = (a + 0.1 * torch.randn((n, 3, h, w), generator=g)).clamp(0, 1)
    return a, b
