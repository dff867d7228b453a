"""LPIPS (AlexNet, v0.1) on the HIP kernels: the perceptual distance of the sender's decision rule.

Mirrors ``lpips.LPIPS(net='alex')`` as the reference builds and calls it (``city_sender.py:302``; ``decide_5to5_lpips``,
``:376-406``: one (3, H, W) frame pair at a time, [0, 1] data passed as is).  The algorithm is the one the reference vendors in
``models/networks_basic.py:62-93`` (``PNetLin.forward``, ``ScalingLayer``), ``models/eval_models.py:35-37`` and
``models/pretrained_networks.py:56-94`` (oracle/lpips.py restates it).  Weights: ``LpipsAlex`` takes a state dict in the packages'
own key names -- ``features.{0,3,6,8,10}.{weight,bias}`` (torchvision ``alexnet``; not in the reference tree, cannot be fetched
offline) plus ``lin{k}.model.1.weight`` (the reference's ``weights/v0.1/alex.pth``; the ``lins.{k}.`` and ``net.slice*``
spellings of a saved ``LPIPS`` module are accepted too) -- or the two files themselves (``from_files``).

Data path: NCHW frames -> ``evc_im2col_nchw_f32`` (ScalingLayer + 11x11 stride-4 patches) -> 1x1 convolution, then
``evc_maxpool3s2_nhwc_f32`` and 5x5 / 3x3 convolutions, all on ``evc_conv2d_nhwc_f32`` with the exact bf16 split (the inputs are
not normalised) and ReLU fused in the epilogue; ``evc_lpips_layer_f32`` per tap.  Both images of a pair go through the
backbone as one batch.

``Lpips`` (second half of the file) is the whole family -- ``alex``, ``vgg``, ``squeeze`` -- on a pixel-parallel head, with
spatial maps: the reported ``--lpips`` value and the ``--lpips-net`` decision rule.  ``LpipsAlex`` is untouched.
"""
import torch

from . import lib as L

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# (features index, Ci, Co, kernel, stride, pad) -- torchvision.models.alexnet().features
CONVS = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1))
# where a saved lpips.LPIPS module keeps the backbone convolutions (lpips/pretrained_networks.py: alexnet slices)
_SLICE_KEYS = {0: "net.slice1.0", 3: "net.slice2.3", 6: "net.slice3.6", 8: "net.slice4.8", 10: "net.slice5.10"}
_IM2COL_LD = 368                                       # 3 * 11 * 11 = 363 patch entries, padded to a multiple of 16


def _find(sd, *names):
    for n in names:
        if n in sd:
            return sd[n]
    raise KeyError(f"LPIPS state dict holds none of {names}")


class LpipsAlex:
    def __init__(self, state_dict, device=None):
        L.hip_lib()                                                  # fails loudly without the HIP library / a gfx950 device
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.arith = L.default_arith()
        dev = self.device
        self.shift = torch.tensor(SHIFT, dtype=torch.float32, device=dev)
        self.scale = torch.tensor(SCALE, dtype=torch.float32, device=dev)
        self.layers = []
        for idx, ci, co, k, stride, pad in CONVS:
            w = _find(state_dict, f"features.{idx}.weight", f"{_SLICE_KEYS[idx]}.weight").detach().float().to(dev)
            b = _find(state_dict, f"features.{idx}.bias", f"{_SLICE_KEYS[idx]}.bias").detach().float().to(dev).contiguous()
            if tuple(w.shape) != (co, ci, k, k) or tuple(b.shape) != (co,):
                raise ValueError(f"features.{idx}: expected weight {(co, ci, k, k)}, got {tuple(w.shape)}")
            if idx == 0:                                             # as a 1x1 convolution over the im2col rows
                wp = torch.zeros((co, _IM2COL_LD, 1, 1), dtype=torch.float32, device=dev)
                wp[:, :ci * k * k, 0, 0] = w.reshape(co, -1)
                w, k = wp, 1
            self.layers.append(dict(w=L.conv_pack_weights(w.contiguous(), self.arith), b=b, co=co, k=k))
        self.lins = []
        for i, (_, _, co, _, _, _) in enumerate(CONVS):
            w = _find(state_dict, f"lin{i}.model.1.weight", f"lins.{i}.model.1.weight").detach().float().to(dev)
            if w.numel() != co:
                raise ValueError(f"lin{i}: expected {co} weights, got {tuple(w.shape)}")
            self.lins.append(w.reshape(-1).contiguous())

    @classmethod
    def from_files(cls, alexnet_path, lin_path, device=None):
        """torchvision's ``alexnet-owt-*.pth`` and lpips' ``weights/v0.1/alex.pth``, read with the weights-only loader."""
        sd = dict(torch.load(alexnet_path, map_location="cpu", weights_only=True))
        sd.update(torch.load(lin_path, map_location="cpu", weights_only=True))
        return cls(sd, device)

    def features(self, x):
        """x: (N, 3, H, W) float32 on the device -> the five ReLU taps, NHWC."""
        h = L.im2col_nchw(x.contiguous(), 11, 11, 4, 2, _IM2COL_LD, self.shift, self.scale)
        taps = []
        for n, e in enumerate(self.layers):
            if n in (1, 2):
                h = L.maxpool3s2_nhwc(h)
            h = L.conv2d_nhwc(h, e["w"], e["co"], e["k"], e["k"], bias=e["b"], act_out=L.ACT_RELU)
            taps.append(h)
        return taps

    def __call__(self, in0, in1):
        """Distances of image pairs, each (3, H, W) or (N, 3, H, W) -> (N,) tensor on the device (lpips returns (N, 1, 1, 1))."""
        a = in0.to(self.device, torch.float32)
        b = in1.to(self.device, torch.float32)
        if a.dim() == 3:
            a, b = a[None], b[None]
        n = a.shape[0]
        taps = self.features(torch.cat([a, b], 0))
        dist = torch.empty(n, dtype=torch.float32, device=self.device)
        for i, t in enumerate(taps):
            L.lpips_layer(t[:n], t[n:], self.lins[i], dist, accumulate=i > 0)
        return dist


# ---- the whole family: VGG16, SqueezeNet 1.1 and AlexNet under one pixel-parallel head, with spatial maps -----------------------
#
# ``models/networks_basic.py:25-88`` (``PNetLin``) takes ``vgg``, ``alex`` and ``squeeze``; ``models/pretrained_networks.py:5-134``
# cuts torchvision's ``features`` into the slices whose ReLU outputs are the taps; ``weights/v0.1/{alex,vgg,squeeze}.pth`` hold
# the trained linear layers.  The benchmark's metric is the spatial form (``fvd_utils/calculate_lpips.py:9-58``):
# ``lpips.LPIPS(net=..., spatial=True)`` on frames mapped to [-1, 1], ``.mean()`` of the map.

NETS = ("alex", "vgg", "squeeze")
CHANNELS = {"alex": (64, 192, 384, 256, 256), "vgg": (64, 128, 256, 512, 512), "squeeze": (64, 128, 256, 384, 384, 512, 512)}
# torchvision.models.vgg16().features: (index, Ci, Co) of the 3x3 pad-1 convolutions, MaxPool2d(2, 2) before the listed indices
# (it sits at 4, 9, 16, 23), taps after the ReLUs of the listed convolutions
VGG_CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256), (17, 256, 512),
             (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512))
VGG_POOL_BEFORE = (5, 10, 17, 24)
VGG_TAPS = (2, 7, 14, 21, 28)
# torchvision.models.squeezenet1_1().features: 0 = Conv2d(3, 64, 3, stride=2), 1 = ReLU, MaxPool2d(3, 2, ceil_mode=True) at
# 2, 5, 8 (i.e. before Fire 3, 6, 9), Fire (index, in, squeeze, expand) with expand1x1 || expand3x3; taps after 1, 4, 7, 9 .. 12
SQUEEZE_FIRES = ((3, 64, 16, 64), (4, 128, 16, 64), (6, 128, 32, 128), (7, 256, 32, 128), (9, 256, 48, 192), (10, 384, 48, 192),
                 (11, 384, 64, 256), (12, 512, 64, 256))
SQUEEZE_POOL_BEFORE = (3, 6, 9)
SQUEEZE_TAPS = (4, 7, 9, 10, 11, 12)
_IM2COL3_LD = 32                                       # 3 * 3 * 3 = 27 patch entries, padded to a multiple of 16
# activation bytes per input pixel and image that one backbone pass keeps alive at its peak, rounded up: VGG holds the taps
# (64 + 128/4 + 256/16 + 512/64 + 512/256 channels' worth = 488 B), the im2col rows (128 B) and one more 64-channel tensor (256 B)
_BYTES_PER_PIXEL = {"vgg": 1024, "squeeze": 256, "alex": 256}
_ACTIVATION_BUDGET = 1 << 30


def _slice_of(net, idx):
    """The ``net.slice<K>`` a saved ``lpips.LPIPS`` module keeps ``features[idx]`` in (pretrained_networks.py)."""
    if net == "alex":
        return _SLICE_KEYS[idx].split(".")[1]
    bounds = (4, 9, 16, 23, 30) if net == "vgg" else (2, 5, 8, 10, 11, 12, 13)
    return "slice%d" % (1 + next(i for i, b in enumerate(bounds) if idx < b))


def parse_spec(spec, net=None):
    """``[NET:]BACKBONE.pth,LIN.pth`` or ``[NET:]ONE_SAVED_STATE_DICT.pth`` -> (net, [paths]).  Every file must exist:
    ``FileNotFoundError`` names the first that does not, before anything touches the device."""
    import os
    head, sep, rest = spec.partition(":")
    if sep and head in NETS:
        net, spec = head, rest
    elif net is None:
        raise ValueError(f"LPIPS spec {spec!r}: expected NET:BACKBONE.pth,LIN.pth with NET one of {', '.join(NETS)}")
    if net not in NETS:
        raise ValueError(f"LPIPS network {net!r}: one of {', '.join(NETS)}")
    paths = [p.strip() for p in spec.split(",")]
    if len(paths) not in (1, 2) or not all(paths):
        raise ValueError(f"LPIPS spec {spec!r}: one saved state dict, or BACKBONE.pth,LIN.pth")
    for p in paths:
        if not os.path.isfile(p):
            raise FileNotFoundError(f"LPIPS ({net}) weight file {p}: no such file")
    return net, paths


class Lpips:
    """``lpips.LPIPS(net=net)`` for ``net`` in ``alex`` / ``vgg`` / ``squeeze``: distances (``net(in0, in1)``), spatial maps
    (``spatial_map``, lpips' ``spatial=True``) and taps (``features``), on the pixel-parallel head (``evc_lpips_map_f32``)."""

    def __init__(self, net, state_dict, device=None, max_pairs=None):
        if net not in NETS:
            raise ValueError(f"LPIPS network {net!r}: one of {', '.join(NETS)}")
        L.hip_lib()                                                  # fails loudly without the HIP library / a gfx950 device
        self.net = net
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.arith = L.default_arith()
        self.max_pairs = max_pairs
        dev = self.device
        self.shift = torch.tensor(SHIFT, dtype=torch.float32, device=dev)
        self.scale = torch.tensor(SCALE, dtype=torch.float32, device=dev)
        sd = state_dict
        self.convs = {}
        if net == "alex":
            for idx, ci, co, k, _, _ in CONVS:
                self._load(sd, idx, "", co, ci, k, _IM2COL_LD if idx == 0 else 0)
        elif net == "vgg":
            for idx, ci, co in VGG_CONVS:
                self._load(sd, idx, "", co, ci, 3, _IM2COL3_LD if idx == 0 else 0)
        else:
            self._load(sd, 0, "", 64, 3, 3, _IM2COL3_LD)
            for idx, ci, sq, ex in SQUEEZE_FIRES:
                self._load(sd, idx, ".squeeze", sq, ci, 1)
                self._load(sd, idx, ".expand1x1", ex, sq, 1)
                self._load(sd, idx, ".expand3x3", ex, sq, 3)
        self.lins = []
        for i, co in enumerate(CHANNELS[net]):
            w = _find(sd, f"lin{i}.model.1.weight", f"lins.{i}.model.1.weight").detach().float().to(dev)
            if w.numel() != co:
                raise ValueError(f"lin{i}: expected {co} weights, got {tuple(w.shape)}")
            self.lins.append(w.reshape(-1).contiguous())

    def _load(self, sd, idx, sub, co, ci, k, im2col_ld=0):
        dev = self.device
        names = (f"features.{idx}{sub}", f"net.{_slice_of(self.net, idx)}.{idx}{sub}")
        w = _find(sd, *(n + ".weight" for n in names)).detach().float().to(dev)
        b = _find(sd, *(n + ".bias" for n in names)).detach().float().to(dev).contiguous()
        if tuple(w.shape) != (co, ci, k, k) or tuple(b.shape) != (co,):
            raise ValueError(f"features.{idx}{sub}: expected weight {(co, ci, k, k)}, got {tuple(w.shape)}")
        if im2col_ld:                                                # as a 1x1 convolution over the im2col rows
            wp = torch.zeros((co, im2col_ld, 1, 1), dtype=torch.float32, device=dev)
            wp[:, :ci * k * k, 0, 0] = w.reshape(co, -1)
            w, k = wp, 1
        self.convs[f"{idx}{sub}"] = dict(w=L.conv_pack_weights(w.contiguous(), self.arith), b=b, co=co, k=k)

    @classmethod
    def from_files(cls, net, backbone_path, lin_path=None, device=None, max_pairs=None):
        """torchvision's checkpoint of the backbone and lpips' ``weights/v0.1/<net>.pth``, or one saved ``lpips.LPIPS`` state
        dict alone, read with the weights-only loader."""
        sd = dict(torch.load(backbone_path, map_location="cpu", weights_only=True))
        if lin_path is not None:
            sd.update(torch.load(lin_path, map_location="cpu", weights_only=True))
        return cls(net, sd, device, max_pairs)

    @classmethod
    def from_spec(cls, spec, net=None, device=None, max_pairs=None):
        """``parse_spec`` + ``from_files``."""
        net, paths = parse_spec(spec, net)
        return cls.from_files(net, paths[0], paths[1] if len(paths) == 2 else None, device, max_pairs)

    def _conv(self, h, name, out=None):
        e = self.convs[name]
        return L.conv2d_nhwc(h, e["w"], e["co"], e["k"], e["k"], bias=e["b"], act_out=L.ACT_RELU, out=out)

    def features(self, x):
        """x: (N, 3, H, W) float32 on the device -> the ReLU taps, NHWC."""
        x = x.contiguous()
        taps = []
        if self.net == "alex":
            h = L.im2col_nchw(x, 11, 11, 4, 2, _IM2COL_LD, self.shift, self.scale)
            for n, (idx, *_) in enumerate(CONVS):
                if n in (1, 2):
                    h = L.maxpool2d_nhwc(h, 3, 2)
                h = self._conv(h, str(idx))
                taps.append(h)
        elif self.net == "vgg":
            h = L.im2col_nchw(x, 3, 3, 1, 1, _IM2COL3_LD, self.shift, self.scale)
            for idx, _, _ in VGG_CONVS:
                if idx in VGG_POOL_BEFORE:
                    h = L.maxpool2d_nhwc(h, 2, 2)
                h = self._conv(h, str(idx))
                if idx in VGG_TAPS:
                    taps.append(h)
        else:
            h = self._conv(L.im2col_nchw(x, 3, 3, 2, 0, _IM2COL3_LD, self.shift, self.scale), "0")
            taps.append(h)
            for idx, _, _, ex in SQUEEZE_FIRES:
                if idx in SQUEEZE_POOL_BEFORE:
                    h = L.maxpool2d_nhwc(h, 3, 2, ceil_mode=True)
                s = self._conv(h, f"{idx}.squeeze")
                h = torch.empty(s.shape[:3] + (2 * ex,), dtype=torch.float32, device=self.device)
                self._conv(s, f"{idx}.expand1x1", out=L.Cols(h, 0, ex))       # the two halves of one tensor: no concat
                self._conv(s, f"{idx}.expand3x3", out=L.Cols(h, ex, ex))
                if idx in SQUEEZE_TAPS:
                    taps.append(h)
        return taps

    def _pairs(self, in0, in1, normalize):
        a = in0.to(self.device, torch.float32)
        b = in1.to(self.device, torch.float32)
        if a.dim() == 3:
            a, b = a[None], b[None]
        if a.shape != b.shape or a.dim() != 4 or a.shape[1] != 3:
            raise ValueError(f"LPIPS takes pairs of (3, H, W) or (N, 3, H, W) images, got {tuple(in0.shape)} and {tuple(in1.shape)}")
        if normalize:                                                # lpips' flag; calculate_lpips.py:15-23
            a, b = a * 2 - 1, b * 2 - 1
        step = self.max_pairs or max(1, _ACTIVATION_BUDGET // (2 * a.shape[2] * a.shape[3] * _BYTES_PER_PIXEL[self.net]))
        for s in range(0, a.shape[0], step):
            n = min(step, a.shape[0] - s)
            taps = self.features(torch.cat([a[s:s + n], b[s:s + n]], 0))
            yield s, n, [(t[:n], t[n:]) for t in taps]

    def __call__(self, in0, in1, normalize=False):
        """Distances of image pairs, each (3, H, W) or (N, 3, H, W) -> (N,) tensor on the device (lpips returns (N, 1, 1, 1))."""
        dist = torch.empty(in0.shape[0] if in0.dim() == 4 else 1, dtype=torch.float32, device=self.device)
        for s, n, taps in self._pairs(in0, in1, normalize):
            for i, (t0, t1) in enumerate(taps):
                L.lpips_map_mean(L.lpips_map(t0, t1, self.lins[i]), dist[s:s + n], accumulate=i > 0)
        return dist

    def spatial_map(self, in0, in1, normalize=False):
        """lpips' ``spatial=True``: every tap's per-pixel distance up-sampled to the image size and summed -> (N, H, W)."""
        H, W = in0.shape[-2:]
        out = torch.empty((in0.shape[0] if in0.dim() == 4 else 1, H, W), dtype=torch.float32, device=self.device)
        for s, n, taps in self._pairs(in0, in1, normalize):
            for i, (t0, t1) in enumerate(taps):
                L.lpips_upsample_add(L.lpips_map(t0, t1, self.lins[i]), out[s:s + n], accumulate=i > 0)
        return out

    def spatial_mean(self, in0, in1, normalize=True):
        """The benchmark's value per pair (calculate_lpips.py:35-58): frames in [0, 1] mapped to [-1, 1], the spatial map, its
        mean -> (N,) tensor."""
        m = self.spatial_map(in0, in1, normalize)
        return L.lpips_map_mean(m, torch.empty(m.shape[0], dtype=torch.float32, device=self.device), accumulate=False)
