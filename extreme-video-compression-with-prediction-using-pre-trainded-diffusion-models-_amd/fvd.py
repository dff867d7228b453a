"""FVD on the HIP kernels: the I3D feature network and the Frechet video distance the reference reports per job.

The reference's ``calculate_fvd`` (``city_sender.py:264-279``, called per (video, q, threshold) job at ``:575-589``) runs the
I3D detector on ``preprocess_single`` of each clip (``models/fvd/fvd.py``: bilinear resize of the shorter side to 224,
``align_corners=False``, the other side ``ceil``-ed, centre crop 224 x 224, ``(x - 0.5) * 2``) and takes the Frechet distance
of the two sets of 400 logits (``frechet_distance`` / ``compute_stats`` at the end of that file).  ``I3d`` is
``InceptionI3d(400, in_channels=3)`` of ``models/fvd/pytorch_i3d.py``; it takes a state dict in that module's key names
(``Conv3d_1a_7x7.conv3d.weight``, ``Mixed_4b.b1b.bn.running_var``, ``logits.conv3d.bias``, ...; a ``module.`` prefix is
stripped), i.e. the ``i3d_pretrained_400.pt`` the reference's commented-out loader reads.  Its TorchScript file
``i3d_torchscript.pt`` is refused: its parameter names cannot be mapped without running it.

Data path, activations NTHWC (B*T images): ``evc_i3d_stem_im2col_f32`` (resize + crop + scale + same padding + 7x7x7 stride-2
patches, in chunks of output frames) -> 1x1 convolution; ``evc_maxpool3d_same_nthwc_f32``; 1x1x1 units on
``evc_conv2d_nhwc_f32``, 3x3x3 units as ``evc_frame_taps_f32`` + 3x3 convolution; each Inception branch writes its channel
slice of the concat directly; ``evc_i3d_head_f32`` for the average pool, logits and the mean over windows.  BatchNorm is folded
into the convolutions in fp64 at load time, ReLU runs in the epilogue, arithmetic is the exact bf16 split (inputs are not
normalised), as for LPIPS.
"""
import math
import os
import zipfile

import numpy as np
import torch

from . import lib as L

RES = 224                      # preprocess_single's resolution
BN_EPS = 1e-5                  # nn.BatchNorm3d(eps=1e-5), pytorch_i3d.py:69
NUM_CLASSES = 400
STEM_K, STEM_S, STEM_CO = 7, 2, 64
STEM_LD = 1040                 # 3 * 7 * 7 * 7 = 1029 patch entries, padded to a multiple of 16
HEAD_KT = 2                    # AvgPool3d(kernel_size=[2, 7, 7], stride 1)
HEAD_HW = 7
# Inception modules: (name, Ci, (b0, b1a, b1b, b2a, b2b, b3b) widths) -- pytorch_i3d.py:226-275
MIXED = {
    "Mixed_3b": (192, (64, 96, 128, 16, 32, 32)),
    "Mixed_3c": (256, (128, 128, 192, 32, 96, 64)),
    "Mixed_4b": (480, (192, 96, 208, 16, 48, 64)),
    "Mixed_4c": (512, (160, 112, 224, 24, 64, 64)),
    "Mixed_4d": (512, (128, 128, 256, 24, 64, 64)),
    "Mixed_4e": (512, (112, 144, 288, 32, 64, 64)),
    "Mixed_4f": (528, (256, 160, 320, 32, 128, 128)),
    "Mixed_5b": (832, (256, 160, 320, 32, 128, 128)),
    "Mixed_5c": (832, (384, 192, 384, 48, 128, 128)),
}
# The end points in order: ("unit", name, Ci, Co, k) | ("pool", name, kernel, stride) | ("mixed", name)
LAYERS = (
    ("unit", "Conv3d_1a_7x7", 3, 64, 7),
    ("pool", "MaxPool3d_2a_3x3", (1, 3, 3), (1, 2, 2)),
    ("unit", "Conv3d_2b_1x1", 64, 64, 1),
    ("unit", "Conv3d_2c_3x3", 64, 192, 3),
    ("pool", "MaxPool3d_3a_3x3", (1, 3, 3), (1, 2, 2)),
    ("mixed", "Mixed_3b"), ("mixed", "Mixed_3c"),
    ("pool", "MaxPool3d_4a_3x3", (3, 3, 3), (2, 2, 2)),
    ("mixed", "Mixed_4b"), ("mixed", "Mixed_4c"), ("mixed", "Mixed_4d"), ("mixed", "Mixed_4e"), ("mixed", "Mixed_4f"),
    ("pool", "MaxPool3d_5a_2x2", (2, 2, 2), (2, 2, 2)),
    ("mixed", "Mixed_5b"), ("mixed", "Mixed_5c"),
)
FLOPS_PER_CLIP_30 = 105.5e9    # 2 FLOP per MAC, 30-frame clip (the layer table of the issue / README)
WEIGHT_FILE = "i3d_pretrained_400.pt"
# where the reference keeps the weights (models/fvd/, and the copies of the fvd package under fvd_utils/ and benchmark/)
WEIGHT_DIRS = ("models/fvd", "fvd_utils/models/fvd", "benchmark/fvd_utils/models/fvd")


def _pad16(n):
    return (n + 15) // 16 * 16


def unit_shapes():
    """{key prefix: (Ci, Co, k, has_bn)} of every Unit3D, in the reference module's names."""
    out = {}
    for e in LAYERS:
        if e[0] == "unit":
            out[e[1]] = (e[2], e[3], e[4], True)
        elif e[0] == "mixed":
            ci, (c0, c1a, c1b, c2a, c2b, c3) = MIXED[e[1]]
            for br, (i, o, k) in dict(b0=(ci, c0, 1), b1a=(ci, c1a, 1), b1b=(c1a, c1b, 3), b2a=(ci, c2a, 1),
                                      b2b=(c2a, c2b, 3), b3b=(ci, c3, 1)).items():
                out[f"{e[1]}.{br}"] = (i, o, k, True)
    out["logits"] = (1024, NUM_CLASSES, 1, False)
    return out


def preprocess_geometry(h, w, res=RES):
    """preprocess_single's resize target (Hr, Wr): the shorter side becomes ``res``, the other ``ceil(side * scale)``."""
    scale = res / min(h, w)
    return (res, math.ceil(w * scale)) if h < w else (math.ceil(h * scale), res)


def _is_torchscript(path):
    if not zipfile.is_zipfile(path):
        return False
    with zipfile.ZipFile(path) as z:
        return any(n.endswith("/constants.pkl") or "/code/" in n for n in z.namelist())


def load_state_dict(path):
    """Read ``i3d_pretrained_400.pt`` with the weights-only loader; refuses the reference's TorchScript detector."""
    if _is_torchscript(path):
        raise ValueError(f"{path} is a TorchScript archive (the reference's i3d_torchscript.pt?): not supported.  Its "
                         f"parameter names cannot be mapped onto InceptionI3d without running it, and nothing shows that it "
                         f"computes the same function; pass the state dict {WEIGHT_FILE} instead (DESIGN.md section 8)")
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: expected a state dict, got {type(sd).__name__}")
    return sd


def normalise_keys(state_dict):
    """Strip the ``module.`` prefix of a DataParallel state dict."""
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state_dict.items()}


def fold_unit(sd, name):
    """A Unit3D's (w, b) with its BatchNorm folded in, fp64: scale = gamma / sqrt(var + eps), w * scale, beta - mean * scale.
    The logits unit has a bias and no BatchNorm.  Shapes are checked against InceptionI3d(400); a mismatch names the key."""
    ci, co, k, bn = unit_shapes()[name]

    def get(key, shape):
        full = f"{name}.{key}"
        if full not in sd:
            raise KeyError(f"I3D state dict has no {full}")
        t = sd[full].detach().to("cpu", torch.float64)
        if tuple(t.shape) != shape:
            raise ValueError(f"I3D state dict: {full} has shape {tuple(t.shape)}, expected {shape}")
        return t

    w = get("conv3d.weight", (co, ci, k, k, k))
    if not bn:
        return w, get("conv3d.bias", (co,))
    gamma, beta = get("bn.weight", (co,)), get("bn.bias", (co,))
    mean, var = get("bn.running_mean", (co,)), get("bn.running_var", (co,))
    scale = gamma / torch.sqrt(var + BN_EPS)
    return w * scale.view(-1, 1, 1, 1, 1), beta - mean * scale


def find_i3d_weights(roots=(".",)):
    """``i3d_pretrained_400.pt`` where the reference keeps it, or None."""
    for root in roots:
        for sub in WEIGHT_DIRS:
            p = os.path.join(root, sub, WEIGHT_FILE)
            if os.path.isfile(p):
                return p
    return None


class I3d:
    """InceptionI3d(400) on the HIP kernels.  ``__call__(clips)``: (B, T, 3, H, W) in [0, 1] -> (B, 400) logits (what the
    reference's detector returns with ``return_features=True``).  ``max_clips`` clips run per pass; the stem's patch rows live
    in a workspace of at most ``stem_workspace_bytes``."""

    def __init__(self, state_dict, device=None, max_clips=8, stem_workspace_bytes=512 << 20):
        L.hip_lib()                                                  # fails loudly without the HIP library / a gfx950 device
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.arith = L.default_arith()
        self.max_clips = max(1, int(max_clips))
        self.stem_ws_bytes = int(stem_workspace_bytes)
        if self.stem_ws_bytes < (RES // STEM_S) ** 2 * STEM_LD * 4:
            raise ValueError("stem_workspace_bytes must hold at least one output frame of patch rows")
        sd = normalise_keys(state_dict)
        dev = self.device
        self.units = {}
        for name, (ci, co, k, bn) in unit_shapes().items():
            w, b = fold_unit(sd, name)
            w, b = w.float(), b.float()
            if name == "logits":
                self.head_w = w.reshape(co, ci).contiguous().to(dev)
                self.head_b = b.contiguous().to(dev)
                continue
            if k == STEM_K:                                          # a 1x1 convolution over the im2col rows
                w2 = torch.zeros((co, STEM_LD, 1, 1))
                w2[:, :ci * k ** 3, 0, 0] = w.reshape(co, -1)
                cop = co
            else:
                # intermediates (b1a / b2a) get Co padded to 16 with zero weights and bias: the padded channels are exact
                # zeros after the ReLU; the 3x3x3 unit that reads them takes zero weights there too
                cop = _pad16(co) if name.endswith(("b1a", "b2a")) else co
                cip = _pad16(ci)
                w2 = torch.zeros((cop, k, cip, k, k))
                w2[:co, :, :ci] = w.permute(0, 2, 1, 3, 4)           # (Co, Ci, kt, kh, kw) -> (Co, kt, Ci, kh, kw)
                w2 = w2.reshape(cop, k * cip, k, k)
                b = torch.cat([b, torch.zeros(cop - co)])
            self.units[name] = dict(w=L.conv_pack_weights(w2.contiguous().to(dev), self.arith), b=b.contiguous().to(dev),
                                    co=cop, k=1 if k == STEM_K else k)

    @classmethod
    def from_file(cls, path, device=None, **kw):
        return cls(load_state_dict(path), device, **kw)

    # ---- layers --------------------------------------------------------------------------------------------------
    def _conv(self, x, name, T, out=None):
        """A Unit3D on (B*T, H, W, C): 1x1x1 directly, 3x3x3 as frame taps + 3x3 convolution; ReLU in the epilogue."""
        e = self.units[name]
        if e["k"] == 3:
            x = L.frame_taps(x, T)
        return L.conv2d_nhwc(x, e["w"], e["co"], e["k"], e["k"], bias=e["b"], act_out=L.ACT_RELU, out=out)

    def _stem(self, clips):
        B, T, C, H, W = clips.shape
        Hr, Wr = preprocess_geometry(H, W)
        To = (T + sum(L.same_pad(T, STEM_K, STEM_S)) - STEM_K) // STEM_S + 1
        Ho = (RES + sum(L.same_pad(RES, STEM_K, STEM_S)) - STEM_K) // STEM_S + 1
        row_bytes = Ho * Ho * STEM_LD * 4
        nf_max = max(1, min(B * To, self.stem_ws_bytes // row_bytes))
        ws = torch.empty((nf_max, Ho, Ho, STEM_LD), device=self.device, dtype=torch.float32)
        e = self.units["Conv3d_1a_7x7"]
        y = torch.empty((B * To, Ho, Ho, STEM_CO), device=self.device, dtype=torch.float32)
        for f0 in range(0, B * To, nf_max):
            nf = min(nf_max, B * To - f0)
            rows = L.i3d_stem_im2col(clips, Hr, Wr, RES, STEM_K, STEM_S, f0, ws[:nf])
            L.conv2d_nhwc(rows, e["w"], STEM_CO, 1, 1, bias=e["b"], act_out=L.ACT_RELU, out=y[f0:f0 + nf])
        return y, To

    def _mixed(self, x, name, T):
        ci, (c0, c1a, c1b, c2a, c2b, c3) = MIXED[name]
        BT, H, W, _ = x.shape
        out = torch.empty((BT, H, W, c0 + c1b + c2b + c3), device=self.device, dtype=torch.float32)
        self._conv(x, f"{name}.b0", T, out=L.Cols(out, 0, c0))
        self._conv(self._conv(x, f"{name}.b1a", T), f"{name}.b1b", T, out=L.Cols(out, c0, c1b))
        self._conv(self._conv(x, f"{name}.b2a", T), f"{name}.b2b", T, out=L.Cols(out, c0 + c1b, c2b))
        p = L.maxpool3d_same_nthwc(x, T, (3, 3, 3), (1, 1, 1))
        self._conv(p, f"{name}.b3b", T, out=L.Cols(out, c0 + c1b + c2b, c3))
        return out

    def forward(self, clips, endpoints=False):
        """clips: (B, T, 3, H, W) float32 on the device, [0, 1].  -> (B, 400) logits; with ``endpoints=True`` also
        {end point name: (B, T', H', W', C) NTHWC tensor}."""
        clips = clips.to(self.device, torch.float32).contiguous()
        if clips.dim() != 5 or clips.shape[2] != 3:
            raise ValueError(f"I3d expects clips (B, T, 3, H, W), got {tuple(clips.shape)}")
        B = clips.shape[0]
        eps = {}
        x, T = self._stem(clips)
        if endpoints:
            eps["Conv3d_1a_7x7"] = x
        for e in LAYERS[1:]:
            if e[0] == "pool":
                x = L.maxpool3d_same_nthwc(x, T, e[2], e[3])
                T = (T + sum(L.same_pad(T, e[2][0], e[3][0])) - e[2][0]) // e[3][0] + 1
            elif e[0] == "unit":
                x = self._conv(x, e[1], T)
            else:
                x = self._mixed(x, e[1], T)
            if endpoints:
                eps[e[1]] = x
        if x.shape[1:3] != (HEAD_HW, HEAD_HW) or T < HEAD_KT:
            raise ValueError(f"I3D head needs {HEAD_KT} x {HEAD_HW} x {HEAD_HW} final maps, got T'={T}, {tuple(x.shape[1:3])}")
        logits = L.i3d_head(x, T, self.head_w, self.head_b, HEAD_KT)
        if endpoints:
            return logits, {k: v.view(B, -1, *v.shape[1:]) for k, v in eps.items()}
        return logits

    def __call__(self, clips):
        """(B, T, 3, H, W) in [0, 1] (any device) -> (B, 400) float32 logits on the device, ``max_clips`` clips per pass."""
        return torch.cat([self.forward(clips[i:i + self.max_clips]) for i in range(0, clips.shape[0], self.max_clips)])


# ---- the distance (host, float64) -----------------------------------------------------------------------------------
def compute_stats(feats):
    feats = np.asarray(feats, dtype=np.float64)
    return feats.mean(axis=0), np.cov(feats, rowvar=False)


def frechet_distance(feats_a, feats_b):
    """||mu_a - mu_b||^2 + tr(sigma_a + sigma_b - 2 sqrtm(sigma_a sigma_b)), real part (models/fvd/fvd.py)."""
    from scipy.linalg import sqrtm
    mu_a, sigma_a = compute_stats(feats_a)
    mu_b, sigma_b = compute_stats(feats_b)
    m = np.square(mu_a - mu_b).sum()
    with np.errstate(invalid="ignore", divide="ignore"):     # sqrtm's residual check divides by |A| = 0 for identical samples
        s, _ = sqrtm(np.dot(sigma_a, sigma_b), disp=False)
    return float(np.real(m + np.trace(sigma_a + sigma_b - s * 2)))


def features(videos, i3d):
    """(N, T, C, H, W) clips -> (N, 400) float64 logits; a clip that repeats an earlier one (``x.repeat(2, ...)``) is not run
    again."""
    uniq, index = [], []
    for v in videos:
        for j, u in enumerate(uniq):
            if v.shape == u.shape and torch.equal(v, u):
                index.append(j)
                break
        else:
            index.append(len(uniq))
            uniq.append(v)
    f = i3d(torch.stack(uniq)).double().cpu().numpy()
    return f[index]


def calculate_fvd(videos1, videos2, i3d):
    """city_sender.py:264-279: videos (B, T, C, H, W) in [0, 1] -> the Frechet distance of their I3D logits.  Both sets go
    through the network together and no clip is run twice."""
    assert videos1.shape == videos2.shape
    f = features(torch.cat([torch.as_tensor(videos1), torch.as_tensor(videos2)]).float(), i3d)
    return frechet_distance(f[:len(videos1)], f[len(videos1):])
