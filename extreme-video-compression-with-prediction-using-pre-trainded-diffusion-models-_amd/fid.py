"""FID and precision / recall on the HIP kernels: pytorch-fid's Inception-v3 feature network and the two set metrics.

The reference's ``evaluation/`` package computes the Frechet Inception distance (``fid_PR.py``: ``calculate_activations`` :110-167,
``calculate_frechet_distance`` :53-107) and the k-NN precision / recall of Kynkaanniemi et al. (``pr.py``) over the features of
``InceptionV3`` (``inception.py``): ``fid_inception_v3()`` (:184-208), i.e. torchvision's Inception-v3 with the patched blocks
``FIDInceptionA / C / E_1 / E_2`` (:211-328), cut into four blocks (:84-124) after a bilinear resize to 299 x 299 and ``2x - 1``
(:146-153).  ``inception.py`` only patches torchvision's classes; the module structure is restated here (``STEM``, ``MIXED``).
The network takes pytorch-fid's state dict ``pt_inception-2015-12-05-6726825d.pth`` in its own key names
(``Conv2d_1a_3x3.conv.weight``, ``Mixed_6b.branch7x7_2.bn.running_var``, ...; ``fc.*`` and ``num_batches_tracked`` are ignored).

Data path, activations NHWC: ``evc_inception_stem_im2col_f32`` (resize + 2x - 1 + the 3x3 stride-2 patches) -> 1x1 convolution;
every stride-1 "same" filter (1x1, 3x3, 5x5, 1x7, 7x1, 1x3, 3x1) directly on ``evc_conv2d_nhwc_f32`` where the dispatch takes the
shape (``lib.conv_accepts``), everything else (the unpadded and the stride-2 3x3 filters) as ``evc_im2col_nhwc_f32`` + 1x1
convolution with the weights permuted to (ky, kx, c) once; each branch writes its channel slice of the block's output;
``evc_pool3x3s1p1_nhwc_f32`` for the branch pools, ``evc_maxpool2d_nhwc_f32`` for the stride-2 ones, ``evc_spatial_mean_nhwc_f32``
at the end.  BatchNorm (eps = 0.001) is folded into weight and bias in fp64 at load time, ReLU runs in the epilogue, the
arithmetic follows EVC_CONV_ARITH with the exact bf16 split as the default (no bound on these operands is known), and every
convolution runs the batch-invariant plan: an image's features do not depend on the images it is batched with.
"""
import numpy as np
import torch

from . import lib as L

RES = L.INCEPTION_RES
BN_EPS = 1e-3                     # torchvision BasicConv2d: nn.BatchNorm2d(eps=0.001)
STEM_LD = 32                      # 3 * 3 * 3 = 27 patch entries, padded to a multiple of 16
BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}         # inception.py:23-28
WEIGHT_FILE = "pt_inception-2015-12-05-6726825d.pth"
MIXED_NAMES = ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a",
               "Mixed_7b", "Mixed_7c")
# (name, Ci, Co, (KH, KW), stride, (PH, PW)) of the stem's BasicConv2d units, torchvision Inception3.__init__
STEM = (("Conv2d_1a_3x3", 3, 32, (3, 3), 2, (0, 0)), ("Conv2d_2a_3x3", 32, 32, (3, 3), 1, (0, 0)),
        ("Conv2d_2b_3x3", 32, 64, (3, 3), 1, (1, 1)), ("Conv2d_3b_1x1", 64, 80, (1, 1), 1, (0, 0)),
        ("Conv2d_4a_3x3", 80, 192, (3, 3), 1, (0, 0)))
# Inception blocks: name -> (kind, Ci, parameter): A: pool_features, C: channels_7x7, E: the pool of its last branch
MIXED = {"Mixed_5b": ("A", 192, 32), "Mixed_5c": ("A", 256, 64), "Mixed_5d": ("A", 288, 64), "Mixed_6a": ("B", 288, None),
         "Mixed_6b": ("C", 768, 128), "Mixed_6c": ("C", 768, 160), "Mixed_6d": ("C", 768, 160), "Mixed_6e": ("C", 768, 192),
         "Mixed_7a": ("D", 768, None), "Mixed_7b": ("E", 1280, L.POOL_AVG), "Mixed_7c": ("E", 2048, L.POOL_MAX)}


def _branches(kind, ci, p):
    """[(branch name, Ci, Co, (KH, KW), stride, (PH, PW))] of one Inception block (torchvision InceptionA .. InceptionE)."""
    k1, k3, k5, k17, k71, k13, k31 = (1, 1), (3, 3), (5, 5), (1, 7), (7, 1), (1, 3), (3, 1)
    same = lambda k: (k[0] // 2, k[1] // 2)                                  # noqa: E731
    c = lambda n, i, o, k=k1, s=1, pad=None: (n, i, o, k, s, same(k) if pad is None else pad)       # noqa: E731
    if kind == "A":
        return [c("branch1x1", ci, 64), c("branch5x5_1", ci, 48), c("branch5x5_2", 48, 64, k5), c("branch3x3dbl_1", ci, 64),
                c("branch3x3dbl_2", 64, 96, k3), c("branch3x3dbl_3", 96, 96, k3), c("branch_pool", ci, p)]
    if kind == "B":
        return [c("branch3x3", ci, 384, k3, 2, (0, 0)), c("branch3x3dbl_1", ci, 64), c("branch3x3dbl_2", 64, 96, k3),
                c("branch3x3dbl_3", 96, 96, k3, 2, (0, 0))]
    if kind == "C":
        return [c("branch1x1", ci, 192), c("branch7x7_1", ci, p), c("branch7x7_2", p, p, k17), c("branch7x7_3", p, 192, k71),
                c("branch7x7dbl_1", ci, p), c("branch7x7dbl_2", p, p, k71), c("branch7x7dbl_3", p, p, k17),
                c("branch7x7dbl_4", p, p, k71), c("branch7x7dbl_5", p, 192, k17), c("branch_pool", ci, 192)]
    if kind == "D":
        return [c("branch3x3_1", ci, 192), c("branch3x3_2", 192, 320, k3, 2, (0, 0)), c("branch7x7x3_1", ci, 192),
                c("branch7x7x3_2", 192, 192, k17), c("branch7x7x3_3", 192, 192, k71), c("branch7x7x3_4", 192, 192, k3, 2, (0, 0))]
    return [c("branch1x1", ci, 320), c("branch3x3_1", ci, 384), c("branch3x3_2a", 384, 384, k13), c("branch3x3_2b", 384, 384, k31),
            c("branch3x3dbl_1", ci, 448), c("branch3x3dbl_2", 448, 384, k3), c("branch3x3dbl_3a", 384, 384, k13),
            c("branch3x3dbl_3b", 384, 384, k31), c("branch_pool", ci, 192)]


def conv_specs():
    """{key prefix: (Ci, Co, (KH, KW), stride, (PH, PW))} of every BasicConv2d of the four blocks, in the state dict's names."""
    out = {n: (ci, co, k, s, p) for n, ci, co, k, s, p in STEM}
    for name, (kind, ci, p) in MIXED.items():
        for n, i, o, k, s, pad in _branches(kind, ci, p):
            out[f"{name}.{n}"] = (i, o, k, s, pad)
    return out


def _out_side(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def flops_per_image():
    """2 FLOP per MAC of every convolution of the forward at 299 x 299, from the layer table."""
    specs = conv_specs()
    side, total = RES, 0
    mac = lambda name, h, w: h * w * specs[name][0] * specs[name][1] * specs[name][2][0] * specs[name][2][1]    # noqa: E731
    for name, _, _, k, s, p in STEM:
        side = _out_side(side, k[0], s, p[0])
        total += mac(name, side, side)
        if name in ("Conv2d_2b_3x3", "Conv2d_4a_3x3"):
            side = _out_side(side, 3, 2, 0)
    for name, (kind, ci, p) in MIXED.items():
        down = _out_side(side, 3, 2, 0)
        for n, _, _, _, s, _ in _branches(kind, ci, p):
            total += mac(f"{name}.{n}", *((down, down) if s == 2 else (side, side)))
        if kind in "BD":
            side = down
    return 2.0 * total


def load_state_dict(path):
    """Read pytorch-fid's weight file with the weights-only loader."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: expected a state dict, got {type(sd).__name__}")
    return sd


def fold_conv(sd, name, spec=None):
    """A BasicConv2d's (w, b) with its BatchNorm folded in, fp64: scale = gamma / sqrt(var + eps), w * scale, beta - mean * scale.
    Shapes are checked against the network definition; a missing key or a mismatch names the key."""
    ci, co, (kh, kw), _, _ = spec or conv_specs()[name]

    def get(key, shape):
        full = f"{name}.{key}"
        if full not in sd:
            raise KeyError(f"Inception state dict has no {full}")
        t = torch.as_tensor(sd[full]).detach().to("cpu", torch.float64)
        if tuple(t.shape) != shape:
            raise ValueError(f"Inception state dict: {full} has shape {tuple(t.shape)}, expected {shape}")
        return t

    w = get("conv.weight", (co, ci, kh, kw))
    gamma, beta = get("bn.weight", (co,)), get("bn.bias", (co,))
    mean, var = get("bn.running_mean", (co,)), get("bn.running_var", (co,))
    scale = gamma / torch.sqrt(var + BN_EPS)
    return w * scale.view(-1, 1, 1, 1), beta - mean * scale


def fold_state_dict(sd):
    """{name: (w, b)} fp64 for every convolution of the network: host only, raises before any device work.  Keys the four
    blocks do not use (``fc.*``, ``AuxLogits.*``, ``num_batches_tracked``) are ignored."""
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    return {name: fold_conv(sd, name, spec) for name, spec in conv_specs().items()}


class InceptionV3:
    """pytorch-fid's InceptionV3 (all four blocks) on the HIP kernels.  ``forward(images)``: (N, 3, H, W) in [0, 1] -> the block
    outputs [(N, 73, 73, 64), (N, 35, 35, 192), (N, 17, 17, 768)] NHWC and (N, 2048); ``max_images`` images run per pass."""

    def __init__(self, state_dict, device=None, max_images=16):
        folded = fold_state_dict(state_dict)                         # a bad state dict raises here, before any launch
        L.hip_lib()                                                  # fails loudly without the HIP library / a gfx950 device
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.arith = L.default_arith()
        self.max_images = max(1, int(max_images))
        self.convs, self._routes = {}, {}
        for name, (ci, co, k, s, p) in conv_specs().items():
            w, b = folded[name]
            self.convs[name] = dict(w=w.float(), b=b.float().contiguous().to(self.device), ci=ci, co=co, k=k, s=s, p=p, packed={})

    @classmethod
    def from_file(cls, path, device=None, **kw):
        return cls(load_state_dict(path), device, **kw)

    # ---- layers --------------------------------------------------------------------------------------------------
    def _packed(self, e, route):
        """The packed weights of a layer for a route, made on first use: "direct" (Co, Ci, KH, KW); "cols" the 1x1 convolution
        over im2col rows, (ky, kx, c) order; "stem" the same over the stem's (c, ky, kx) rows padded to STEM_LD."""
        if route not in e["packed"]:
            w, co = e["w"], e["co"]
            if route == "cols":
                w = w.permute(0, 2, 3, 1).reshape(co, -1, 1, 1)
            elif route == "stem":
                w2 = torch.zeros((co, STEM_LD, 1, 1))
                w2[:, :w[0].numel(), 0, 0] = w.reshape(co, -1)
                w = w2
            e["packed"][route] = L.conv_pack_weights(w.contiguous().to(self.device), self.arith)
        return e["packed"][route]

    def _direct(self, name, B, H, W):
        """Whether the layer runs on the convolution itself: a stride-1 "same" filter the dispatch accepts for this shape."""
        key = (name, B, H, W)
        if key not in self._routes:
            e = self.convs[name]
            (kh, kw), same = e["k"], e["s"] == 1 and e["p"] == (e["k"][0] // 2, e["k"][1] // 2)
            self._routes[key] = same and L.conv_accepts(B, H, W, e["ci"], e["co"], kh, kw, self.arith, invariant=True)
        return self._routes[key]

    def _conv(self, x, name, out=None):
        """A BasicConv2d on (N, H, W, C): convolution, folded BatchNorm, ReLU.  ``out``: a ``Cols`` slice of the block's output."""
        e = self.convs[name]
        B, H, W, _ = x.shape
        (kh, kw) = e["k"]
        if self._direct(name, B, H, W):
            return L.conv2d_nhwc(x, self._packed(e, "direct"), e["co"], kh, kw, bias=e["b"], act_out=L.ACT_RELU, out=out,
                                 invariant=True)
        rows = L.im2col_nhwc(x, kh, kw, (e["s"], e["s"]), e["p"])
        return L.conv2d_nhwc(rows, self._packed(e, "cols"), e["co"], 1, 1, bias=e["b"], act_out=L.ACT_RELU, out=out,
                             invariant=True)

    def _chain(self, x, block, names, out=None):
        for i, n in enumerate(names):
            x = self._conv(x, f"{block}.{n}", out=out if i == len(names) - 1 else None)
        return x

    def _stem(self, images, f0, nf):
        e = self.convs["Conv2d_1a_3x3"]
        rows = torch.empty((nf, L.INCEPTION_STEM_OUT, L.INCEPTION_STEM_OUT, STEM_LD), device=self.device, dtype=torch.float32)
        L.inception_stem_im2col(images, f0, rows)
        return L.conv2d_nhwc(rows, self._packed(e, "stem"), e["co"], 1, 1, bias=e["b"], act_out=L.ACT_RELU, invariant=True)

    def _mixed(self, x, name):
        kind, ci, p = MIXED[name]
        B, H, W, _ = x.shape
        widths = {"A": (64, 64, 96, p), "B": (384, 96, ci), "C": (192,) * 4, "D": (320, 192, ci), "E": (320, 768, 768, 192)}[kind]
        if kind in "BD":
            H, W = _out_side(H, 3, 2, 0), _out_side(W, 3, 2, 0)
        out = torch.empty((B, H, W, sum(widths)), device=self.device, dtype=torch.float32)
        at = [sum(widths[:i]) for i in range(len(widths))]
        cols = lambda i, c0=0, c=None: L.Cols(out, at[i] + c0, widths[i] if c is None else c)     # noqa: E731
        if kind == "A":
            self._chain(x, name, ["branch1x1"], cols(0))
            self._chain(x, name, ["branch5x5_1", "branch5x5_2"], cols(1))
            self._chain(x, name, ["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"], cols(2))
            self._chain(L.pool3x3s1p1_nhwc(x, L.POOL_AVG), name, ["branch_pool"], cols(3))
        elif kind == "B":
            self._chain(x, name, ["branch3x3"], cols(0))
            self._chain(x, name, ["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"], cols(1))
            L.affine_act(L.maxpool2d_nhwc(x, 3, 2), None, L.ACT_NONE, out=cols(2))
        elif kind == "C":
            self._chain(x, name, ["branch1x1"], cols(0))
            self._chain(x, name, ["branch7x7_1", "branch7x7_2", "branch7x7_3"], cols(1))
            self._chain(x, name, ["branch7x7dbl_1", "branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4", "branch7x7dbl_5"], cols(2))
            self._chain(L.pool3x3s1p1_nhwc(x, L.POOL_AVG), name, ["branch_pool"], cols(3))
        elif kind == "D":
            self._chain(x, name, ["branch3x3_1", "branch3x3_2"], cols(0))
            self._chain(x, name, ["branch7x7x3_1", "branch7x7x3_2", "branch7x7x3_3", "branch7x7x3_4"], cols(1))
            L.affine_act(L.maxpool2d_nhwc(x, 3, 2), None, L.ACT_NONE, out=cols(2))
        else:
            self._chain(x, name, ["branch1x1"], cols(0))
            t = self._conv(x, f"{name}.branch3x3_1")
            self._conv(t, f"{name}.branch3x3_2a", cols(1, 0, 384))
            self._conv(t, f"{name}.branch3x3_2b", cols(1, 384, 384))
            t = self._chain(x, name, ["branch3x3dbl_1", "branch3x3dbl_2"])
            self._conv(t, f"{name}.branch3x3dbl_3a", cols(2, 0, 384))
            self._conv(t, f"{name}.branch3x3dbl_3b", cols(2, 384, 384))
            self._chain(L.pool3x3s1p1_nhwc(x, p), name, ["branch_pool"], cols(3))
        return out

    def _forward_chunk(self, images, f0, nf, eps):
        x = self._stem(images, f0, nf)                               # Conv2d_1a_3x3: 299 -> 149
        x = self._conv(x, "Conv2d_2a_3x3")                           # -> 147
        x = self._conv(x, "Conv2d_2b_3x3")
        b0 = x = L.maxpool2d_nhwc(x, 3, 2)                           # -> 73, block 0
        x = self._conv(x, "Conv2d_3b_1x1")
        x = self._conv(x, "Conv2d_4a_3x3")                           # -> 71
        b1 = x = L.maxpool2d_nhwc(x, 3, 2)                           # -> 35, block 1
        b2 = None
        for name in MIXED_NAMES:
            x = self._mixed(x, name)
            if eps is not None:
                eps.setdefault(name, []).append(x)
            if name == "Mixed_6e":
                b2 = x                                               # block 2
        return [b0, b1, b2, L.spatial_mean_nhwc(x)]                  # block 3: AdaptiveAvgPool2d((1, 1))

    def forward(self, images, endpoints=False):
        """images: (N, 3, H, W) float32 in [0, 1] (any device).  -> the four block outputs; with ``endpoints=True`` also
        {Mixed_* name: (N, H', W', C) NHWC tensor}.  N is cut into chunks of ``max_images``."""
        images = torch.as_tensor(images).to(self.device, torch.float32).contiguous()
        if images.dim() != 4 or images.shape[1] != 3 or images.shape[0] < 1:
            raise ValueError(f"InceptionV3 expects images (N, 3, H, W), got {tuple(images.shape)}")
        eps = {} if endpoints else None
        chunks = [self._forward_chunk(images, f0, min(self.max_images, images.shape[0] - f0), eps)
                  for f0 in range(0, images.shape[0], self.max_images)]
        blocks = [torch.cat([c[i] for c in chunks]) if len(chunks) > 1 else chunks[0][i] for i in range(4)]
        if endpoints:
            return blocks, {k: torch.cat(v) if len(v) > 1 else v[0] for k, v in eps.items()}
        return blocks

    __call__ = forward


def features(images, net, dims=2048):
    """(N, 3, H, W) images in [0, 1] -> (N, dims) float32 numpy features: the block ``BLOCK_INDEX_BY_DIM[dims]``, a map reduced
    by its spatial mean (calculate_activations, fid_PR.py:155-162)."""
    if dims not in BLOCK_INDEX_BY_DIM:
        raise ValueError(f"dims must be one of {sorted(BLOCK_INDEX_BY_DIM)}, got {dims}")
    f = net.forward(images)[BLOCK_INDEX_BY_DIM[dims]]
    if f.dim() == 4:
        f = L.spatial_mean_nhwc(f)
    return f.cpu().numpy()


# ---- the set metrics ----------------------------------------------------------------------------------------------------
def frechet_distance(feats_a, feats_b):
    """calculate_frechet_distance (fid_PR.py:53-107) of the two feature sets' np.mean / np.cov(rowvar=False), float64:
    |mu_a - mu_b|^2 + Tr(S_a) + Tr(S_b) - 2 Tr sqrt(S_a S_b).  With the centred matrices A_c (n, d), B_c (m, d): S_a S_b =
    A_c^T (A_c B_c^T) B_c / ((n - 1)(m - 1)), whose non-zero eigenvalues are those of M^T M for M = A_c B_c^T / sqrt((n - 1)(m - 1)),
    so Tr sqrt(S_a S_b) is the nuclear norm of M: no d x d sqrtm, and exact in the rank-deficient case where the reference adds
    eps to the diagonals."""
    a, b = np.asarray(feats_a, dtype=np.float64), np.asarray(feats_b, dtype=np.float64)
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1] or len(a) < 2 or len(b) < 2:
        raise ValueError(f"frechet_distance needs two (n >= 2, d) feature sets of one width, got {a.shape} and {b.shape}")
    mu_a, mu_b = a.mean(axis=0), b.mean(axis=0)
    ac, bc = a - mu_a, b - mu_b
    n, m = len(a), len(b)
    tr_a, tr_b = np.square(ac).sum() / (n - 1), np.square(bc).sum() / (m - 1)
    cross = np.linalg.svd(ac @ bc.T, compute_uv=False).sum() / np.sqrt((n - 1.0) * (m - 1.0))
    return float(np.square(mu_a - mu_b).sum() + tr_a + tr_b - 2.0 * cross)


def precision_recall(feats_real, feats_gen, k=3, device=None):
    """calculate_precision_recall (pr.py:44-53) on ``evc_knn_radius_f32`` / ``evc_manifold_hits_f32``: precision = the share of
    generated rows inside some real row's k-NN ball, recall = the share of real rows inside some generated row's.  -> floats."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    r = torch.as_tensor(np.ascontiguousarray(feats_real, dtype=np.float32)).to(dev)
    g = torch.as_tensor(np.ascontiguousarray(feats_gen, dtype=np.float32)).to(dev)
    if r.dim() != 2 or g.dim() != 2 or r.shape[1] != g.shape[1]:
        raise ValueError(f"precision_recall needs two (n, d) feature sets of one width, got {tuple(r.shape)} and {tuple(g.shape)}")
    precision = int(L.manifold_hits(g, r, L.knn_radius(r, k)).sum()) / g.shape[0]
    recall = int(L.manifold_hits(r, g, L.knn_radius(g, k)).sum()) / r.shape[0]
    return precision, recall


def calculate_fid(images_a, images_b, net, dims=2048):
    """Two image sets (N, 3, H, W) / (M, 3, H, W) in [0, 1] -> the Frechet distance of their Inception features."""
    return frechet_distance(features(images_a, net, dims), features(images_b, net, dims))


def fid_and_pr(feats_real, feats_gen, k=3):
    """(FID, precision, recall) of two feature sets: what the CLI prints per job."""
    p, r = precision_recall(feats_real, feats_gen, k)
    return frechet_distance(feats_real, feats_gen), p, r
