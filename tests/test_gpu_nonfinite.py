"""GPU tests of the non-finite contract (include/evc_hip.h): a NaN / inf input stays non-finite through every export, exactly
where torch makes it non-finite, and nowhere else.

Method: NaN, +inf and -inf are injected one value at a time at chosen positions and the kernel is compared with torch on the
same injected input (CPU, float64).  Two rules hold in every case:
- no swallowing: every element torch makes non-finite is non-finite in the kernel's output;
- no leaking: every element torch leaves finite is finite, and within the op's tolerance of test_gpu_ops.py.
Two documented exceptions may produce a larger non-finite set, each named where it is used and checked against its bound:
- a NaN element bound of the fp16-split kernels (conv_igemm.hip in_scale, attention.hip): the whole output is NaN by design;
- the polyphase stride-2 kernels: a zero-padded phase tap multiplies a NaN by 0, so the bound is torch's set dilated by one
  output pixel.
The large convolution dispatch shapes are not compared with an fp64 reference of the whole layer: the kernel runs on the clean
and on the injected input, and outside the footprint of the injected positions (dilated over the kernel window) the two outputs
are bitwise equal (the kernels are deterministic), inside it every output is non-finite."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rnd

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
BAD = [NAN, INF, -INF]
BAD_IDS = ["nan", "+inf", "-inf"]


@pytest.fixture(scope="module")
def L():
    import evc_amd  # noqa: F401
    from evc_amd import lib
    lib.hip_lib()
    return lib


@pytest.fixture(autouse=True)
def clean_events(L):
    """The injected values raise EVC_RANGE_NONFINITE in the sticky device word: no other test may see it."""
    L.range_events(reset=True)
    yield
    L.range_events(reset=True)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def check(got, ref, tol, what=""):
    """No swallowing, no leaking, finite elements within ``tol`` of ref's finite max magnitude."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, what
    bad_ref, bad_got = ~torch.isfinite(ref), ~torch.isfinite(got)
    assert bool(bad_ref.any()) or what.endswith("finite"), ("the injected value must reach the output", what)
    assert bool(bad_got[bad_ref].all()), ("swallowed", what, int((~bad_got & bad_ref).sum()))
    assert not bool(bad_got[~bad_ref].any()), ("leaked", what, int((bad_got & ~bad_ref).sum()))
    fin = ~bad_ref
    if bool(fin.any()):
        err = float((got[fin] - ref[fin]).abs().max() / (ref[fin].abs().max() + 1e-30))
        assert err < tol, (what, err)


def check_exact(got, ref, what=""):
    """Bit-exact ops (copies, max pools): the same values, NaN where torch has NaN."""
    np.testing.assert_array_equal(got.detach().cpu().numpy(), ref.detach().cpu().numpy(), err_msg=what)


# ----------------------------------------------------------------------------------------------------------------------
# sampler step kernels (csrc/elementwise.hip): NaN stays NaN, +-inf clamps to +-1 exactly as torch.clamp does
# ----------------------------------------------------------------------------------------------------------------------

K1, K2, C1, C2, SG = 1.3, 0.7, 0.4, 0.55, 0.2
LC = [55 / 24, -59 / 24, 37 / 24, -9 / 24]


def _clip(v, on):
    return v.clamp(-1, 1) if on else v


def _step_ops(L):
    """name -> (operand names, kernel(ops) -> tensor, torch reference(ops in float64) -> tensor)."""
    def ddpm(noise, clip):
        def k(o):
            y = o["x"].clone()
            L.ddpm_step(y, o["e"], o["z"] if noise else None, K1, K2, C1, C2, SG, clip)
            return y

        def r(o):
            y = C1 * _clip(K1 * (o["x"] - K2 * o["e"]), clip) + C2 * o["x"]
            return y + SG * o["z"] if noise else y
        return (["x", "e", "z"] if noise else ["x", "e"]), k, r

    def ddim(clip):
        def k(o):
            y = o["x"].clone()
            L.ddim_step(y, o["e"], K1, K2, C1, C2, clip)
            return y
        return ["x", "e"], k, lambda o: C1 * _clip(K1 * (o["x"] - K2 * o["e"]), clip) + C2 * o["e"]

    def pndm(clip):
        return (["x", "e"], lambda o: L.pndm_transfer(o["x"], o["e"], 0.1, 0.8, 1.1, clip),
                lambda o: _clip(o["x"] + 0.1 * (0.8 * o["x"] - 1.1 * o["e"]), clip))

    def lincomb(ws):
        names = [f"e{i}" for i in range(4)]
        return names, (lambda o: L.lincomb4([o[n] for n in names], ws)), (lambda o: sum(w * o[n] for w, n in zip(ws, names)))

    def scale(clamp):
        return (["x"], lambda o: L.scale_clamp(o["x"], 0.5, 0.5, clamp),
                lambda o: (o["x"] * 0.5 + 0.5).clamp(*clamp) if clamp else o["x"] * 0.5 + 0.5)

    ops = {f"ddpm_noise_clip{c}": ddpm(True, c) for c in (0, 1)}
    ops.update({f"ddpm_clip{c}": ddpm(False, c) for c in (0, 1)})
    ops.update({f"ddim_clip{c}": ddim(c) for c in (0, 1)})
    ops.update({f"pndm_clip{c}": pndm(c) for c in (0, 1)})
    ops["axpy"] = (["x", "e"], lambda o: L.axpy(o["x"], o["e"], -0.3), lambda o: o["x"] - 0.3 * o["e"])
    ops["lincomb4"] = lincomb(LC)
    ops["lincomb4_zero_weights"] = lincomb([0.5, 0.0, 2.0, 0.0])          # torch: 0 * NaN = NaN, 0 * inf = NaN
    ops["scale_clamp0"] = scale(None)
    ops["scale_clamp1"] = scale((0.0, 1.0))
    ops["gate_residual"] = (["a", "b", "x"], lambda o: L.gate_residual(o["a"], o["b"], o["x"]),
                            lambda o: o["a"] * torch.sigmoid(o["b"]) + o["x"])
    return ops


STEP_OPS = ["ddpm_noise_clip0", "ddpm_noise_clip1", "ddpm_clip0", "ddpm_clip1", "ddim_clip0", "ddim_clip1", "pndm_clip0",
            "pndm_clip1", "axpy", "lincomb4", "lincomb4_zero_weights", "scale_clamp0", "scale_clamp1", "gate_residual"]


@pytest.mark.parametrize("op", STEP_OPS)
def test_sampler_step_kernels(L, op):
    """Every operand separately, each bad value, at element 0, an interior element and the last element of a size that is
    not a multiple of 256 (1920 = 7.5 blocks)."""
    names, kern, ref_fn = _step_ops(L)[op]
    n = 1920
    base = {nm: rnd(400 + i, n) * 1.5 for i, nm in enumerate(["x", "e", "z", "a", "b", "e0", "e1", "e2", "e3"])}
    for nm in names:
        for v, vid in zip(BAD, BAD_IDS):
            ops = {k: base[k].clone() for k in names}
            for pos in (0, 1037, n - 1):
                ops[nm][pos] = v
            want = ref_fn({k: t.double() for k, t in ops.items()})
            got = kern({k: t.cuda() for k, t in ops.items()}).cpu()
            what = f"{op}: {vid} in {nm}"
            assert torch.equal(torch.isnan(got), torch.isnan(want)), what                   # NaN exactly where torch has NaN
            inf = torch.isinf(want)
            assert torch.equal(got[inf].double(), want[inf]), what                          # +-inf with torch's sign
            fin = torch.isfinite(want)
            assert bool(torch.isfinite(got[fin]).all()), what
            assert float((got[fin].double() - want[fin]).abs().max() / want[fin].abs().max()) < 1e-6, what


# ----------------------------------------------------------------------------------------------------------------------
# convolution: one case per kernel the dispatcher picks (kernel name read through L.CONV_PROFILE)
# ----------------------------------------------------------------------------------------------------------------------

# (B, H, W, C0, C1, Co, K, arith, splits asked, (kernel plain, kernel with GroupNorm + SiLU on load), splits the dispatcher
#  chooses, split-K workspace in use, what).  Kernel names: conv_igemm_kernel<TM, TN, mode>, conv_split_kernel<TM, TN, mode>,
#  conv_splitn_kernel<planes, TM, TN, mode>, conv_split_rr_kernel<planes, 2 = 128- / 4 = 256-pixel tiles, TN, mode>,
#  conv_wide_kernel<mode, 4 = W 128 / 3 = other widths, fused 1x1>; mode 0 = plain, 2 = GroupNorm + SiLU.
CONV_CASES = [
    (2, 6, 7, 32, 16, 48, 3, 0, 0, ("conv_igemm_kernel<1, 1, 0>", "conv_igemm_kernel<1, 1, 2>"), 3, True,
     "f32, 64-pixel tiles (TM 1), split-K"),
    (2, 64, 64, 32, 16, 64, 3, 0, 0, ("conv_igemm_kernel<2, 1, 0>", "conv_igemm_kernel<2, 1, 2>"), 3, True,
     "f32, 128-pixel tiles (TM 2), split-K"),
    (3, 8, 8, 96, 32, 128, 1, 1, 0, ("conv_split_kernel<1, 2, 0>", "conv_split_kernel<1, 2, 2>"), 1, False, "bf16x6 1x1"),
    (3, 8, 8, 96, 32, 128, 1, 2, 0, ("conv_splitn_kernel<2, 1, 2, 0>", "conv_splitn_kernel<2, 1, 2, 2>"), 1, False, "f16x3 1x1"),
    (256, 8, 8, 32, 16, 192, 3, 2, 0, ("conv_split_rr_kernel<2, 2, 3, 0>", "conv_split_rr_kernel<2, 2, 3, 2>"), 2, True,
     "row-reuse, 128-pixel tiles, W = 8: every tile spans two images; split-K"),
    (8, 128, 128, 16, 16, 64, 3, 2, 0, ("conv_split_rr_kernel<2, 4, 1, 0>", "conv_split_rr_kernel<2, 4, 1, 2>"), 1, False,
     "row-reuse, 256-pixel tiles"),
    (5, 128, 128, 96, 32, 128, 3, 2, 0, ("conv_split_rr_kernel<2, 2, 2, 0>", "conv_split_rr_kernel<2, 2, 2, 2>"), 1, True,
     "row-reuse, 128-pixel tiles, K-split tail (unsplit grid, tail slabs)"),
    (4, 128, 128, 32, 16, 192, 3, 2, 0, ("conv_wide_kernel<0, 4, false>", "conv_wide_kernel<2, 4, false>"), 1, False,
     "wide: exactly one round"),
    (5, 128, 128, 192, 0, 192, 3, 2, 0, ("conv_wide_kernel<0, 4, false>", "conv_wide_kernel<2, 4, false>"), 1, True,
     "wide: one round + K-split tail"),
    (9, 32, 32, 128, 64, 384, 3, 2, 0, ("conv_wide_kernel<0, 3, false>", "conv_wide_kernel<2, 3, false>"), 3, True,
     "wide: below one round, uniform 3-way split + combine"),
    (9, 64, 64, 256, 128, 192, 3, 2, 0, ("conv_wide_kernel<0, 3, false>", "conv_wide_kernel<2, 3, false>"), 2, True,
     "wide: two unequal K pieces (wide_cut) + combine"),
    (3, 8, 8, 32, 16, 192, 3, 2, 3, ("conv_splitn_kernel<2, 1, 3, 0>", "conv_splitn_kernel<2, 1, 3, 2>"), 3, True,
     "f16x3, forced splits = 3 (combine kernel)"),
]
CONV_IDS = ["igemm_tm1", "igemm_tm2", "split_1x1", "splitn_1x1", "rr128_w8", "rr256", "rr_tail", "wide_round", "wide_tail",
            "wide_uniform", "wide_cut", "forced_splits"]


def _chosen_splits(L, B, H, W, C0, C1, Co, K, arith, splits):
    """evc_conv_choose_splits for a plain call of this shape (host-side dispatch query, no launch)."""
    import ctypes
    d = ctypes.c_void_p(16)
    a = L.ConvArgs(d, d if C1 else None, C0, C1, C0, C1, None, None, L.ACT_NONE, d, None, d, Co, 1.0, L.ACT_NONE, d, Co,
                   B, H, W, Co, K, K, splits, None, arith, None)
    return L.hip_lib().evc_conv_choose_splits(ctypes.byref(a))


def _positions(B, H, W, C0, C1):
    """(b, y, x, source, channel) of the injected values: the last pixel of image 0, both sides of the 128- and 256-pixel tile
    boundaries, an image corner, a channel of the second concat source, the last pixel of the batch (inside a K-split tail)."""
    def pix(m):
        return m // (H * W), (m % (H * W)) // W, m % W
    M = B * H * W
    out = [(*pix(H * W - 1), 0, 1), (B - 1, 0, 0, 0, C0 - 1), (*pix(M - 1), 0, 2)]
    for m in (127, 128, 255, 256):
        if m < M:
            out.append((*pix(m), 0, m % C0))
    if C1:
        out.append((*pix(M // 2), 1, C1 - 1))
    return out


def _footprint(mask, K):
    """(B, H, W) bool -> outputs whose K x K window holds a masked input pixel."""
    return F.max_pool2d(mask.float()[:, None], K, stride=1, padding=K // 2)[:, 0] > 0


def _conv_run(L, x0, x1, wp, Co, K, **kw):
    """-> (result, (kernel name, split-K workspace in use)) of one conv2d_nhwc call."""
    prof = []
    L.CONV_PROFILE = prof
    try:
        r = L.conv2d_nhwc(x0, wp, Co, K, K, src1=x1, **kw)
    finally:
        L.CONV_PROFILE = None
    return r, (prof[0]["kernel"], prof[0]["split"])


@pytest.mark.parametrize("B,H,W,C0,C1,Co,K,arith,splits,knames,nsplit,ws,what", CONV_CASES, ids=CONV_IDS)
def test_conv_nonfinite_footprint(L, B, H, W, C0, C1, Co, K, arith, splits, knames, nsplit, ws, what):
    torch.manual_seed(0)
    assert _chosen_splits(L, B, H, W, C0, C1, Co, K, arith, splits) == nsplit, what
    if "wide_cut" in what:
        L.conv_set_option("wide_cut", 0)
        try:
            assert _chosen_splits(L, B, H, W, C0, C1, Co, K, arith, splits) == 1, what      # the 2 pieces are the cut
        finally:
            L.conv_set_option("wide_cut", 1)
    dev = "cuda"
    x0 = nhwc(rnd(410, B, C0, H, W)).to(dev)
    x1 = nhwc(rnd(411, B, C1, H, W)).to(dev) if C1 else None
    C = C0 + C1
    w = (rnd(412, Co, C, K, K) / np.sqrt(K * K * C)).to(dev)
    bias = (0.1 * rnd(413, Co)).to(dev)
    res = nhwc(rnd(414, B, Co, H, W)).to(dev)
    a, s = (1 + 0.2 * rnd(415, B, C)).to(dev), (0.3 * rnd(416, B, C)).to(dev)      # finite GroupNorm coefficients
    wp = L.conv_pack_weights(w, arith)
    pos = _positions(B, H, W, C0, C1)
    in_mask = torch.zeros(B, H, W, dtype=torch.bool)
    for b, y, x, _, _ in pos:
        in_mask[b, y, x] = True
    foot = _footprint(in_mask, K).cuda()
    modes = {"plain": dict(),
             "gn_silu": dict(coef=(a, s), act_in=L.ACT_SILU),
             "relu_in": dict(act_in=L.ACT_RELU),
             "relu_out": dict(act_out=L.ACT_RELU)}
    # after a ReLU on the output a -inf sum becomes 0, so only NaN is followed through act_out (its set is the footprint again)
    values = {"plain": BAD, "gn_silu": BAD, "relu_in": BAD, "relu_out": [NAN]}

    def inject(v):
        b0, b1 = x0.clone(), (x1.clone() if C1 else None)
        for b, y, x, src, c in pos:
            (b0 if src == 0 else b1)[b, y, x, c] = v
        return b0, b1
    for mode, mkw in modes.items():
        kw = dict(bias=bias, res=res, out_scale=0.70710678, splits=splits, **mkw)
        clean, kernel = _conv_run(L, x0, x1, wp, Co, K, **kw)
        if mode in ("plain", "gn_silu"):
            assert kernel == (knames[0] if mode == "plain" else knames[1], ws), (what, mode, kernel)
        for v in values[mode]:
            out, _ = _conv_run(L, *inject(v), wp, Co, K, **kw)
            tag = f"{what}, {mode}, {v}"
            if mode == "relu_in" and v == -INF:
                # torch: ReLU(-inf) = 0, nothing non-finite -- the same bits as zeros at those positions
                zero, _ = _conv_run(L, *inject(0.0), wp, Co, K, **kw)
                assert torch.equal(out, zero) and bool(torch.isfinite(out).all()), tag
                continue
            outside = ~foot[..., None].expand_as(out)
            assert torch.equal(out[outside], clean[outside]), tag                          # bitwise, outside the footprint
            assert not bool(torch.isfinite(out[~outside]).any()), tag                      # non-finite, inside
            L.range_events(reset=True)
    # a NaN in the residual: exactly that output element
    rb = res.clone()
    rb[B - 1, H - 1, 0, Co - 1] = NAN
    kw = dict(bias=bias, res=rb, out_scale=0.70710678, splits=splits, act_out=L.ACT_RELU)
    clean = L.conv2d_nhwc(x0, wp, Co, K, K, src1=x1, **{**kw, "res": res})
    out = L.conv2d_nhwc(x0, wp, Co, K, K, src1=x1, **kw)
    mask = torch.zeros_like(out, dtype=torch.bool)
    mask[B - 1, H - 1, 0, Co - 1] = True
    assert torch.equal(out[~mask], clean[~mask]) and bool(torch.isnan(out[mask]).all()), what
    # fused moments: a NaN in sample 0 only makes sample 0's moments non-finite, the other samples' are bitwise unchanged,
    # and the GroupNorm coefficients of them raise RANGE_NONFINITE
    if B > 1:
        kw = dict(bias=bias, res=res, out_scale=0.70710678, splits=splits, coef=(a, s), act_in=L.ACT_SILU, want_stats=True)
        (clean, st0), _ = _conv_run(L, x0, x1, wp, Co, K, **kw)
        b0 = x0.clone()
        b0[0, H // 2, W // 2, 1] = NAN
        (out, st), _ = _conv_run(L, b0, x1, wp, Co, K, **kw)
        assert torch.equal(out[1:], clean[1:]) and torch.equal(st[1:], st0[1:]), what
        assert not bool(torch.isfinite(st[0].double().sum(0)).any()), what
        L.range_events(reset=True)
        G = 32 if Co % 32 == 0 else 16
        L.gn_coeffs([st], H * W, G, 1e-5)
        assert L.range_events(reset=True) & L.RANGE_NONFINITE, what


def test_conv_nan_bound_poisons_the_whole_output_by_design(L):
    """Documented exception: an fp16-split operand scaled by a NaN element bound (conv_igemm.hip in_scale) -- every output is
    NaN, a superset of torch's set."""
    B, H, W, C, Co = 2, 8, 8, 32, 64
    x = nhwc(rnd(420, B, C, H, W)).cuda()
    x[1, 3, 4, 5] = NAN
    w = (rnd(421, Co, C, 3, 3) / np.sqrt(9 * C)).cuda()
    bound = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.moments_bound(L.chan_stats(x), 0, C, bound)
    out = L.conv2d_nhwc(x, L.conv_pack_weights(w, L.ARITH_F16X3), Co, 3, 3, in_bound=bound)
    assert bool(torch.isnan(out).all())
    assert L.range_events(reset=True) & L.RANGE_NONFINITE


# ----------------------------------------------------------------------------------------------------------------------
# stride-2 and ELIC layers
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("v", BAD, ids=BAD_IDS)
def test_conv5x5s2_and_deconv5x5s2_within_the_polyphase_bound(L, v):
    """Documented exception: the polyphase kernels multiply zero-padded phase taps by the input, so a NaN / inf may reach the
    outputs next to torch's set; the bound is torch's set dilated by one output pixel."""
    B, Ho, Wo, Ci, Co = 2, 6, 5, 32, 48
    x = rnd(430, B, Ci, 2 * Ho, 2 * Wo)
    w, b = rnd(431, Co, Ci, 5, 5) / np.sqrt(25 * Ci), 0.1 * rnd(432, Co)
    x[0, 3, 2 * Ho - 1, 2 * Wo - 1] = v
    x[1, 7, 4, 5] = v
    conv = L.Conv5x5s2(w.cuda(), b.cuda())
    got = nchw(conv(nhwc(x).cuda()))
    ref = F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=2)
    _check_dilated(got, ref, 2e-5, f"conv5x5s2 {v}")
    # compressai deconv: ConvTranspose2d(k 5, s 2, p 2, output_padding 1); weight (Ci, Co, 5, 5)
    xd = rnd(433, B, Ci, Ho, Wo)
    wd = rnd(434, Ci, Co, 5, 5) / np.sqrt(25 * Ci / 4)
    xd[0, 0, 0, 0] = v
    xd[1, Ci - 1, 3, 2] = v
    deconv = L.Deconv5x5s2(wd.cuda(), b.cuda())
    got = nchw(deconv(nhwc(xd).cuda()))
    ref = F.conv_transpose2d(xd.double(), wd.double(), b.double(), stride=2, padding=2, output_padding=1)
    _check_dilated(got, ref, 2e-5, f"deconv5x5s2 {v}")


def _check_dilated(got, ref, tol, what):
    got, ref = got.detach().cpu().double(), ref.double()
    bad_ref, bad_got = ~torch.isfinite(ref), ~torch.isfinite(got)
    assert bool(bad_ref.any()), what
    assert bool(bad_got[bad_ref].all()), ("swallowed", what)
    bound = F.max_pool2d(bad_ref.any(1, keepdim=True).double(), 3, stride=1, padding=1) > 0
    assert not bool((bad_got & ~bound.expand_as(bad_got)).any()), ("beyond the bound", what)
    fin = ~bad_got
    assert float((got[fin] - ref[fin]).abs().max() / ref[~bad_ref].abs().max()) < tol, what


@pytest.mark.parametrize("inverse", [False, True], ids=["gdn", "igdn"])
def test_gdn(L, inverse):
    """GDN mixes the channels of one pixel: a NaN poisons that pixel's channels, no other pixel.  (An inf is not followed:
    torch's x / sqrt(inf) is 0 in the pixel's other channels, while the split arithmetic of the channel mix turns inf into
    NaN there.)"""
    B, H, W, C = 2, 5, 6, 32
    beta = 1 + 0.1 * rnd(440, C).abs()
    gamma = 0.1 * rnd(441, C, C).abs() + 0.05 * torch.eye(C)
    g = L.GDN(beta.cuda(), gamma.cuda(), inverse=inverse)
    x = nhwc(rnd(442, B, C, H, W))
    ped = g.PEDESTAL
    bt = torch.clamp(beta.double(), min=(1e-6 + ped) ** 0.5) ** 2 - ped
    gmm = torch.clamp(gamma.double(), min=ped ** 0.5) ** 2 - ped
    xb = x.clone()
    xb[0, 0, 0, 3] = NAN
    xb[1, H - 1, W - 1, C - 1] = NAN
    got = g(xb.cuda()).cpu()
    xd = xb.double()
    norm = torch.sqrt(bt + (xd * xd) @ gmm.t())
    check(got, xd * norm if inverse else xd / norm, 2e-6, f"gdn inverse={inverse}")


# ----------------------------------------------------------------------------------------------------------------------
# upfirdn2d
# ----------------------------------------------------------------------------------------------------------------------

def upfirdn_ref(x, k, up, down, pad):
    """The zero-insertion form in torch: insert up - 1 zeros, pad, correlate with the flipped kernel, keep every down-th."""
    B, C, H, W = x.shape
    z = x.new_zeros(B, C, H * up, W * up)
    z[:, :, ::up, ::up] = x
    z = F.pad(z, (pad[0], pad[1], pad[0], pad[1]))
    kt = torch.flip(torch.as_tensor(k, dtype=x.dtype), [0, 1])[None, None].repeat(C, 1, 1, 1)
    return F.conv2d(z, kt, groups=C, stride=down)


# The up-2 / down-2 fast paths of evc_upfirdn2d_nhwc_f32 (fir_up2_nhwc_kernel, fir_down2_nhwc_kernel) need a 4x4 kernel, act
# NONE or SILU, pad (2, 1) with even H, W for up 2 and pad (1, 1) with H, W multiples of 4 for down 2 (csrc/fir.hip): 8 x 12
# meets both; ReLU on those shapes and the odd 9 x 10 cases run the generic kernel.
@pytest.mark.parametrize("up,down,pad,kk,H,W", [(2, 1, (2, 1), 4, 8, 12), (1, 2, (1, 1), 4, 8, 12), (2, 1, (2, 1), 4, 9, 10),
                                                (3, 2, (2, 2), 5, 9, 10), (1, 1, (1, 1), 3, 9, 10)],
                         ids=["up2_fast", "down2_fast", "up2_generic_odd", "generic_up3_down2", "generic_1_1"])
def test_upfirdn2d(L, up, down, pad, kk, H, W):
    B, C = 2, 32
    k = (rnd(450, kk, kk).abs() + 0.1).numpy().astype(np.float32)
    x = rnd(451, B, C, H, W)
    a, s = 1 + 0.2 * rnd(452, B, C), 0.3 * rnd(453, B, C)
    acts = {L.ACT_NONE: lambda t: t, L.ACT_SILU: F.silu, L.ACT_RELU: F.relu}
    for v in BAD:
        xb = x.clone()
        xb[0, 3, 0, W - 1] = v                   # border pixel
        xb[1, C - 1, H // 2, W // 2] = v         # interior pixel
        xb[1, 5, H - 1, W - 1] = v               # the last pixel: the last block of the fast paths
        got = L.upfirdn2d_nchw(xb.cuda(), k, up=up, down=down, pad=pad)
        check(got, upfirdn_ref(xb.double(), k, up, down, pad), 5e-6, f"nchw {up} {down} {v}")
        for act, fn in acts.items():
            for coef in (None, (a, s)):
                pre = xb.double() if coef is None else xb.double() * a.double()[:, :, None, None] + s.double()[:, :, None, None]
                ref = upfirdn_ref(fn(pre), k, up, down, pad)
                got = L.upfirdn2d_nhwc(nhwc(xb).cuda(), k, up, down, pad,
                                       coef=None if coef is None else (a.cuda(), s.cuda()), act=act)
                what = f"nhwc up {up} down {down} act {act} coef {coef is not None} {v}"
                if act == L.ACT_RELU and v == -INF:
                    what += " finite"
                check(nchw(got), ref, 5e-6, what)


# ----------------------------------------------------------------------------------------------------------------------
# norm
# ----------------------------------------------------------------------------------------------------------------------

def test_affine_act(L):
    B, H, W, C = 2, 5, 7, 48
    x = nhwc(rnd(460, B, C, H, W))
    a, s = 1 + 0.2 * rnd(461, B, C), 0.3 * rnd(462, B, C)
    fns = {L.ACT_NONE: lambda t: t, L.ACT_SILU: F.silu, L.ACT_RELU: F.relu}
    for act, fn in fns.items():
        for v in BAD:
            xb = x.clone()
            xb[0, 0, 0, 0] = v
            xb[1, H - 1, W - 1, C - 1] = v
            xb[1, 2, 3, 17] = v
            got = L.affine_act(xb.cuda(), (a.cuda(), s.cuda()), act)
            ref = fn(xb.double() * a.double()[:, None, None, :] + s.double()[:, None, None, :])
            check(got, ref, 1e-6, f"affine_act {act} {v}" + (" finite" if act == L.ACT_RELU and v == -INF else ""))


def test_spade_act(L):
    B, H, W, C = 2, 4, 6, 32
    x = rnd(470, B, H, W, C)
    a, s = 1 + 0.2 * rnd(471, B, C), 0.3 * rnd(472, B, C)
    maps = torch.cat([1 + 0.1 * rnd(473, B, H, W, C), 0.1 * rnd(474, B, H, W, C)], -1)
    for where in ("x", "gamma", "beta"):
        for v in BAD:
            xb, mb = x.clone(), maps.clone()
            if where == "x":
                xb[1, 2, 3, 4] = v
            else:
                mb[0, 1, 5, (0 if where == "gamma" else C) + 7] = v
            got = L.spade_act(xb.cuda().contiguous(), (a.cuda(), s.cuda()), mb.cuda().contiguous(), C, act=L.ACT_SILU)
            xd, md = xb.double(), mb.double()
            n = xd * a.double()[:, None, None, :] + s.double()[:, None, None, :]
            ref = F.silu(n * md[..., :C] + md[..., C:])
            check(got, ref, 1e-6, f"spade {where} {v}")


def test_chan_stats_and_gn_coeffs_localise_a_nan_to_its_sample(L):
    """cat[h (96 ch), skip (64 ch)] in 32 groups of 5 (groups straddle the tensors), a NaN in sample 1 of the second tensor:
    sample 1's coefficients are non-finite in its groups only... and the other samples' are bitwise unchanged."""
    B, H, W = 3, 8, 8
    h, sk = nhwc(rnd(480, B, 96, H, W)).cuda(), nhwc(rnd(481, B, 64, H, W)).cuda()
    ca0, cs0 = L.gn_coeffs([L.chan_stats(h), L.chan_stats(sk)], H * W, 32, 1e-5)
    assert L.range_events(reset=True) == 0
    skb = sk.clone()
    skb[1, 2, 3, 0] = NAN                           # channel 96 of the concat: group 19 (channels 95 .. 99)
    ca, cs = L.gn_coeffs([L.chan_stats(h), L.chan_stats(skb)], H * W, 32, 1e-5)
    assert L.range_events(reset=True) & L.RANGE_NONFINITE
    others = [0, 2]
    assert torch.equal(ca[others], ca0[others]) and torch.equal(cs[others], cs0[others])
    g = torch.arange(160) // 5
    bad = (~torch.isfinite(ca[1].cpu())) | (~torch.isfinite(cs[1].cpu()))
    assert bool(bad[g == 19].all())
    assert torch.equal(ca[1].cpu()[g != 19], ca0[1].cpu()[g != 19])


# ----------------------------------------------------------------------------------------------------------------------
# attention
# ----------------------------------------------------------------------------------------------------------------------

def attn_ref(qkv, C, heads):
    B, N, _ = qkv.shape
    D = C // heads
    q, k, v = [t.reshape(B, N, heads, D).permute(0, 2, 1, 3) for t in qkv.double().split(C, dim=2)]
    w = torch.softmax(torch.einsum("bhqd,bhkd->bhqk", q, k) * (D ** -0.5), dim=-1)
    return torch.einsum("bhqk,bhkd->bhqd", w, v).permute(0, 2, 1, 3).reshape(B, N, C)


@pytest.mark.parametrize("B,heads,N,D", [(1, 2, 64, 64), (2, 2, 96, 32), (1, 2, 200, 192)], ids=["single", "ragged", "key_split"])
def test_attention_f32(L, B, heads, N, D):
    """A NaN in query row n poisons that row of that head; in key row n the whole head; in v[n, d] column d of the head; a
    +inf query element gives rows of +-inf scores (torch: NaN rows)."""
    C = heads * D
    lib = L.hip_lib()
    qkv = rnd(490, B, N, 3 * C)
    h = heads - 1
    cases = {"q row": (B - 1, N - 1, h * D + 3), "k row": (0, N // 2, C + h * D), "v element": (0, 5, 2 * C + h * D + D - 1),
             "q first": (0, 0, 0)}
    for name, (b, n, c) in cases.items():
        for v in BAD:
            x = qkv.clone()
            x[b, n, c] = v
            got = L.attention(x.cuda(), C, heads)
            check(got, attn_ref(x, C, heads), 2e-5, f"attention {name} {v}")
            if lib.evc_attention_workspace_bytes(B, heads, N, D) > 0:                 # the key-split plan: also single pass
                import ctypes
                out1 = torch.empty(B, N, C, device="cuda")
                xc = x.cuda()
                base = xc.data_ptr()
                assert lib.evc_attention_f32(ctypes.c_void_p(base), ctypes.c_void_p(base + 4 * C), ctypes.c_void_p(base + 8 * C),
                                             3 * C, L.fptr(out1), C, B, heads, N, D, D ** -0.5, L.stream_ptr()) == 0
                check(out1, attn_ref(x, C, heads), 2e-5, f"attention single pass {name} {v}")


def test_attention_f16x3_nan_bound_poisons_the_whole_output_by_design(L):
    """Documented exception (attention.hip): a NaN element bound makes every output NaN -- through the kv-planes pre-pass."""
    B, heads, N, D = 1, 2, 576, 192
    C = heads * D
    qkv = rnd(491, B, N, 3 * C)
    qkv[0, 7, 2 * C + 5] = NAN
    qkv = qkv.cuda()
    bounds = torch.zeros(3, dtype=torch.int32, device="cuda")
    L.moments_bound(L.chan_stats(qkv.view(B, 1, N, 3 * C)), 0, C, bounds)
    out = L.attention(qkv, C, heads, bounds=bounds)
    assert bool(torch.isnan(out).all())


# ----------------------------------------------------------------------------------------------------------------------
# frame kernels (pseudo-3-D network)
# ----------------------------------------------------------------------------------------------------------------------

def _video(seed, B, N, H, W, C):
    v = rnd(seed, B, N, H, W, C)
    return v.reshape(B * N, H, W, C), v


def test_frame_kernels(L):
    B, N, H, W, C, G, heads = 2, 5, 3, 4, 32, 8, 2
    x, _ = _video(500, B, N, H, W, C)
    gamma, beta = 1 + 0.1 * rnd(501, C), 0.1 * rnd(502, C)
    wm, bm = rnd(503, 3, N) / np.sqrt(N), 0.1 * rnd(504, 3)
    qkv, _ = _video(505, B, N, H, W, 3 * C)
    D = C // heads
    for val in BAD:
        xb = x.clone()
        xb[N + 2, 1, 2, 9] = val                    # sample 1, frame 2
        v = xb.reshape(B, N, H, W, C).double()
        # group norm over (C / G channels x N frames) of one pixel
        ref = F.group_norm(v.permute(0, 2, 3, 4, 1).reshape(B * H * W, C, N), G, gamma.double(), beta.double(), 1e-6)
        got = L.frame_group_norm(xb.cuda(), N, gamma.cuda(), beta.cuda(), G, 1e-6)
        check(got.cpu().reshape(B, N, H, W, C).permute(0, 2, 3, 4, 1).reshape(B * H * W, C, N), ref, 2e-6, f"frame_gn {val}")
        ref = torch.einsum("bnhwc,mn->bmhwc", v, wm.double()) + bm.double()[None, :, None, None, None]
        got = L.frame_mix(xb.cuda(), N, wm.cuda(), bm.cuda())
        check(got.cpu().reshape(B, 3, H, W, C), ref, 2e-6, f"frame_mix {val}")
        taps = L.frame_taps(xb.cuda(), N).cpu().reshape(B, N, H, W, 3, C)
        z = torch.zeros(B, 1, H, W, C, dtype=torch.float32)
        xf = xb.reshape(B, N, H, W, C)
        check_exact(taps, torch.stack([torch.cat([z, xf[:, :-1]], 1), xf, torch.cat([xf[:, 1:], z], 1)], 4), f"frame_taps {val}")
        qb = qkv.clone()
        qb[N + 1, 2, 0, 2 * C + 3] = val            # v of sample 1, frame 1
        qb[1, 0, 3, 4] = val                        # q of sample 0, frame 1
        qd = qb.reshape(B, N, H, W, 3 * C).permute(0, 2, 3, 4, 1).reshape(B * H * W, 3 * C, N).double()
        q, k, vv = (qd[:, j * C:(j + 1) * C].reshape(-1, D, N) for j in range(3))
        w = torch.softmax(torch.einsum("bct,bci->bti", q, k) * (int(D) ** (-0.5)), dim=-1)
        ref = torch.einsum("bti,bci->bct", w, vv).reshape(B * H * W, C, N)
        got = L.frame_attention(qb.cuda(), N, C, heads)
        check(got.cpu().reshape(B, N, H, W, C).permute(0, 2, 3, 4, 1).reshape(B * H * W, C, N), ref, 2e-6, f"frame_attn {val}")


# ----------------------------------------------------------------------------------------------------------------------
# LPIPS and I3D
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("v", BAD, ids=BAD_IDS)
def test_maxpools_keep_nan_bit_exactly(L, v):
    import i3d_recipe as R
    f = rnd(510, 2, 64, 9, 11)
    f[0, 3, 4, 4] = v                       # inside two windows
    f[1, 63, 8, 10] = v                     # the last pixel
    f[1, 10, 0, 0] = NAN                    # a NaN next to the bad value's window
    got = L.maxpool3s2_nhwc(nhwc(f).cuda()).cpu()
    check_exact(nchw(got), F.max_pool2d(f, 3, 2), f"maxpool3s2 {v}")
    for kernel, stride, shape in (((1, 3, 3), (1, 2, 2), (1, 5, 13, 9, 8)), ((3, 3, 3), (2, 2, 2), (2, 7, 9, 13, 4)),
                                  ((2, 2, 2), (2, 2, 2), (1, 5, 7, 11, 4))):
        B, T, H, W, C = shape
        x = -torch.rand(shape) - 0.5                 # negative: the zero same-padding wins at the borders
        x[0, 0, 0, 0, 0] = v
        x[B - 1, T - 1, H - 1, W - 1, C - 1] = v
        x[0, T // 2, H // 2, W // 2, 1] = NAN
        got = L.maxpool3d_same_nthwc(x.view(B * T, H, W, C).cuda(), T, kernel, stride).cpu()
        xc = x.permute(0, 4, 1, 2, 3)
        ref = F.max_pool3d(F.pad(xc, R.same_pad_args((T, H, W), kernel, stride)), kernel, stride).permute(0, 2, 3, 4, 1)
        check_exact(got.view(ref.shape), ref, f"maxpool3d {kernel} {v}")


def test_lpips_distance_of_a_nan_frame_is_nan(L):
    import evc_amd  # noqa: F401
    from evc_amd.lpips import LpipsAlex
    from evc_amd.policy import CallableMetric
    from oracle import lpips as OL
    from conftest import golden
    lin = golden("lpips_alex_lin")
    sd = OL.seeded_state_dict(5, lin)
    net = LpipsAlex(sd)
    a = torch.rand(3, 3, 64, 64, generator=torch.Generator().manual_seed(3))
    b = (a + 0.1 * rnd(511, 3, 3, 64, 64)).clamp(0, 1)
    clean = net(a.cuda(), b.cuda()).cpu()
    bn = b.clone()
    bn[1, 2, 40, 21] = NAN
    got = net(a.cuda(), bn.cuda()).cpu()
    want = OL.distance({k: v.double() for k, v in sd.items()}, a.double(), bn.double())
    assert bool(torch.isnan(want[1])) and bool(torch.isnan(got[1]))
    assert torch.equal(got[[0, 2]], clean[[0, 2]])
    assert CallableMetric.accept(float(got[1]), 0.5) is False


def test_i3d_logits_of_a_nan_clip_are_nan(L):
    import i3d_recipe as R
    import evc_amd  # noqa: F401
    from evc_amd import fvd
    net = fvd.I3d(R.seeded_state_dict(), device="cuda:0")
    clips = torch.stack([R.clip(31, 16, 64, 64), R.clip(32, 16, 64, 64)])
    clean = net(clips).cpu()
    single = net(clips[1:]).cpu()
    bad = clips.clone()
    bad[0, 5, 1, 30, 17] = NAN
    got = net(bad).cpu()
    assert bool(torch.isnan(got[0]).all())
    assert torch.equal(got[1], clean[1])                                 # the same launch shapes: bitwise
    assert float((got[1] - single[0]).abs().max() / single[0].abs().max()) <= 1e-5   # and the clip alone, as batching allows


# ----------------------------------------------------------------------------------------------------------------------
# sampler chains and the decoder
# ----------------------------------------------------------------------------------------------------------------------

class _StubNet:
    """What the samplers read of a score network: the schedule buffers.  The network itself is ``sampler._eps``, patched."""

    def __init__(self, sched):
        self.betas, self.alphas, self.alphas_prev = sched


def _stub_eps(shape, at_call, idx):
    """0.1 x, plus a NaN at element ``idx`` on call ``at_call``: elementwise, so torch's mask stays local."""
    state = {"n": 0}

    def eps(x):
        e = 0.1 * x
        if state["n"] == at_call:
            e = e.clone()
            e.view(-1)[idx] = NAN
        state["n"] += 1
        return e
    return eps


@pytest.mark.parametrize("name", ["DDPM", "DDIM", "FPNDM"])
def test_sampler_chains_keep_a_nan_from_the_network(L, monkeypatch, name):
    import evc_amd  # noqa: F401
    from evc_amd import sampler as S
    from oracle import samplers as OS, schedule as OSch
    sched = OSch.base_schedule()
    shape = (2, 15, 8, 8)
    x_T = rnd(520, *shape)
    noises = [rnd(521 + i, *shape) for i in range(12)]
    idx = 1234
    hip_eps = _stub_eps(shape, 1, idx)
    monkeypatch.setattr(S, "_eps", lambda net, x, label, cond: hip_eps(x))
    fn = S.get_sampler(name)
    kw = dict(subsample_steps=4, clip_before=True)
    if name != "FPNDM":
        kw.update(denoise=True)
    if name == "DDPM":
        kw["noise_fn"] = lambda i, x: noises[i].cuda()
    got = fn(x_T.cuda(), _StubNet(sched), final_only=True, **kw).cpu()
    ref_eps = _stub_eps(shape, 1, idx)
    okw = dict(kw)
    if name == "DDPM":
        okw["noise_fn"] = lambda i, x: noises[i]
    ofn = {"DDPM": OS.ddpm, "DDIM": OS.ddim, "FPNDM": OS.fpndm}[name]
    ref = ofn(x_T.clone(), lambda x, t: ref_eps(x), sched, **okw)
    assert bool(torch.isnan(ref).view(-1)[idx]), "the oracle must carry the NaN"
    assert torch.equal(torch.isfinite(got), torch.isfinite(ref)), name
    fin = torch.isfinite(ref)
    assert float((got[fin] - ref[fin]).abs().max() / ref[fin].abs().max()) < 1e-4, name


def _decoder_net():
    from oracle.scorenet import Dims, seeded_params
    from evc_amd.config import default_config
    from evc_amd.scorenet import ScoreNet
    d = Dims(ngf=32, n_head_channels=32, image_size=32)
    return ScoreNet(default_config(32, 32, 32), seeded_params(d, 91))


def _decoder(net, recovery):
    from evc_amd import sampler as S
    from evc_amd.config import default_config
    from evc_amd.decoder import ClipDecoder
    return ClipDecoder(net, None, default_config(32, 32, 32, subsample=3), S.get_sampler("DDPM"), range_recovery=recovery,
                       log=lambda s: None)


@pytest.mark.parametrize("at", ["mid", "last"])
def test_decoder_does_not_hide_a_nan_from_the_network(L, monkeypatch, at):
    """A NaN in the network's output at one evaluation of a chunk: with per-layer recovery the chunk is refused
    (NumericsError), with recovery off the frames are non-finite and check_numerics stops the run.  ``mid``: the second
    evaluation, so the next one sees a NaN input and its moments raise range events.  ``last``: the chunk's final
    evaluation, which no later kernel sees -- no range event at all, only the isfinite backstops of recovery.py and
    cli.check_numerics can catch it."""
    import evc_amd  # noqa: F401
    from evc_amd import cli, sampler as S
    real = S._eps
    state = {"n": 0, "inject": None}

    def eps(n, x, label, cond):
        e = real(n, x, label, cond)
        if state["inject"] is not None and state["n"] % state["per_chunk"] == state["inject"]:
            e = e.clone()
            e[1, 4, 7, 9] = NAN
        state["n"] += 1
        return e
    monkeypatch.setattr(S, "_eps", eps)
    cond = torch.from_numpy(np.random.default_rng(5).random((2, 2, 3, 32, 32), dtype=np.float32)).cuda()
    clean = _decoder(_decoder_net(), "off").generate(cond, generator=torch.Generator(device="cuda").manual_seed(11))
    assert bool(torch.isfinite(clean).all()) and L.range_events(reset=True) == 0
    state.update(per_chunk=state["n"], n=0, inject=1 if at == "mid" else state["n"] - 1)   # evaluations per chunk pass
    assert state["per_chunk"] >= 3
    with pytest.raises(cli.NumericsError) as err:
        _decoder(_decoder_net(), "layer").generate(cond, generator=torch.Generator(device="cuda").manual_seed(11))
    quiet = "range-event word 0x0, site words {}, chunk finite: False" in str(err.value)
    assert quiet == (at == "last"), str(err.value)
    L.range_events(reset=True)
    state["n"] = 0
    frames = _decoder(_decoder_net(), "off").generate(cond, generator=torch.Generator(device="cuda").manual_seed(11))
    assert not bool(torch.isfinite(frames).all())
    with pytest.raises(cli.NumericsError, match="range-event word 0x0, frames finite: False" if at == "last" else "frames finite"):
        cli.check_numerics(frames, "chunk")
