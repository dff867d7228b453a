"""GPU tests of ``lib.nin_gemm`` (csrc/nin_gemm.hip): the attention blocks' projections as one GEMM launch without K split.

1. bits: equal to ``conv2d_nhwc(..., splits=1)`` on ``conv_splitn_kernel<2, ...>`` (the arithmetic it must reproduce);
2. fp64: the bars of tests/test_gpu_conv_ledger.py for the same families, relative to max |ref| -- 2e-6 for the raw operand
   with an element bound, at most twice the error of the same case under EVC_ARITH_F32 for the affine form;
3. moments: summed over runs against the fp64 sums of ``out`` (< 1e-5 relative, the ledger's rule), and run-to-run equality;
4. non-finite footprint: a NaN / inf input element poisons exactly its pixel's output row, a NaN bound word everything;
5. routing in ``ScoreNet._attn`` on the reduced network of the other GPU tests."""
import numpy as np
import pytest
import torch

from conftest import rnd

pytestmark = pytest.mark.gpu

SCALE = 0.70710678
MAGNITUDES = (1.0, 8.0, 0.125)          # raw form: one magnitude per sample under ONE bound word

# (B, H, W, Ci, Co): one tile and one stage | three samples, two stages (both LDS buffers) | 128-pixel tiles, an odd stage
# count | many channel tiles
SMALL = [(1, 8, 8, 64, 64), (3, 8, 8, 128, 192), (2, 16, 16, 192, 128), (2, 32, 32, 64, 576)]
# the six projections of the full-size network: (H = W, Ci, Co)
PRODUCT = [(32, 384, 1152), (32, 384, 384), (16, 576, 1728), (16, 576, 576), (8, 768, 2304), (8, 768, 768)]


@pytest.fixture(scope="module")
def L():
    import evc_amd  # noqa: F401
    from evc_amd import lib
    lib.hip_lib()   # raises if libevc_hip.so is missing or the device is not gfx950: no silent fallback
    return lib


@pytest.fixture(autouse=True)
def clean_events(L):
    L.range_events(reset=True)
    yield
    assert L.range_events(reset=True) == 0


_cases = {}


def case(L, B, H, W, Ci, Co, form):
    """Inputs of one (shape, on-load form), made once and shared by the tests (never written to)."""
    key = (B, H, W, Ci, Co, form)
    if key not in _cases:
        x = rnd(700, B, H, W, Ci)
        kw = {}
        if form == "raw":
            x = x * torch.tensor([MAGNITUDES[b % 3] for b in range(B)]).view(-1, 1, 1, 1)
            x = x.cuda()
            word = torch.zeros(1, dtype=torch.int32, device="cuda")
            L.gn_coeffs([L.chan_stats(x)], H * W, Ci // 16, 1e-5, bound=word)      # as the network makes a bound: from moments
            kw["in_bound"] = word
        else:
            x = x.cuda()
            kw["coef"] = ((1 + 0.2 * rnd(704, B, Ci)).cuda(), (0.3 * rnd(705, B, Ci)).cuda())
        w = (rnd(701, Co, Ci, 1, 1) / np.sqrt(Ci)).cuda()
        _cases[key] = dict(x=x, w=w, wp=L.conv_pack_weights(w, L.ARITH_F16X3), bias=rnd(702, Co).cuda(),
                           res=rnd(703, B, H, W, Co).cuda(), kw=kw)
    return _cases[key]


def conv_unsplit(L, c, Co, **kw):
    """The reference launch: the 1x1 convolution forced unsplit, which must be conv_splitn_kernel<2, ...> without slabs."""
    prof = []
    L.CONV_PROFILE = prof
    try:
        r = L.conv2d_nhwc(c["x"], c["wp"], Co, 1, 1, splits=1, **c["kw"], **kw)
    finally:
        L.CONV_PROFILE = None
    assert prof[0]["kernel"].startswith("conv_splitn_kernel<2, "), prof[0]["kernel"]
    assert prof[0]["split"] is False
    return r


def fp64_ref(c, res, scale):
    x = c["x"].double()
    if "coef" in c["kw"]:
        a, s = c["kw"]["coef"]
        x = x * a.double()[:, None, None, :] + s.double()[:, None, None, :]
    r = x @ c["w"].double()[:, :, 0, 0].t() + c["bias"].double()
    return (r + (c["res"].double() if res else 0.0)) * scale


@pytest.mark.parametrize("form", ["affine", "raw"])
@pytest.mark.parametrize("shape", SMALL, ids=["x".join(map(str, s)) for s in SMALL])
def test_bits_of_the_unsplit_convolution_kernel(L, shape, form):
    B, H, W, Ci, Co = shape
    c = case(L, B, H, W, Ci, Co, form)
    assert L.nin_gemm_supported(B, H, W, Ci, Co, coef=form == "affine")
    for res in (False, True):
        for scale in (1.0, SCALE):
            for stats in (False, True):
                kw = dict(bias=c["bias"], res=c["res"] if res else None, out_scale=scale, want_stats=stats)
                got = L.nin_gemm(c["x"], c["wp"], Co, **c["kw"], **kw)
                ref = conv_unsplit(L, c, Co, **kw)
                if stats:       # (the moments are not pinned to the convolution's bits: the compiler is free to contract the
                    got, ref = got[0], ref[0]      # output scale into their sums in either kernel; test_moments_... has their rule)
                assert torch.equal(got, ref), (res, scale, stats, float((got - ref).abs().max()))
    # every kernel instance the shape admits (the tile is chosen by grid size: a small batch alone reaches the smallest only)
    kw = dict(bias=c["bias"], res=c["res"], out_scale=SCALE, want_stats=True)
    ref, _ = conv_unsplit(L, c, Co, **kw)
    tiles = [t for t in (11, 21, 22) if L.nin_gemm_supported(B, H, W, Ci, Co, coef=form == "affine", tile=t)]
    assert 11 in tiles and (H * W < 128 or 21 in tiles) and (H * W < 128 or Co % 128 or 22 in tiles)
    for t in tiles:
        got, gst = L.nin_gemm(c["x"], c["wp"], Co, tile=t, **c["kw"], **kw)
        assert torch.equal(got, ref), (t, float((got - ref).abs().max()))
        o = got.double().reshape(B, H * W, Co)
        want = torch.stack([o.sum(1), (o * o).sum(1)], -1)
        assert gst.shape[1] == H * W // (32 * (t // 10))
        assert float((gst.double().sum(1) - want).abs().max() / want.abs().max()) < 1e-5, t


@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("shape", PRODUCT, ids=["%dx%d_%dto%d" % (s[0], s[0], s[1], s[2]) for s in PRODUCT])
def test_bits_on_the_projections_of_the_full_size_network(L, shape, B):
    """As ``ScoreNet._attn`` calls them: q | k | v = affine GroupNorm on load, bias, moments; output = raw operand with a
    bound, bias, residual, 1/sqrt(2), moments."""
    H, Ci, Co = shape
    form = "affine" if Co == 3 * Ci else "raw"
    c = case(L, B, H, H, Ci, Co, form)
    kw = dict(bias=c["bias"], want_stats=True)
    if form == "raw":
        kw.update(res=c["res"], out_scale=SCALE)
    # (a grid the support query leaves to the convolution -- B = 9, 32 x 32 q | k | v -- still has the kernel: forced tile)
    tile = 0 if L.nin_gemm_supported(B, H, H, Ci, Co, coef=form == "affine") else 21
    got, gst = L.nin_gemm(c["x"], c["wp"], Co, tile=tile, **c["kw"], **kw)
    ref, _ = conv_unsplit(L, c, Co, **kw)
    assert torch.equal(got, ref), float((got - ref).abs().max())
    o = got.double().reshape(B, H * H, Co)
    want = torch.stack([o.sum(1), (o * o).sum(1)], -1)
    assert float((gst.double().sum(1) - want).abs().max() / want.abs().max()) < 1e-5
    _cases.pop((B, H, H, Ci, Co, form))          # the large inputs are used here only


@pytest.mark.parametrize("form", ["affine", "raw"])
@pytest.mark.parametrize("shape", SMALL, ids=["x".join(map(str, s)) for s in SMALL])
def test_against_fp64(L, shape, form):
    B, H, W, Ci, Co = shape
    c = case(L, B, H, W, Ci, Co, form)
    ref = fp64_ref(c, True, SCALE)
    out = L.nin_gemm(c["x"], c["wp"], Co, bias=c["bias"], res=c["res"], out_scale=SCALE, **c["kw"])
    err = float((out.double() - ref).abs().max() / ref.abs().max())
    if form == "raw":
        bar, e32 = 2e-6, None
    else:       # the rule of the ledger for families without a fixed bar: at most twice the exact-product arithmetic's error
        o32 = L.conv2d_nhwc(c["x"], L.conv_pack_weights(c["w"], L.ARITH_F32), Co, 1, 1, bias=c["bias"], res=c["res"],
                            out_scale=SCALE, coef=c["kw"]["coef"])
        e32 = float((o32.double() - ref).abs().max() / ref.abs().max())
        bar = 2.0 * e32
    print(f"NIN {shape} {form} | err {err:.3e} | bar {bar:.3e} | f32 {'-' if e32 is None else format(e32, '.3e')}")
    assert err <= bar, (err, bar)


@pytest.mark.parametrize("form", ["affine", "raw"])
@pytest.mark.parametrize("shape", SMALL, ids=["x".join(map(str, s)) for s in SMALL])
def test_moments_and_repeatability(L, shape, form):
    B, H, W, Ci, Co = shape
    c = case(L, B, H, W, Ci, Co, form)
    kw = dict(bias=c["bias"], res=c["res"], out_scale=SCALE, want_stats=True, **c["kw"])
    out, st = L.nin_gemm(c["x"], c["wp"], Co, **kw)
    runs = L.nin_gemm_plan(B, H, W, Ci, Co, coef=form == "affine")["stats_runs"]
    assert st.shape == (B, runs, Co, 2) and (H * W) % runs == 0
    o = out.double().reshape(B, H * W, Co)
    want = torch.stack([o.sum(1), (o * o).sum(1)], -1)
    assert float((st.double().sum(1) - want).abs().max() / want.abs().max()) < 1e-5
    # the moments are what gn_coeffs / moments_bound consume: they take the run count from the tensor
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.moments_bound(st, 0, Co, word)
    bound = float(word.view(torch.float32))
    assert float(out.abs().max()) ** 2 <= bound <= float((out.double() ** 2).reshape(B, -1, Co).sum(1).max()) * (1 + 1e-5)
    out2, st2 = L.nin_gemm(c["x"], c["wp"], Co, **kw)
    assert torch.equal(out2, out) and torch.equal(st2, st)


@pytest.mark.parametrize("form", ["affine", "raw"])
def test_nonfinite_footprint(L, form):
    """A NaN and an inf in one input element each make exactly that pixel's output row non-finite and nothing else (the bound
    word is that of the clean tensor: a poisoned tensor's bound is the NaN pattern, next test)."""
    B, H, W, Ci, Co = SMALL[2]
    c = case(L, B, H, W, Ci, Co, form)
    kw = dict(bias=c["bias"], res=c["res"], out_scale=SCALE, **c["kw"])
    clean = L.nin_gemm(c["x"], c["wp"], Co, **kw)
    assert bool(torch.isfinite(clean).all())
    pos = [(0, 0, 0, 0), (0, 7, 15, Ci - 1), (1, 8, 0, 65), (B - 1, H - 1, W - 1, 17)]       # tile corners and edges, both samples
    for v in (float("nan"), float("inf"), float("-inf")):
        x = c["x"].clone()
        mask = torch.zeros(B, H, W, dtype=torch.bool, device="cuda")
        for b, y, xx, ch in pos:
            x[b, y, xx, ch] = v
            mask[b, y, xx] = True
        out = L.nin_gemm(x, c["wp"], Co, **kw)
        bad = ~torch.isfinite(out)
        assert bool((bad == mask[..., None].expand_as(bad)).all()), v
        assert torch.equal(out[~mask], clean[~mask]), v


def test_nan_bound_word_makes_the_whole_output_nan(L):
    B, H, W, Ci, Co = SMALL[1]
    c = case(L, B, H, W, Ci, Co, "raw")
    word = torch.tensor([0x7fc00000], dtype=torch.int32, device="cuda")
    out, st = L.nin_gemm(c["x"], c["wp"], Co, bias=c["bias"], in_bound=word, want_stats=True)
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(st).all())


def test_refusals_raise(L):
    """No silent fallback: what ``nin_gemm_supported`` refuses raises from the launch."""
    c = case(L, *SMALL[0], "raw")
    with pytest.raises(L.EvcKernelError):      # neither on-load form
        L.nin_gemm(c["x"], c["wp"], 64, bias=c["bias"])
    with pytest.raises(L.EvcKernelError):      # a bf16x6 pack
        L.nin_gemm(c["x"], L.conv_pack_weights(c["w"], L.ARITH_BF16X6), 64, bias=c["bias"], **c["kw"])


# ---- routing -----------------------------------------------------------------------------------------------------------

def reduced_net():
    from evc_amd.config import default_config
    from evc_amd.scorenet import ScoreNet
    from oracle.scorenet import Dims, seeded_params
    return ScoreNet(default_config(32, 32, 32), seeded_params(Dims(ngf=32, n_head_channels=32, image_size=32), 91))


def profiled_forward(L, net, x, cond):
    """-> (output, the 1x1 convolution launches as (shape (B, H, W, Ci, Co), call record), shapes of the nin_gemm launches)"""
    conv, nin = [], []
    L.CONV_PROFILE, L.NIN_PROFILE = conv, nin
    try:
        out = net.forward_label(x, 500, cond)
    finally:
        L.CONV_PROFILE, L.NIN_PROFILE = None, None
    torch.cuda.synchronize()
    return out, [(r["shape"][:5], r["call"]) for r in conv if r["shape"][5] == 1], [r["shape"] for r in nin]


def test_routing_in_the_score_network(L):
    net = reduced_net()
    x, cond = rnd(92, 2, 15, 32, 32).cuda(), rnd(93, 2, 6, 32, 32).cuda()
    assert net.nin_gemm is True
    # off: every projection is a 1x1 convolution.  Those the GEMM takes (the reduced network also has 32-wide blocks and a
    # 4 x 4 level, which it does not): q | k | v = GroupNorm coefficients on load, Co = 3 Ci; output = bound + residual, Co = Ci
    net.forward_label(x, 500, cond)          # the label's AdaGN row (time-embedding linears) is made once, here
    net.nin_gemm = False
    out_off, k1_off, nin_off = profiled_forward(L, net, x, cond)
    net.nin_gemm = True
    assert nin_off == []
    want = sorted(s for s, c in k1_off if L.nin_gemm_supported(*s, coef=c["coef"], bound=c["bound"]) and
                  ((c["coef"] and s[4] == 3 * s[3]) or (c["bound"] and c["res"] and s[4] == s[3])))
    blocks = [i for i, m in enumerate(net.program) if m["kind"] == "attn" and m["ch"] % 64 == 0]
    assert 6 <= len(want) <= 2 * len(blocks) and len(want) % 2 == 0
    shapes = set(want)
    # on: exactly those moved, nothing else did, and no 1x1 convolution of an attention shape is left
    out_on, k1_on, nin_on = profiled_forward(L, net, x, cond)
    assert sorted(nin_on) == want
    assert sorted([s for s, _ in k1_on] + nin_on) == sorted(s for s, _ in k1_off)
    assert not [s for s, _ in k1_on if s in shapes]
    # (numbers: the module taps and sampler goldens of tests/test_gpu_scorenet.py run through the GEMM and keep their bars)
    print("nin_gemm on vs off, max rel diff of the forward:", float((out_on - out_off).abs().max() / out_off.abs().max()))
    assert bool(torch.isfinite(out_on).all())
    # the batch-invariant view keeps the convolution whatever the attribute says
    _, k1_inv, nin_inv = profiled_forward(L, net.invariant_view(), x, cond)
    assert nin_inv == [] and sorted(s for s, _ in k1_inv if s in shapes) == want
    # a demoted attention block (packs moved to bf16x6) is back on the convolution, the others stay on the GEMM
    i = next(j for j in blocks if (2, 8, 8, net.program[j]["ch"], 3 * net.program[j]["ch"]) in shapes)
    net.demote([s["site"] for s in net.sites if s["module"] == i and s["tag"] in ("attn_norm", "attn_qkv")])
    _, k1_dem, nin_dem = profiled_forward(L, net, x, cond)
    back = [(s, c) for s, c in k1_dem if s in shapes]
    assert len(nin_dem) == len(want) - 2 and len(back) == 2 and all(c["arith"] == L.ARITH_BF16X6 for _, c in back)
    assert sorted(nin_dem + [s for s, _ in back]) == want
    assert L.range_events() == 0 and L.site_events(net) == {}
