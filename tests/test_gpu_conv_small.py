"""GPU tests of ``lib.small_conv`` (csrc/conv_small.hip): the 3x3 convolutions of the 16 x 16 / 8 x 8 levels in one launch,
the K range divided over wave groups inside the workgroup.

1. fp64: the bars of tests/test_gpu_conv_ledger.py for the f16x3 plan classes, relative to max |ref| -- 2e-6 for an operand
   with an element bound, else at most twice the error of the same case under EVC_ARITH_F32 -- and at most FACTOR times the
   error of ``conv2d_nhwc`` (its split-K plan) on the same call;
2. moments: summed over runs against the fp64 sums of ``out`` (< 1e-5 relative, the ledger's rule);
3. run-to-run equality, and equality of the two workgroup orders;
4. halo: image-border pixels hold a large constant, so a pixel read from the wrong side of a border shows;
5. non-finite footprint (the rule of tests/test_gpu_nonfinite.py for convolutions): a NaN / inf input element poisons exactly
   its 3x3 neighbourhood, the rest keeps its bits; NaN moments of one sample raise the range word in gn_coeffs;
6. routing in ``ScoreNet._res`` on the reduced network of the other GPU tests, ``small_conv`` on against off."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rnd

pytestmark = pytest.mark.gpu

SCALE = 0.70710678
# Error of small_conv against fp64 over the error of conv2d_nhwc on the same call.  Both add the same exact-to-fp32 products
# in different orders, the convolution in 7 .. 24 short split-K pieces, this kernel in 2 .. 8 longer ones.  Measured over
# three seeds of every case below, every kernel instance (profiles/NOTES.md, "Small-grid convolutions"): the largest ratio
# per seed was 2.00, 2.03 and 2.05 (errors of 2.2 .. 2.7e-7 against 1.1 .. 1.3e-7, at most 0.75 of the ledger's bar); the
# maximum of a few thousand such ratios moves by tens of per cent from seed to seed, hence 3.
FACTOR = 3.0

# chunk counts 3 and 5: with G = 4 an empty group and an uneven split, with G = 8 mostly empty groups; a concat boundary
# inside the K range
SOURCES = [(48, 0), (32, 16), (80, 0)]
SHAPES = [(H, B, Co, C0, C1) for H in (8, 16) for B in (1, 3) for Co in (64, 192) for (C0, C1) in SOURCES]
VARIANTS = {8: (1, 2), 16: (3, 4)}


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


def case(L, H, B, Co, C0, C1, form, seed=800):
    """Inputs of one (shape, on-load form) and the fp64 convolution of them, made once and shared (never written to).
    form: "affine" = GroupNorm coefficients + SiLU on load; "plain" = an activated input as it is."""
    key = (H, B, Co, C0, C1, form, seed)
    if key not in _cases:
        C = C0 + C1
        x = rnd(seed, B, H, H, C).cuda()
        w = (rnd(seed + 1, Co, C, 3, 3) / np.sqrt(9 * C)).cuda()
        kw = {}
        pre = x.double()
        if form == "affine":
            a, s = (1 + 0.2 * rnd(seed + 4, B, C)).cuda(), (0.3 * rnd(seed + 5, B, C)).cuda()
            kw.update(coef=(a, s), act_in=L.ACT_SILU)
            pre = F.silu(pre * a.double()[:, None, None, :] + s.double()[:, None, None, :])
        x0, x1 = x[..., :C0].contiguous(), (x[..., C0:].contiguous() if C1 else None)
        word = torch.zeros(1, dtype=torch.int32, device="cuda")
        L.gn_coeffs([L.chan_stats(t) for t in (x0, x1) if t is not None], H * H, C // 16, 1e-5, bound=word)
        ref = F.conv2d(pre.permute(0, 3, 1, 2), w.double(), padding=1).permute(0, 2, 3, 1)
        _cases[key] = dict(x0=x0, x1=x1, w=w, wp=L.conv_pack_weights(w, L.ARITH_F16X3), w32=L.conv_pack_weights(w, L.ARITH_F32),
                           bias=rnd(seed + 2, Co).cuda(), res=rnd(seed + 3, B, H, H, Co).cuda(), kw=kw, word=word, ref=ref)
    return _cases[key]


def rel(out, ref):
    return float((out.double() - ref).abs().max() / ref.abs().max())


def errors(L, c, Co, res, scale, stats, bound, variant=0):
    """-> (error of small_conv, of conv2d_nhwc on the same call, the bar, small_conv's output and moments)"""
    kw = dict(bias=c["bias"], src1=c["x1"], res=c["res"] if res else None, out_scale=scale, **c["kw"])
    ref = (c["ref"] + c["bias"].double() + (c["res"].double() if res else 0.0)) * scale
    bkw = dict(in_bound=c["word"]) if bound else {}
    got = L.small_conv(c["x0"], c["wp"], Co, want_stats=stats, variant=variant, **kw, **bkw)
    got, st = got if stats else (got, None)
    old = L.conv2d_nhwc(c["x0"], c["wp"], Co, 3, 3, **kw, **bkw)
    if bound:
        bar = 2e-6
    else:       # the ledger's rule for families without a fixed bar: at most twice the exact-product arithmetic's error
        bar = 2.0 * rel(L.conv2d_nhwc(c["x0"], c["w32"], Co, 3, 3, **kw), ref)
    return rel(got, ref), rel(old, ref), bar, got, st


def check_moments(out, st, runs):
    B, H, W, Co = out.shape
    assert st.shape == (B, runs, Co, 2)
    o = out.double().reshape(B, H * W, Co)
    want = torch.stack([o.sum(1), (o * o).sum(1)], -1)
    assert float((st.double().sum(1) - want).abs().max() / want.abs().max()) < 1e-5


@pytest.mark.parametrize("form", ["affine", "plain"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d_b%d_co%d_%d+%d" % (s[0], s[0], *s[1:]) for s in SHAPES])
def test_against_fp64_and_the_convolution(L, shape, form):
    H, B, Co, C0, C1 = shape
    c = case(L, H, B, Co, C0, C1, form)
    assert L.small_conv_supported(B, H, H, C0, C1, Co, coef=form == "affine")
    runs = L.small_conv_plan(B, H, H, C0, C1, Co, coef=form == "affine")["stats_runs"]
    for res in (False, True):
        for scale in (1.0, SCALE):
            for stats in (False, True):
                for bound in ((False, True) if form == "plain" else (False,)):       # a bound belongs to a raw / activated operand
                    err, old, bar, out, st = errors(L, c, Co, res, scale, stats, bound)
                    print(f"SMALL {shape} {form} res={res} scale={scale:.3f} bound={bound} | err {err:.3e} | conv {old:.3e} | bar {bar:.3e}")
                    assert err <= bar, (err, bar)
                    assert err <= FACTOR * old, (err, old)
                    if stats:
                        check_moments(out, st, runs)


@pytest.mark.parametrize("H", [8, 16])
def test_every_kernel_instance_and_repeatability(L, H):
    """Each instance the plan can return (and the forced ones), both workgroup orders: the bars of the test above, two runs
    of one call equal, the two orders equal (the order changes which workgroup computes a tile, not how)."""
    for (C0, C1) in SOURCES:
        c = case(L, H, 3, 192, C0, C1, "affine")
        for v in VARIANTS[H]:
            plan = L.small_conv_plan(3, H, H, C0, C1, 192, coef=True, variant=v)
            err, old, bar, out, st = errors(L, c, 192, True, SCALE, True, False, variant=v)
            print(f"SMALL variant {v} {plan['kernel']} {H}x{H} {C0}+{C1} | err {err:.3e} | conv {old:.3e} | bar {bar:.3e}")
            assert err <= bar and err <= FACTOR * old, (v, err, old, bar)
            check_moments(out, st, plan["stats_runs"])
            for order in (0, 16):
                _, _, _, out2, st2 = errors(L, c, 192, True, SCALE, True, False, variant=v + order)
                assert torch.equal(out2, out) and torch.equal(st2, st), (v, order)


@pytest.mark.parametrize("H", [8, 16])
def test_border_pixels_with_a_large_constant(L, H):
    """The pixels on the image border are 100: a tap that wraps into the neighbouring row, the other half of the image or
    the next sample instead of the zero padding changes an output by O(100)."""
    B, Co, C0, C1 = 3, 64, 32, 16
    x = rnd(820, B, H, H, C0 + C1)
    x[:, 0], x[:, -1], x[:, :, 0], x[:, :, -1] = 100.0, 100.0, 100.0, 100.0
    x = x.cuda()
    x0, x1 = x[..., :C0].contiguous(), x[..., C0:].contiguous()
    w = (rnd(821, Co, C0 + C1, 3, 3) / np.sqrt(9 * (C0 + C1))).cuda()
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.gn_coeffs([L.chan_stats(x0), L.chan_stats(x1)], H * H, (C0 + C1) // 16, 1e-5, bound=word)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), padding=1).permute(0, 2, 3, 1)
    for v in (0,) + VARIANTS[H]:
        out = L.small_conv(x0, L.conv_pack_weights(w, L.ARITH_F16X3), Co, src1=x1, in_bound=word, variant=v)
        assert rel(out, ref) <= 2e-6, (v, rel(out, ref))


@pytest.mark.parametrize("form", ["affine", "plain"])
@pytest.mark.parametrize("H", [8, 16])
def test_nonfinite_footprint(L, H, form):
    B, Co, C0, C1 = 3, 64, 32, 16
    c = case(L, H, B, Co, C0, C1, form)
    kw = dict(bias=c["bias"], src1=c["x1"], res=c["res"], out_scale=SCALE, **c["kw"])
    clean = L.small_conv(c["x0"], c["wp"], Co, **kw)
    assert bool(torch.isfinite(clean).all())
    # corners, the row where the two 128-pixel tiles of a 16 x 16 image meet, both sources, every sample
    pos = [(0, 0, 0, 0, 0), (0, H - 1, H - 1, 1, C1 - 1), (1, H // 2 - 1, 3, 0, 17), (1, H // 2, 0, 1, 0), (B - 1, H - 1, 0, 0, C0 - 1)]
    mask = torch.zeros(B, 1, H, H)
    for b, y, x, _, _ in pos:
        mask[b, 0, y, x] = 1.0
    foot = (F.conv2d(mask, torch.ones(1, 1, 3, 3), padding=1)[:, 0] > 0).cuda()
    for v in (float("nan"), float("inf"), float("-inf")):
        x0, x1 = c["x0"].clone(), c["x1"].clone()
        for b, y, x, src, ch in pos:
            (x0 if src == 0 else x1)[b, y, x, ch] = v
        out = L.small_conv(x0, c["wp"], Co, **{**kw, "src1": x1})
        outside = ~foot[..., None].expand_as(out)
        assert torch.equal(out[outside], clean[outside]), v
        assert not bool(torch.isfinite(out[~outside]).any()), v


def test_nonfinite_moments_stay_in_their_sample_and_raise_the_range_word(L):
    H, B, Co, C0, C1 = 8, 3, 64, 32, 16
    c = case(L, H, B, Co, C0, C1, "affine")
    kw = dict(bias=c["bias"], src1=c["x1"], res=c["res"], out_scale=SCALE, want_stats=True, **c["kw"])
    clean, st0 = L.small_conv(c["x0"], c["wp"], Co, **kw)
    x0 = c["x0"].clone()
    x0[0, H // 2, H // 2, 1] = float("nan")
    out, st = L.small_conv(x0, c["wp"], Co, **kw)
    assert torch.equal(out[1:], clean[1:]) and torch.equal(st[1:], st0[1:])
    assert not bool(torch.isfinite(st[0].double().sum(0)).any())
    L.range_events(reset=True)
    L.gn_coeffs([st], H * H, 32, 1e-5)
    assert L.range_events(reset=True) & L.RANGE_NONFINITE
    # the NaN pattern in the bound word: the whole output and every moment
    word = torch.tensor([0x7fc00000], dtype=torch.int32, device="cuda")
    out, st = L.small_conv(c["x0"], c["wp"], Co, bias=c["bias"], src1=c["x1"], in_bound=word, want_stats=True)
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(st).all())


def test_refusals_raise(L):
    """No silent fallback: what ``small_conv_supported`` refuses raises from the launch."""
    c = case(L, 8, 1, 64, 48, 0, "affine")
    with pytest.raises(L.EvcKernelError):      # coefficients without the SiLU
        L.small_conv(c["x0"], c["wp"], 64, coef=c["kw"]["coef"])
    with pytest.raises(L.EvcKernelError):      # a bf16x6 pack
        L.small_conv(c["x0"], L.conv_pack_weights(c["w"], L.ARITH_BF16X6), 64, **c["kw"])
    with pytest.raises(L.EvcKernelError):      # an instance of the other image width
        L.small_conv(c["x0"], c["wp"], 64, variant=3, **c["kw"])


# ---- routing -----------------------------------------------------------------------------------------------------------

def reduced_net():
    from evc_amd.config import default_config
    from evc_amd.scorenet import ScoreNet
    from oracle.scorenet import Dims, seeded_params
    net = ScoreNet(default_config(32, 32, 32), seeded_params(Dims(ngf=32, n_head_channels=32, image_size=32), 91))
    # everything on the current stream: routing is what is tested here, and a test that makes no stream of its own leaves the
    # streams of the tests that run after it in this process (tests/test_gpu_ops.py's clock probe) where they were
    net.overlap_skip = False
    return net


def profiled_forward(L, net, x, cond):
    """-> (output, the 3x3 convolution launches as (B, H, W, Ci, Co), shapes of the small_conv launches)"""
    conv, small = [], []
    L.CONV_PROFILE, L.SMALL_CONV_PROFILE = conv, small
    try:
        out = net.forward_label(x, 500, cond)
    finally:
        L.CONV_PROFILE, L.SMALL_CONV_PROFILE = None, None
    torch.cuda.synchronize()
    return out, [(r["shape"][:5], r["call"]) for r in conv if r["shape"][5] == 3], [r["shape"] for r in small]


def test_routing_in_the_score_network(L):
    """``small_conv`` on against off in one process: exactly the 16 x 16 / 8 x 8 3x3 convolutions without a fused 1x1 operand
    move, and the forward agrees.  Tolerance: the switch changes the fp32 summation order of these layers and nothing else,
    so the two forwards differ as two plans of the convolution do -- each layer's error against fp64 is <= 5e-7 of its
    largest output (the ledger), the reduced network chains 14 such layers between the switch and the output, and the
    module-tap tests of tests/test_gpu_scorenet.py hold the whole chain to 1e-4: an order of magnitude inside that."""
    net = reduced_net()
    x, cond = rnd(92, 2, 15, 32, 32).cuda(), rnd(93, 2, 6, 32, 32).cuda()
    assert net.small_conv is True
    net.forward_label(x, 500, cond)          # the label's AdaGN row (time-embedding linears) is made once, here
    net.small_conv = False
    out_off, k3_off, small_off = profiled_forward(L, net, x, cond)
    net.small_conv = True
    assert small_off == []
    want = sorted(s for s, c in k3_off if s[1] in (8, 16) and not c["x2"] and
                  L.small_conv_supported(s[0], s[1], s[2], c["C0"], c["C1"], s[4], coef=c["coef"], act_in=c["act_in"], bound=c["bound"]))
    assert len(want) >= 6
    out_on, k3_on, small_on = profiled_forward(L, net, x, cond)
    assert sorted(small_on) == want
    assert sorted([s for s, _ in k3_on] + small_on) == sorted(s for s, _ in k3_off)
    assert not [s for s, c in k3_on if s[1] in (8, 16) and not c["x2"]]
    d = float((out_on - out_off).abs().max() / out_off.abs().max())
    print("small_conv on vs off, max rel diff of the forward:", d)
    assert bool(torch.isfinite(out_on).all()) and d <= 1e-5
    # the batch-invariant view keeps the convolution whatever the attribute says
    _, k3_inv, small_inv = profiled_forward(L, net.invariant_view(), x, cond)
    assert small_inv == [] and len(k3_inv) == len(k3_off)
    assert L.range_events() == 0 and L.site_events(net) == {}
