"""Host tests of the NIN GEMM's queries (csrc/nin_gemm.hip; no device needed): what ``evc_nin_gemm_supported`` takes and
refuses, that the launch refuses the same arguments before it touches a device, and that the convolution planner still
answers for the projection shapes as it did (the GEMM is a separate operation, not a plan of the convolution)."""
import ctypes

import pytest

import evc_amd  # noqa: F401
from evc_amd import lib as L

UNSUPPORTED = -2
# the six projections of the full-size network: (H = W, Ci, Co, affine GroupNorm on load)
PRODUCT = [(32, 384, 1152, True), (32, 384, 384, False), (16, 576, 1728, True), (16, 576, 576, False),
           (8, 768, 2304, True), (8, 768, 768, False)]
REFUSED = {
    "ci_not_64": dict(Ci=96),
    "co_not_64": dict(Co=96),
    "bf16x6_pack": dict(arith=L.ARITH_BF16X6),
    "f32_pack": dict(arith=L.ARITH_F32),
    "two_sources": dict(two_sources=True),
    "output_activation": dict(act_out=L.ACT_SILU),
    "both_on_load_forms": dict(coef=True, bound=True),
    "no_on_load_form": dict(coef=False, bound=False),
    "pixels_not_a_tile": dict(H=6, W=6),
}


def query(**over):
    kw = dict(B=2, H=8, W=8, Ci=64, Co=128, arith=L.ARITH_F16X3, coef=False)
    kw.update(over)
    return L.nin_query_args(**kw)


def conv_keeps(B, H, Co):
    """The grids left to the convolution because it measured faster there (profiles/NOTES.md, "Attention projections": at
    B = 9 the 32 x 32 q | k | v projection, 35.4 us against the GEMM's 37.1): its own 128-pixel x 192-channel tiles divide the
    shape and there are at least 256 of them, one per CU."""
    return Co % 192 == 0 and (H * H) % 128 == 0 and (B * H * H // 128) * (Co // 192) >= 256


@pytest.mark.parametrize("H,Ci,Co,coef", PRODUCT)
def test_supported_for_the_projections_of_the_full_size_network(H, Ci, Co, coef):
    """1 for the six projections at B = 1..32, except the grids measured faster on the convolution, which answer 0 (and only
    those: at the benchmark's B = 9 that is the 32 x 32 q | k | v projection alone).  A forced tile is never refused for it."""
    assert [conv_keeps(9, h, co) for h, _, co, _ in PRODUCT] == [True, False, False, False, False, False]
    for B in range(1, 33):
        assert L.nin_gemm_supported(B, H, H, Ci, Co, coef=coef) == (not conv_keeps(B, H, Co)), B
        assert L.nin_gemm_supported(B, H, H, Ci, Co, coef=coef, tile=11)
        if conv_keeps(B, H, Co):
            continue
        p = L.nin_gemm_plan(B, H, H, Ci, Co, coef=coef)
        tm, tn = p["tile"]
        assert (H * H) % tm == 0 and Co % tn == 0 and p["stages"] * 64 == Ci      # no tile straddles two samples
        assert p["stats_runs"] * 32 * (tm // 64) == H * H
        assert p["kernel"] == "nin_gemm_kernel<%d, %d, %s>" % (tm // 64, tn // 64, "true" if coef else "false")


def test_the_tile_is_a_function_of_the_shape_alone():
    """Pure function of (M, K, N) and the pixels per sample: the same for both on-load forms and for B x H*W factorings
    that keep M and the sample size."""
    for H, Ci, Co, _ in PRODUCT:
        for B in (1, 5, 9, 32):
            if conv_keeps(B, H, Co):
                continue
            assert L.nin_gemm_plan(B, H, H, Ci, Co, coef=True)["tile"] == L.nin_gemm_plan(B, H, H, Ci, Co, coef=False)["tile"]
            assert L.nin_gemm_plan(B, H, H, Ci, Co)["tile"] == L.nin_gemm_plan(B, H // 2, 2 * H, Ci, Co)["tile"]


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_by_the_query_and_by_the_launch(name):
    lib = L.hip_lib(require_device=False)
    assert lib.evc_nin_gemm_supported(ctypes.byref(query())) == 1
    a = query(**REFUSED[name])
    assert lib.evc_nin_gemm_supported(ctypes.byref(a)) == 0
    assert lib.evc_nin_gemm_plan_query(ctypes.byref(a), ctypes.byref(L.NinPlan())) == UNSUPPORTED
    # the launch validates before it touches the device (the pointers are dummies): the same refusal, no fallback
    assert lib.evc_nin_gemm_f32(ctypes.byref(a), None) == UNSUPPORTED


def test_forced_tiles():
    assert L.nin_gemm_plan(9, 32, 32, 384, 1152, coef=True, tile=22)["tile"] == (128, 128)
    assert L.nin_gemm_plan(9, 32, 32, 384, 1152, coef=True, tile=11)["tile"] == (64, 64)
    assert not L.nin_gemm_supported(9, 8, 8, 768, 768, tile=21)          # H*W = 64: no 128-pixel tile
    assert not L.nin_gemm_supported(9, 16, 16, 576, 576, tile=22)        # 576 is not a multiple of 128
    assert not L.nin_gemm_supported(9, 16, 16, 576, 576, tile=12)        # not a tile


@pytest.mark.parametrize("H,Ci,Co,coef", PRODUCT)
def test_the_convolution_planner_does_not_know_the_gemm(H, Ci, Co, coef):
    for B in (1, 9, 32):
        assert L.conv_plan(B, H, H, Ci, 0, Co, 1, L.ARITH_F16X3, coef=coef)["kernel"].startswith("conv_splitn_kernel<2, ")
