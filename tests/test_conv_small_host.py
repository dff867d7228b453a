"""Host tests of the small-grid convolution's queries (csrc/conv_small.hip; no device needed): what
``evc_small_conv_supported`` takes and refuses, that the launch refuses the same arguments before it touches a device, the
plan per shape, and that the convolution planner answers exactly as it does without the operation (it is a separate
operation, not a plan of the convolution)."""
import ctypes
import os
import subprocess
import sys

import pytest

import evc_amd  # noqa: F401
from evc_amd import lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED = -2
# the 3x3 convolutions of the full-size network's 16 x 16 and 8 x 8 levels that carry no fused 1x1 operand:
# (H = W, C0, C1, Co, GroupNorm + SiLU on load)
# (tests/test_invariant_plan.py FULL_SIZE_CONVS, the 3x3 rows of these two sizes)
PRODUCT = [(8, 576, 0, 576, False), (8, 576, 0, 576, True), (8, 576, 0, 768, True), (8, 768, 0, 768, True),
           (8, 768, 576, 768, True), (8, 768, 768, 768, True),
           (16, 384, 0, 384, False), (16, 384, 0, 576, True), (16, 576, 0, 576, True), (16, 576, 384, 576, True),
           (16, 576, 576, 576, True), (16, 768, 0, 768, False), (16, 768, 576, 576, True),
           (16, 384, 0, 384, True), (16, 768, 0, 768, True)]       # (these two only occur with a fused 1x1 operand)


def test_the_list_above_is_the_network_s():
    from test_invariant_plan import FULL_SIZE_CONVS
    want = sorted({(H, C0, C1, Co, bool(coef)) for (H, W, C0, C1, Co, K, ar, coef, act, x2, bound) in FULL_SIZE_CONVS
                   if K == 3 and H == W and H in (8, 16)})
    assert sorted(PRODUCT) == want


REFUSED = {
    "bf16x6_pack": dict(arith=L.ARITH_BF16X6),
    "f32_pack": dict(arith=L.ARITH_F32),
    "filter_1x1": dict(K=1),
    "grid_32x32": dict(H=32, W=32),
    "grid_4x4": dict(H=4, W=4),
    "not_square": dict(H=8, W=16),
    "batch_invariant": dict(invariant=True),
    "fused_1x1_operand": dict(x2=True),
    "output_activation": dict(act_out=L.ACT_SILU),
    "coefficients_without_silu": dict(coef=True, act_in=L.ACT_NONE),
    "silu_without_coefficients": dict(coef=False, act_in=L.ACT_SILU),
    "relu_on_load": dict(act_in=L.ACT_RELU),
    "c0_not_16": dict(C0=40),
    "c1_not_16": dict(C1=8),
    "co_not_32": dict(Co=48),
    "variant_of_the_other_width": dict(variant=3),
    "no_such_variant": dict(variant=5),
    "long_k_at_16x16": dict(H=16, W=16, C0=400, C1=0),
    "long_k_at_8x8_on_a_small_grid": dict(C0=784, C1=0),
    "more_than_a_round_at_16x16": dict(H=16, W=16, B=33, Co=128),
}


def query(**over):
    kw = dict(B=2, H=8, W=8, C0=48, C1=16, Co=64)
    kw.update(over)
    return L.small_conv_query_args(**kw)


@pytest.mark.parametrize("H,C0,C1,Co,coef", PRODUCT)
@pytest.mark.parametrize("B", [1, 6, 9])
def test_supported_and_planned_for_the_small_levels_of_the_full_size_network(B, H, C0, C1, Co, coef):
    """What measured faster (profiles/NOTES.md "Small-grid convolutions"); the rest answers 0 unless an instance is forced.
    8 x 8: up to 768 input channels at every batch, the concat layers where the last round of workgroups (Co / 32 x B on 256
    CUs) is 3/4 full -- B = 9, not 6 or 1.  16 x 16: up to 384 input channels while the 128 x 32 tiles fit one round."""
    Ct = C0 + C1
    t3 = Co // 32 * 2 * B
    if H == 8:
        taken, v = Ct <= 768 or 4 * (Co // 32 * B) >= 3 * 256 * -(-(Co // 32 * B) // 256), 1
        assert taken == (Ct <= 768 or B == 9)
    else:
        taken, v = Ct <= 384 and t3 <= 256, 3
        assert taken == (Ct <= 384 and not (Co == 576 and B == 9))
    for bound in (False, True):
        assert L.small_conv_supported(B, H, H, C0, C1, Co, coef=coef, bound=bound) == taken
        assert L.small_conv_supported(B, H, H, C0, C1, Co, coef=coef, bound=bound, variant=1 if H == 8 else 4)
    if not taken:
        return
    p = L.small_conv_plan(B, H, H, C0, C1, Co, coef=coef)
    wm, wn, g = {1: (1, 1, 8), 3: (2, 1, 4)}[v]
    assert p["variant"] == v and p["tile"] == (64 * wm, 32 * wn) and p["groups"] == g
    assert p["kernel"] == "conv_small_kernel<%d, %d, %d, %s>" % (wm, wn, g, "true" if coef else "false")
    assert p["chunks"] == (C0 + C1) // 16 and p["rounds"] == -(-p["chunks"] // g)
    assert (H * H) % p["tile"][0] == 0 and Co % p["tile"][1] == 0          # no tile straddles two samples
    assert p["stats_runs"] * 64 == H * H


def test_the_plan_is_a_function_of_the_layer_alone():
    for H, C0, C1, Co, coef in PRODUCT:
        plans = [L.small_conv_plan(B, H, H, C0, C1, Co, coef=coef, variant=1 if H == 8 else 3) for B in (1, 2, 9, 32)]
        assert all(p == plans[0] for p in plans)


def test_chunk_counts_the_groups_do_not_divide():
    """Fewer chunks than groups, and an uneven split: rounds = chunks of the longest group, the rest idle."""
    assert L.small_conv_plan(1, 8, 8, 48, 0, 64, variant=2)["rounds"] == 1         # 3 chunks, G = 4: one empty group
    assert L.small_conv_plan(1, 8, 8, 80, 0, 64, variant=2)["rounds"] == 2         # 5 chunks, G = 4: 2 + 2 + 1 + 0
    assert L.small_conv_plan(1, 8, 8, 48, 0, 64)["rounds"] == 1                    # G = 8: five empty groups
    assert L.small_conv_plan(1, 16, 16, 32, 16, 64, variant=4)["rounds"] == 2      # 3 chunks, G = 2: 2 + 1


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_by_the_query_and_by_the_launch(name):
    lib = L.hip_lib(require_device=False)
    assert lib.evc_small_conv_supported(ctypes.byref(query())) == 1
    a = query(**REFUSED[name])
    assert lib.evc_small_conv_supported(ctypes.byref(a)) == 0
    assert lib.evc_small_conv_plan_query(ctypes.byref(a), ctypes.byref(L.SmallConvPlan())) == UNSUPPORTED
    # the launch validates before it touches the device (the pointers are dummies): the same refusal, no fallback
    assert lib.evc_small_conv_f32(ctypes.byref(a), None) == UNSUPPORTED


def test_forced_variants():
    for v, H, tile, g in ((1, 8, (64, 32), 8), (2, 8, (64, 64), 4), (3, 16, (128, 32), 4), (4, 16, (128, 64), 2)):
        for order in (0, 16):
            p = L.small_conv_plan(9, H, H, 96, 0, 192, variant=v + order)
            assert (p["variant"], p["tile"], p["groups"]) == (v, tile, g)
    assert not L.small_conv_supported(9, 8, 8, 96, 0, 96, variant=2)          # 96 channels: no 64-channel tile
    assert L.small_conv_supported(9, 8, 8, 96, 0, 96, variant=1)


@pytest.mark.parametrize("H,C0,C1,Co,coef", PRODUCT)
def test_the_convolution_planner_does_not_know_the_operation(H, C0, C1, Co, coef):
    for B in (1, 9):
        p = L.conv_plan(B, H, H, C0, C1, Co, 3, L.ARITH_F16X3, coef=coef, act_in=L.ACT_SILU if coef else L.ACT_NONE)
        assert p["kernel"].split("<")[0] in ("conv_split_rr_kernel", "conv_splitn_kernel", "conv_wide_kernel")


def test_plan_dump_of_the_convolution_planner_with_and_without_the_operation_loaded():
    """tools/conv_plan_dump.py in a fresh process, and in one that has called the small-grid queries first (its code is loaded
    and has run): the same bytes."""
    tool = os.path.join(REPO, "tools", "conv_plan_dump.py")
    plain = subprocess.run([sys.executable, tool], capture_output=True, check=True, cwd=REPO).stdout
    pre = ("import sys, runpy; sys.path.insert(0, %r); import evc_amd; from evc_amd import lib as L; "
           "assert L.small_conv_supported(9, 8, 8, 768, 0, 768, coef=True); L.small_conv_plan(9, 16, 16, 384, 0, 384, coef=True); "
           "sys.argv = [%r]; runpy.run_path(%r, run_name='__main__')" % (REPO, tool, tool))
    loaded = subprocess.run([sys.executable, "-c", pre], capture_output=True, check=True, cwd=REPO).stdout
    assert len(plain) > 1000 and loaded == plain
