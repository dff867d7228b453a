"""Same-process A/B of the 3x3 convolutions of the score network's 16 x 16 and 8 x 8 levels that carry no fused 1x1 operand
(B clips): the split-K convolution (``conv2d_nhwc``, its combine launch included) against the one-launch kernel with the K
groups inside the workgroup (``small_conv``), called as ``ScoreNet._res`` calls them.  Variants alternate over the rounds; the
calls of a round are captured once into a HIP graph and replayed, which takes the host's per-call cost out of the figures;
median (min ... max) over the rounds per call, achieved TFLOP/s.

    python tools/small_conv_ab.py [B] [rounds] [calls per round] [variants]

``variants``: also time every forced kernel instance of the shape's width and the plain workgroup order (+16) next to the
chosen one.  A shape belongs on ``small_conv`` only if its maximum is below the convolution's minimum."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import evc_amd  # noqa: E402,F401
from evc_amd import lib as L  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 9
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
calls = int(sys.argv[3]) if len(sys.argv) > 3 else 100
all_variants = "variants" in sys.argv[4:]
WARM = 5

# (H = W, C0, C1, Co, form): Conv_0 = GroupNorm + SiLU on load (or, behind the FIR pass of an up / down block, a plain
# activated input), bias, moments; Conv_1 of a block without a skip convolution adds the residual and 1 / sqrt(2)
SHAPES = [(8, 576, 0, 576, "plain"), (8, 576, 0, 576, "res"), (8, 576, 0, 768, "affine"), (8, 768, 0, 768, "res"),
          (8, 768, 576, 768, "affine"), (8, 768, 768, 768, "affine"),
          (16, 384, 0, 384, "plain"), (16, 384, 0, 576, "affine"), (16, 576, 0, 576, "res"), (16, 576, 384, 576, "affine"),
          (16, 576, 576, 576, "affine"), (16, 768, 0, 768, "plain"), (16, 768, 576, 576, "affine")]

for (H, C0, C1, Co, form) in SHAPES:
    C = C0 + C1
    x0 = torch.randn(B, H, H, C0, device="cuda")
    x1 = torch.randn(B, H, H, C1, device="cuda") if C1 else None
    wp = L.conv_pack_weights(torch.randn(Co, C, 3, 3, device="cuda") / (9 * C) ** 0.5, L.ARITH_F16X3)
    kw = dict(bias=torch.randn(Co, device="cuda"), src1=x1, want_stats=True)
    coef = form != "plain"
    if coef:
        kw.update(coef=(1 + 0.2 * torch.randn(B, C, device="cuda"), 0.3 * torch.randn(B, C, device="cuda")), act_in=L.ACT_SILU)
    if form == "res":
        kw.update(res=torch.randn(B, H, H, Co, device="cuda"), out_scale=0.70710678)
    plan = L.conv_plan(B, H, H, C0, C1, Co, 3, L.ARITH_F16X3, coef=coef, act_in=L.ACT_SILU if coef else L.ACT_NONE)
    variants = {"conv": lambda: L.conv2d_nhwc(x0, wp, Co, 3, 3, **kw)}
    names = {"conv": f"{plan['kernel']} splits {plan['splits']}"}
    forced = [v + o for v in ((1, 2) if H == 8 else (3, 4)) for o in (0, 16)] if all_variants else []
    for v in [0] + forced:
        if L.small_conv_supported(B, H, H, C0, C1, Co, coef=coef, variant=v):
            variants[f"small{v or ''}"] = lambda v=v: L.small_conv(x0, wp, Co, variant=v, **kw)
            names[f"small{v or ''}"] = L.small_conv_plan(B, H, H, C0, C1, Co, coef=coef, variant=v)["kernel"]
    runs = {}
    for v, fn in variants.items():
        for _ in range(WARM):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(calls):
                fn()
        runs[v] = g.replay
    res = {}
    for r in range(rounds):
        for v, fn in runs.items():
            fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            res.setdefault(v, []).append(e0.elapsed_time(e1) / calls * 1e3)
    flops = 2.0 * B * H * H * 9 * C * Co
    for v in variants:
        us = statistics.median(res[v])
        verdict = "" if v == "conv" else ("  FASTER" if max(res[v]) < min(res["conv"]) else "  not clearly faster")
        print(f"B={B} {H}x{H} {C0}+{C1}->{Co} {form:6s} {v:8s} {names[v]:44s}: {us:6.1f} us (min {min(res[v]):.1f} ... max "
              f"{max(res[v]):.1f})  {flops / us / 1e6:6.1f} TFLOP/s{verdict}", flush=True)
