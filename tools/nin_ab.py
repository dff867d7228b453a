"""Same-process A/B of the attention blocks' projections at the score network's six shapes (B clips): the 1x1 convolution
(``conv2d_nhwc``, its split-K combine launch included) against the no-split GEMM (``nin_gemm``), called as ``ScoreNet._attn``
calls them.  Alternating rounds of back-to-back calls between HIP events after warm-up calls; median (min ... max) over the
rounds per call, achieved TFLOP/s and bytes/s (bytes from the shapes: x, packed weights, out, residual).

    python tools/nin_ab.py [B] [rounds] [calls per round] [tiles] [graph]

``tiles``: also time every forced tile of the GEMM (22 / 21 / 11) next to the chosen one.  ``graph``: the calls of a round are
captured once into a HIP graph and replayed, which takes the host's per-call cost out of the figures.
A shape belongs on the GEMM only if its maximum is below the convolution's minimum."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import evc_amd  # noqa: E402,F401
from evc_amd import lib as L  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 9
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
calls = int(sys.argv[3]) if len(sys.argv) > 3 else 200
all_tiles = "tiles" in sys.argv[4:]
graph = "graph" in sys.argv[4:]
WARM = 20

for (H, Ci, Co) in ((32, 384, 1152), (32, 384, 384), (16, 576, 1728), (16, 576, 576), (8, 768, 2304), (8, 768, 768)):
    qkv = Co == 3 * Ci
    x = torch.randn(B, H, H, Ci, device="cuda")
    wp = L.conv_pack_weights(torch.randn(Co, Ci, 1, 1, device="cuda") / Ci ** 0.5, L.ARITH_F16X3)
    bias = torch.randn(Co, device="cuda")
    if qkv:         # affine GroupNorm on load, moments for the q | k | v bounds
        kw = dict(bias=bias, coef=(1 + 0.2 * torch.randn(B, Ci, device="cuda"), 0.3 * torch.randn(B, Ci, device="cuda")),
                  want_stats=True)
    else:           # raw attention output under v's bound, residual, 1 / sqrt(2), moments for the next GroupNorm
        word = torch.zeros(1, dtype=torch.int32, device="cuda")
        L.gn_coeffs([L.chan_stats(x)], H * H, Ci // 16, 1e-5, bound=word)
        kw = dict(bias=bias, res=torch.randn(B, H, H, Co, device="cuda"), out_scale=0.70710678, in_bound=word, want_stats=True)
    plan = L.conv_plan(B, H, H, Ci, 0, Co, 1, L.ARITH_F16X3, coef=qkv)
    variants = {"conv": lambda: L.conv2d_nhwc(x, wp, Co, 1, 1, **kw)}
    names = {"conv": f"{plan['kernel']} splits {plan['splits']}"}
    for t in (0, 22, 21, 11) if all_tiles else (0,):
        if L.nin_gemm_supported(B, H, H, Ci, Co, coef=qkv, tile=t):
            variants[f"nin{t or ''}"] = lambda t=t: L.nin_gemm(x, wp, Co, tile=t, **kw)
            names[f"nin{t or ''}"] = L.nin_gemm_plan(B, H, H, Ci, Co, coef=qkv, tile=t)["kernel"]
    runs = {}
    for v, fn in variants.items():
        for _ in range(WARM):
            fn()
        torch.cuda.synchronize()
        runs[v] = fn
        if graph:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(calls):
                    fn()
            runs[v] = g.replay
    res = {}
    for r in range(rounds):
        for v, fn in runs.items():
            for _ in range(1 if graph else WARM):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(1 if graph else calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res.setdefault(v, []).append(e0.elapsed_time(e1) / calls * 1e3)
    M = B * H * H
    flops = 2.0 * M * Ci * Co
    nbytes = 4.0 * (M * Ci + Ci * Co + M * Co * (1 if qkv else 2))
    for v in variants:
        us = statistics.median(res[v])
        verdict = "" if v == "conv" else ("  FASTER" if max(res[v]) < min(res["conv"]) else "  not clearly faster")
        print(f"B={B} {H}x{H} {Ci}->{Co} {'qkv' if qkv else 'out'} {v:6s} {names[v]:40s}: {us:6.1f} us (min {min(res[v]):.1f} ... max "
              f"{max(res[v]):.1f})  {flops / us / 1e6:6.1f} TFLOP/s  {nbytes / us / 1e3:6.0f} GB/s{verdict}", flush=True)
