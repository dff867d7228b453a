#!/usr/bin/env python3
"""Benchmark of the decode hot path on MI355X: decoded frames/s for 30-frame 128x128 clips at q3.

    python bench.py --gpus N --steps K --warmup W

With N > 1 and no torchrun environment the script LAUNCHES the N ranks itself (child processes of
``python -m torch.distributed.run``, one per GPU, rendezvous on 127.0.0.1) before it makes any HIP call, relays
rank 0's JSON line and exits with the launcher's status; under an existing torchrun environment
(``python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N``) it is a rank.  A world size
that differs from ``--gpus`` is an error, never a silent 1-GPU measurement.

One "step" = one pass of the receiver over one batch of clips per GPU (BASELINE.json configs[1]: 9 clips =
city_bonn[0..8], q3): per clip 2 ELIC key frames are entropy-decoded + synthesised and 28 frames are generated
by 6 diffusion chunks (DDPM, 1000-step schedule subsampled to 100, + 1 denoise call = 101 score-network
forwards per chunk, fp32).  Weak scaling: every GPU decodes its own 9 clips; no data-path collective
(clips are independent); weights are broadcast once from rank 0 over RCCL before timing.
Synthetic data, seeded random weights of the reference architecture (no checkpoints / dataset offline).

Rank 0 prints ONE JSON line (contract in the task statement) with these extra objects:
  roofline     -- the dominant kernel (one template instance of the implicit-GEMM convolution): algorithmic FLOPs per launch
                  / its average launch duration measured live with HIP events recorded around that kernel on the launch
                  stream; `rocprof` quotes the committed rocprofv3 --kernel-trace --stats CSV and `traffic` the committed
                  PMC passes when (and only when) they were taken on the kernel source that is running
  hbm_classes  -- achieved HBM rate of the memory-bound kernel classes, HIP-event timed at the
                  benchmark's shapes
  cpu_baseline -- the CPU oracle (a port, kind "port") timed on this box's host cores on a bounded sample (single-rank
                  runs only: with N > 1 ranks the other ranks would sit in a collective while rank 0 measures)
  per_rank_value / range_events -- every rank's own frames/s (load imbalance shows here), and the sticky range-event
                  word of the fp16-split arithmetic (0 = every operand provably in range, every tensor finite)
"""
import argparse
import hashlib
import json
import os
import sys
import time

# dmabuf IPC (RCCL / device-tensor sharing across the ranks of a node): the only mode this host driver supports; normally already
# exported by the environment, set here before the HIP runtime starts in case a launcher dropped it
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

FWD_FLOP_PER_SAMPLE = 345_201_475_584      # one score-network forward, one sample
ELIC_DECODE_FLOP = 10.865e9                # one 128x128 key-frame decode
F32_MFMA_PEAK_TFLOPS = 157.3               # /opt/skills/guides/MI355X_MICROARCH.md: dense f32 matrix == vector peak
MFMA16_PEAK_TFLOPS = 2500.0                # same guide: dense bf16 / fp16 MFMA (no sparsity)
HBM_PEAK_GBS = 8000.0
# fp32-equivalent roofs of the split arithmetics: `achieved` stays ALGORITHMIC fp32 FLOPs (2*M*Co*taps*Ci) per second,
# the kernel issues 6 (bf16x6) or 3 (f16x3) 16-bit MFMAs per fp32 product.
ARITH_INFO = {
    0: ("f32", F32_MFMA_PEAK_TFLOPS, "dense f32 MFMA 157.3 TFLOP/s (v_mfma_f32_32x32x2_f32)"),
    1: ("bf16x6", MFMA16_PEAK_TFLOPS / 6.0, "dense bf16 MFMA 2500 TFLOP/s / 6 MFMAs per fp32 product (exact 3-way bf16 "
                                           "split, fp32 accumulate); f32-MFMA roof would be 157.3"),
    2: ("f16x3", MFMA16_PEAK_TFLOPS / 3.0, "dense fp16 MFMA 2500 TFLOP/s / 3 MFMAs per fp32 product (operands scaled "
                                          "into range + 2-way fp16 split = 22 significand bits, fp32 accumulate; error vs "
                                          "fp64 below the f32-MFMA chain, profiles/r02_split_numerics.log); the bf16x6 "
                                          "roof would be 416.7, the f32-MFMA roof 157.3"),
}
CONV_SOURCES = ("extreme-video-compression-with-prediction-using-pre-trainded-diffusion-models-_amd/csrc/conv_igemm.hip",)


def progress(msg):
    """Progress goes to stderr (stdout carries exactly one JSON line): long phases must not look like a hang."""
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--clips", type=int, default=9, help="clips per GPU per step (configs[1]: start 0 end 8)")
    ap.add_argument("--total-clips", type=int, default=0,
                    help="fixed JOB size instead of --clips per GPU: the clips are block-sharded over the ranks "
                         "(evc_amd.dist.shard_range: 46 over 8 -> 6,6,6,6,6,6,5,5 = BASELINE configs[2]; 256 with "
                         "--sampler FPNDM --subsample 50 = configs[4]); reported as strong scaling")
    ap.add_argument("--subsample", type=int, default=100)
    ap.add_argument("--sampler", default="DDPM", choices=["DDPM", "DDIM", "FPNDM"])
    ap.add_argument("--groups", type=int, default=1,
                    help="concurrent clip groups per GPU during generation (one HIP stream each)")
    ap.add_argument("--preactivate", action="store_true",
                    help="apply AdaGN+SiLU once per tensor in its own pass instead of inside the conv operand load")
    ap.add_argument("--graphs", action="store_true",
                    help="replay every score-network forward from a captured HIP graph (host enqueue 4.8 -> 0.2 ms per forward; "
                         "same kernels, bit-identical results): for hosts whose CPU share per rank is small")
    ap.add_argument("--fail-rank", type=int, default=-1,
                    help="(plumbing test) this rank exits with an error before the first collective: the job must end "
                         "non-zero within EVC_DIST_TIMEOUT_S instead of hanging")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-baseline-seconds", type=float, default=10.0,
                    help="budget of EACH leg of the CPU baseline (all-threads forwards, 1-thread forward)")
    ap.add_argument("--plumbing-only", action="store_true",
                    help="run only the multi-rank plumbing (launch, rendezvous, weight-style broadcast, barriers, "
                         "max-over-ranks) and print the JSON skeleton: works without a GPU (gloo)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step decoded as DIR/<name>.npy (float32, at most "
                         "64 MB over all ranks; a seeded sample of the clips when the whole output is larger)")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return a


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, frames, rank, world):
    """What the timed path returned in its last step, as float32 .npy files under ``out_dir``.  ``frames`` is one rank's
    (clips, 30, 3, H, W) decode; every rank writes its own file (``frames.npy`` for one rank, ``frames_rank<r>.npy``
    otherwise) within an equal share of DUMP_LIMIT_BYTES.  Beyond that share a fixed, seeded choice of whole frames is
    written as (k, 3, H, W), in order, with their flat indices clip * 30 + frame in ``<name>_index.npy``."""
    os.makedirs(out_dir, exist_ok=True)
    name = "frames" if world == 1 else f"frames_rank{rank}"
    flat = frames.reshape(-1, *frames.shape[2:])
    per_frame = flat[0].numel() * 4
    keep = max(1, (DUMP_LIMIT_BYTES // world - 4096) // (per_frame + 8))
    if keep < flat.shape[0]:
        idx = np.sort(np.random.default_rng(4321 + rank).choice(flat.shape[0], keep, replace=False))
        frames = flat[torch.from_numpy(idx).to(flat.device)]
        np.save(os.path.join(out_dir, f"{name}_index.npy"), idx.astype(np.float64))
    np.save(os.path.join(out_dir, f"{name}.npy"), frames.float().cpu().numpy())


def source_sha():
    h = hashlib.sha256()
    for rel in CONV_SOURCES:
        h.update(open(os.path.join(REPO, rel), "rb").read())
    return h.hexdigest()[:16]


def roofline_leg(net, clips, device):
    """Profiled forwards at the benchmark batch size: HIP events around every conv launch, on the launch stream."""
    from evc_amd import lib as L
    x = torch.randn(clips, 15, 128, 128, device=device)
    c = torch.randn(clips, 6, 128, 128, device=device)
    # per-kernel durations: the forward normally overlaps each res-block's 1x1 skip convolution (side stream) with its
    # 3x3 convolution; HIP events around concurrent launches would charge each with the other's time, so the profiled
    # forwards run the launches one after another on one stream
    overlap, net.overlap_skip = getattr(net, "overlap_skip", False), False
    graphs, net.use_graphs = getattr(net, "use_graphs", False), False        # a graph replay makes no per-launch calls
    net.forward_label(x, 500, c)            # warm
    torch.cuda.synchronize()
    prof = []
    L.CONV_PROFILE = prof
    reps = 3
    tf0 = time.perf_counter()
    net.forward_label(x, 500, c)
    torch.cuda.synchronize()
    probe = L.ClockProbe(int(max(1.0, 2.0 * reps * (time.perf_counter() - tf0) * 1e3) * 1e3), device)   # ends with the forwards below
    prof.clear()
    for _ in range(reps):
        net.forward_label(x, 500, c)
    probe.stop()
    L.CONV_PROFILE = None
    torch.cuda.synchronize()
    live_clock = probe.ghz()
    net.overlap_skip, net.use_graphs = overlap, graphs
    per, kern = {}, {}
    for r in prof:
        # e0..ec brackets the convolution kernel alone (recorded inside the C call, before the split-K combine kernel):
        # the duration rocprofv3 --kernel-trace reports for that kernel; e0..e1 includes the combine launch
        ms_k, ms_all = r["e0"].elapsed_time(r["ec"]), r["e0"].elapsed_time(r["e1"])
        v = per.setdefault((r["arith"], r["variant"]), dict(n=0, ms=0.0, flops=0.0))
        v["n"] += 1
        v["ms"] += ms_all
        v["flops"] += r["flops"]
        # the kernel template instance this launch runs, as the library's dispatch names it (evc_conv_kernel_name): the name
        # rocprofv3 --kernel-trace --stats reports
        c = r["call"]
        name = r["kernel"]
        kv = kern.setdefault((name, r["arith"]), dict(n=0, ms=0.0, ms_all=0.0, flops=0.0, bytes=0.0))
        kv["n"] += 1; kv["ms"] += ms_k; kv["ms_all"] += ms_all; kv["flops"] += r["flops"]
        # algorithmic HBM bytes of the launch: every operand read once, the output written once (fp32 activations, the
        # packed weights as they are stored: two fp16 / three bf16 planes or fp32)
        M = c["B"] * c["H"] * c["W"]
        wbytes = {0: 4, 1: 6, 2: 4}[r["arith"]]
        kv["bytes"] += (4.0 * M * (c["C0"] + c["C1"] + c["x2"] + c["Co"] * (2 if c["res"] else 1))
                        + wbytes * c["Co"] * (c["K"] * c["K"] * (c["C0"] + c["C1"]) + c["x2"]))
    total_ms = sum(v["ms"] for v in per.values()) / reps
    total_flops = sum(v["flops"] for v in per.values()) / reps
    # THE dominant kernel: the template instance with the largest share of the convolution time.  achieved = its algorithmic
    # FLOPs per launch / its average launch duration (the kernel alone); the committed rocprofv3 --kernel-trace --stats CSV of
    # the same forward (profiles/r04_forward_b9_kernel_stats.csv, side stream off like this leg) holds the same average.
    (dk_name, dk_arith), dk = max(kern.items(), key=lambda kv: kv[1]["ms"])
    aname, peak, basis = ARITH_INFO[dk_arith]
    us = dk["ms"] / dk["n"] * 1e3
    gflop = dk["flops"] / dk["n"] / 1e9
    achieved = dk["flops"] / (dk["ms"] * 1e-3) / 1e12
    out = {"bound": "mfma", "achieved": round(achieved, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
           "frac": round(achieved / peak, 4), "traffic": None, "kernel": dk_name, "peak_basis": basis,
           "launches_per_forward": dk["n"] // reps, "avg_launch_us": round(us, 2),
           "algorithmic_gflop_per_launch": round(gflop, 3),
           "algorithmic_bytes_per_launch": int(dk["bytes"] / dk["n"]),
           "avg_launch_us_incl_combine": round(dk["ms_all"] / dk["n"] * 1e3, 2),
           "share_of_conv_time": round(dk["ms_all"] / reps / total_ms, 3),
           "achieved_over_f32_mfma_peak": round(achieved / F32_MFMA_PEAK_TFLOPS, 3)}
    try:
        import csv
        meta = json.load(open(os.path.join(REPO, "profiles", "r04_forward_b9_kernel_stats.json")))
        if meta.get("source_sha") == source_sha() and meta.get("batch") == clips:
            for row in csv.DictReader(open(os.path.join(REPO, "profiles", "r04_forward_b9_kernel_stats.csv"))):
                if dk_name in row["Name"]:
                    rus = float(row["AverageNs"]) / 1e3
                    out["rocprof"] = {"csv": "profiles/r04_forward_b9_kernel_stats.csv", "avg_us": round(rus, 2),
                                      "calls": int(row["Calls"]), "frac": round(gflop * 1e9 / (rus * 1e-6) / 1e12 / peak, 4)}
                    break
            if meta.get("held_clock_ghz"):
                out.setdefault("rocprof", {})["held_clock_ghz_pmc"] = meta["held_clock_ghz"]
            if meta.get("mfma_busy_frac"):
                out["mfma_busy_frac_pmc"] = meta["mfma_busy_frac"]
        else:
            out["rocprof"] = (f"profiles/r04_forward_b9_kernel_stats.csv was taken on source {meta.get('source_sha')} at "
                              f"B={meta.get('batch')}, this is {source_sha()} at B={clips}: not quoted")
    except Exception:
        pass
    if live_clock:
        # the chip does not hold its 2.4 GHz peak under these kernels (~2.05 GHz across a forward at ~1 000 W of the 1 400 W cap;
        # back-to-back launches of the heavy kernels reach the cap, profiles/r03_power_cap.log); `peak` is priced at 2.4 GHz regardless
        out["held_clock_ghz"] = round(live_clock, 3)
        out["held_clock_note"] = ("s_memtime / s_memrealtime of an idle probe wave (evc_clock_probe) across these forwards; "
                                  "2.4 GHz is the clock `peak` assumes")
        out["frac_at_held_clock"] = round(achieved / (peak * live_clock / 2.4), 4)
    prov = "no rocprofv3 PMC profile committed for this kernel source"
    try:       # HBM bytes per launch: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, only if taken on THIS source
        pmc = json.load(open(os.path.join(REPO, "profiles", f"r04_conv_{aname}_pmc.json")))
        if pmc.get("source_sha") != source_sha():
            prov = f"profiles/r04_conv_{aname}_pmc.json is stale (taken on source {pmc.get('source_sha')}): not reported"
        elif clips != pmc.get("batch") or pmc.get("kernel") != dk_name:
            prov = f"profiles/r04_conv_{aname}_pmc.json covers {pmc.get('kernel')} at B={pmc.get('batch')}"
        else:
            out["traffic"] = pmc["hbm_bytes_per_launch"]
            out["traffic_over_algorithmic_bytes"] = round(pmc["hbm_bytes_per_launch"] / (dk["bytes"] / dk["n"]), 2)
            prov = f"profiles/r04_conv_{aname}_pmc.json, source {pmc['source_sha']}, FETCH_SIZE x2 + WRITE_SIZE"
    except Exception:
        pass
    out["traffic_provenance"] = prov
    out["conv_ms_per_forward"] = round(total_ms, 3)
    out["all_conv_tflops"] = round(total_flops / (total_ms * 1e-3) / 1e12, 2)
    out["kernels"] = {n: {"launches_per_forward": v["n"] // reps, "avg_us": round(v["ms"] / v["n"] * 1e3, 1),
                          "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1),
                          "ms_per_forward_incl_combine": round(v["ms_all"] / reps, 3)}
                      for (n, _), v in sorted(kern.items(), key=lambda kv: -kv[1]["ms_all"])}
    out["families"] = {f"{ARITH_INFO[a][0]}<TN={t}>": {"launches_per_forward": v["n"] // reps,
                                                       "ms_per_forward": round(v["ms"] / reps, 3),
                                                       "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1)}
                       for (a, t), v in sorted(per.items())}
    out["batch"] = clips
    out["note"] = ("launch durations measured with the res-block side stream OFF (launches one after another; the timed region "
                   "runs with it on); `families` / conv_ms_per_forward include the split-K combine launches.  Inside a forward the "
                   "heavy convolution launches alternate with light kernels: the package averages ~1 000 W of its 1 400 W cap and "
                   "holds ~2.05 GHz (held_clock_ghz), so frac is bounded by CYCLES -- non-MFMA work per MFMA in the K loop "
                   "(weight-fragment loads ~26 %, operand staging arithmetic ~14 %, epilogue + prologue ~12 % of a tile: "
                   "profiles/r04_wide_ablation_duty.log, r04_wide_stamps_v2.log; DESIGN.md section 9) -- not by the power cap")
    return out


def hbm_classes_leg(clips, device):
    """achieved HBM rate per memory-bound kernel class = algorithmic bytes (every tensor read / written
    once) / HIP-event time, at the benchmark's shapes."""
    from evc_amd import lib as L

    def timeit(fn, iters=20):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters * 1e3      # us

    out = {}

    def rep(name, nbytes, us):
        gbs = nbytes / us / 1e3
        out[name] = {"GB/s": round(gbs), "frac": round(gbs / HBM_PEAK_GBS, 3), "us": round(us, 1),
                     "MB": round(nbytes / 1e6, 1)}
    B = clips
    k = np.outer([1, 3, 3, 1], [1, 3, 3, 1]).astype(np.float32) / 64
    x = torch.randn(B, 128, 128, 192, device=device)
    a, s = torch.rand(B, 192, device=device) + 0.5, torch.randn(B, 192, device=device)
    n = x.numel() * 4
    xs = torch.randn(B, 64, 64, 192, device=device)
    rep("fir_down2_adagn_silu_128to64_c192", n + n // 4,
        timeit(lambda: L.upfirdn2d_nhwc(x, k, 1, 2, (1, 1), coef=(a, s), act=L.ACT_SILU)))
    rep("fir_up2_adagn_silu_64to128_c192", xs.numel() * 4 + n,
        timeit(lambda: L.upfirdn2d_nhwc(xs, k * 4, 2, 1, (2, 1), coef=(a, s), act=L.ACT_SILU)))
    rep("chan_stats_128_c192", n, timeit(lambda: L.chan_stats(x)))
    rep("affine_act_128_c192", 2 * n, timeit(lambda: L.affine_act(x, (a, s), L.ACT_SILU)))
    xt = torch.randn(B, 15, 128, 128, device=device)
    e, nz = torch.randn_like(xt), torch.randn_like(xt)
    rep("ddpm_step", 4 * xt.numel() * 4, timeit(lambda: L.ddpm_step(xt, e, nz, 1.0, 0.1, 0.5, 0.5, 0.1, True)))
    c = torch.randn(B, 6, 128, 128, device=device)
    rep("pack_nchw_to_nhwc", (21 + 32) * B * 128 * 128 * 4, timeit(lambda: L.pack_nchw_to_nhwc(xt, c, 32)))
    return out


def cpu_baseline_leg(sd_d, sd_e, seconds):
    """The CPU oracle (oracle/, a port of the reference's PyTorch-CPU path) on this box's host cores.  Bounded sample
    of the same workload: whole fp32 score-network forwards at B=1 at all threads AND at 1 thread (what the
    reference CLI runs with: Inference.py:15 sets torch.set_num_threads(1) process-wide), a short DDPM chunk through
    the oracle sampler (sampler-step cost on top of the forwards), one ELIC key-frame decode."""
    from oracle import elic as OE, samplers as OS, schedule as OSch, scorenet as ON
    try:
        import psutil
        physical = psutil.cpu_count(logical=False)
    except Exception:
        physical = None
    d = ON.Dims()
    p = {k: v.cpu() for k, v in sd_d.items() if k.startswith("unet.all_modules.")}
    x, c = torch.randn(1, 15, 128, 128), torch.randn(1, 6, 128, 128)
    lab = torch.tensor([500])
    # "all threads" = torch's own default (one per physical core).  torchrun exports OMP_NUM_THREADS=1 to its ranks:
    # then fall back to the physical core count.  Never the logical-CPU count: 256 threads on this box's CPU share
    # oversubscribe it and run 50x slower (measured: 135 s per forward instead of ~2.5 s).
    n_before = torch.get_num_threads()
    n_all = n_before if n_before > 1 else min(physical or os.cpu_count() or 1, 128)
    torch.set_num_threads(n_all)

    def time_forwards(budget, max_n, warm=True):
        if warm:
            ON.forward(p, d, x, lab, cond=c)
        n, t0 = 0, time.time()
        while n < 1 or (time.time() - t0 < budget and n < max_n):
            ON.forward(p, d, x, lab, cond=c)
            n += 1
        return (time.time() - t0) / n, n
    # Thread count: torch's default (one per physical core) or 16 -- this box's CPU share can be far smaller than its core
    # count, and an oversubscribed run is 10-30x slower -- whichever runs a probe forward faster; the bounded sample
    # (forwards + a short chunk) then runs at that count.
    cands = [n_all] + ([16] if n_all > 16 else [])
    probe = {}
    for n in cands:
        torch.set_num_threads(n)
        probe[n], _ = time_forwards(0.0, 1)
        progress(f"cpu baseline: probe forward at {n} threads: {probe[n]:.2f} s")
    n_best = min(probe, key=probe.get)
    torch.set_num_threads(n_best)
    t_all, n_fwd = time_forwards(seconds, 40)
    progress(f"cpu baseline: {t_all:.3f} s/forward at {n_best} threads ({n_fwd} forwards); 2-step DDPM chunk through the oracle sampler")
    # a 2-step DDPM chunk = 3 forwards + 2 updates + denoise: the per-step sampler cost beside the forwards
    t0 = time.time()
    OS.ddpm(x.clone(), lambda xx, t: ON.forward(p, d, xx, t, cond=c), OSch.base_schedule(), subsample_steps=2)
    t_chunk3 = time.time() - t0
    step_overhead = max(0.0, (t_chunk3 - 3 * t_all) / 3)
    chunk_all = 101 * (t_all + step_overhead)
    progress("cpu baseline: one forward at 1 thread (the reference CLI's setting)")
    torch.set_num_threads(1)
    try:
        got_one = torch.get_num_threads()
        t_one, n_one = time_forwards(0.0, 1, warm=False)       # a single un-warmed forward
    finally:
        torch.set_num_threads(n_best)
    # one ELIC key-frame decode on the CPU (oracle nets; range coding through the native coder, as compressai's is C++)
    elic_ms = None
    progress(f"cpu baseline: {t_one:.1f} s/forward at 1 thread; one ELIC key-frame decode")
    try:
        from evc_amd import lib as L

        class _Coder:
            encode_with_indexes = staticmethod(L.rans_encode)
            decode_with_indexes = staticmethod(L.rans_decode)
        pe = {k: v.cpu() for k, v in sd_e.items()}
        img = torch.rand(1, 3, 128, 128)
        enc = OE.compress(pe, img, coder=_Coder)
        t0 = time.time()
        OE.decompress(pe, enc["strings"], enc["shape"], coder=_Coder)
        elic_ms = (time.time() - t0) * 1e3
    except Exception as ex:       # the baseline must never take the benchmark down
        elic_ms = f"failed: {type(ex).__name__}: {ex}"
    torch.set_num_threads(n_before)
    clip_s = 6 * chunk_all + 2 * (elic_ms / 1e3 if isinstance(elic_ms, float) else 0.0)
    return {"value": round(30.0 / clip_s, 5), "unit": "frames/s", "cores": n_best, "kind": "port",
            "physical_cores": physical,
            "sample": f"{n_fwd} fp32 score-network forwards (B=1, 345.2 GFLOP each) at {n_best} threads: {t_all:.3f} s/forward "
                      f"(probe forwards: {', '.join(f'{n} threads {t:.2f} s' for n, t in probe.items())}); "
                      f"a 2-step DDPM chunk through the oracle sampler: {t_chunk3:.2f} s (sampler step overhead "
                      f"{step_overhead * 1e3:.0f} ms/step); {n_one} forward at "
                      f"torch.set_num_threads(1) (get_num_threads() = {got_one}; the reference CLI's setting): {t_one:.2f} s; one ELIC key-frame "
                      f"decode: {elic_ms if not isinstance(elic_ms, float) else round(elic_ms, 1)} ms.  value = 30 frames / "
                      f"(6 chunks x 101 x (forward + step) + 2 key-frame decodes) with the fastest thread count ({n_best}), extrapolated "
                      f"from the sample",
            "forward_s": round(t_all, 4), "probe_forward_s_by_threads": {str(n): round(t, 3) for n, t in probe.items()},
            "forward_s_1_thread": round(t_one, 3),
            "chunk_s_best_threads": round(chunk_all, 1), "chunk_s_1_thread": round(101 * (t_one + step_overhead), 1),
            "frames_per_s_1_thread": round(30.0 / (6 * 101 * (t_one + step_overhead)), 6),
            "elic_keyframe_decode_ms": elic_ms if not isinstance(elic_ms, float) else round(elic_ms, 1),
            "note": "the reference additionally re-reads its 1 GB checkpoint for every chunk (city_sender.py:337); not "
                    "included"}


def rank_clips(a, rank, world):
    """-> (clips this rank decodes per step, config.workload text, scaling).  ``--clips`` per GPU is weak scaling (the
    driver's contract); ``--total-clips`` is a fixed job block-sharded over the ranks (BASELINE configs[2] / [4])."""
    from evc_amd import dist as D
    fwd = {"DDPM": a.subsample + 1, "DDIM": a.subsample + 1, "FPNDM": 12 + (a.subsample - 3)}[a.sampler]
    tail = f"x 30 frames 128x128, q3, 2 ELIC key frames + 6 chunks x {fwd} forwards ({a.sampler}-{a.subsample})"
    if a.total_clips > 0:
        lo, hi = D.shard_range(a.total_clips, rank, world)
        sizes = [D.shard_range(a.total_clips, r, world) for r in range(world)]
        plan = ",".join(str(h - l) for l, h in sizes)
        name = "custom"
        if (a.total_clips, a.sampler, a.subsample) == (46, "DDPM", 100):
            name = "configs[2]"
        elif (a.total_clips, a.sampler, a.subsample) == (256, "FPNDM", 50):
            name = "configs[4]"
        return hi - lo, f"{name}: {a.total_clips} clips over {world} rank(s) ({plan}) {tail}, one launch batch per rank", "strong"
    name = "configs[1]" if (a.clips, a.sampler, a.subsample) == (9, "DDPM", 100) else "custom"
    return a.clips, f"{name}: {a.clips} clips/GPU {tail}, B={a.clips} per launch", "weak"


def plumbing_only(a, D):
    """Multi-rank plumbing without the GPU path: what a CPU (gloo) test can assert about `bench.py --gpus N`."""
    rank, world, device = D.init()
    if world != a.gpus:
        print(f"error: --gpus {a.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        return 2
    if rank == a.fail_rank:
        print(f"rank {rank}: simulated failure (--fail-rank)", file=sys.stderr, flush=True)
        os._exit(7)
    sd = {"w": torch.arange(1000, dtype=torch.float32)} if rank == 0 else None
    sd = D.broadcast_state_dict(sd, src=0, device=device, world=world)
    ok = bool((sd["w"].cpu() == torch.arange(1000, dtype=torch.float32)).all())
    D.barrier()
    t0 = time.perf_counter()
    D.barrier()
    elapsed = D.max_over_ranks(time.perf_counter() - t0, device)
    seen = int(D.sum_over_ranks(1, device))
    n_own, workload, scaling = rank_clips(a, rank, world)
    per_rank_clips = [int(v) for v in D.gather_over_ranks(n_own, device)]
    if rank == 0:
        print(json.dumps({"metric": "decoded frames/sec (128x128x30) at q3", "value": None, "unit": "frames/s",
                          "n_gpus": world, "ranks_seen": seen, "backend": D.backend_name(), "plumbing_only": True,
                          "broadcast_ok": ok, "barrier_s": elapsed, "per_rank_clips": per_rank_clips, "scaling": scaling,
                          "config": {"workload": workload},
                          "self_launched": os.environ.get("EVC_SELF_LAUNCHED") == "1"}), flush=True)
    D.barrier()
    return 0 if ok and seen == world else 1


def main():
    a = parse()
    import evc_amd  # noqa: F401   (no HIP call: the library loads lazily)
    from evc_amd import dist as D
    if D.needs_self_launch(a.gpus):
        # parent: never touches the GPU; N child ranks do the work and rank 0 prints the line
        sys.exit(D.self_launch(os.path.abspath(__file__), sys.argv[1:], a.gpus))
    if a.plumbing_only:
        sys.exit(plumbing_only(a, D))

    from evc_amd import lib as L, sampler as S, synthetic
    from evc_amd.config import default_config
    from evc_amd.decoder import ClipDecoder, all_generated_mask
    from evc_amd.elic import ElicModel
    from evc_amd.scorenet import ScoreNet

    rank, world, device = D.init()
    if world != a.gpus:
        print(f"error: --gpus {a.gpus} but WORLD_SIZE={world}: refusing to report a {world}-rank run as {a.gpus} GPUs",
              file=sys.stderr)
        sys.exit(2)
    L.hip_lib()
    torch.cuda.set_device(device)
    cfg = default_config(192, 192, 128, subsample=a.subsample)
    if rank == 0:
        progress(f"rank 0 of {world}: building seeded weights, broadcast, packing")

    # weights: rank 0 owns the (synthetic, reference-layout) checkpoints; ONE broadcast per model over RCCL
    sd_d = synthetic.diffusion_state_dict(cfg, 1234) if rank == 0 else None
    sd_e = synthetic.elic_state_dict(3) if rank == 0 else None     # quality index 3 (q3)
    sd_d = D.broadcast_state_dict(sd_d, src=0, device=device, world=world)
    sd_e = D.broadcast_state_dict(sd_e, src=0, device=device, world=world)
    net = ScoreNet(cfg, sd_d, device=device, preactivate=a.preactivate, use_graphs=a.graphs)
    elic = ElicModel(sd_e, device=device)
    dec = ClipDecoder(net, elic, cfg, S.get_sampler(a.sampler), groups=a.groups)

    # inputs: this rank's clips; key frames 0,1 are ELIC-encoded once (sender side, untimed)
    n_own, workload, scaling = rank_clips(a, rank, world)
    if n_own < 1:
        print(f"error: rank {rank} of {world} has no clip to decode (--total-clips {a.total_clips})", file=sys.stderr)
        sys.exit(2)
    clips = torch.from_numpy(synthetic.make_clips(n_own, seed=100 + rank).astype(np.float32) / 255.0)
    key_strings, shape = [], None
    for f in range(2):
        enc = elic.compress(clips[:, f].to(device))
        key_strings.append(enc["strings"])
        shape = enc["shape"]
    d = all_generated_mask()
    gen = torch.Generator(device=device).manual_seed(1234 + rank)

    def step():
        return dec.decode(d, key_strings, shape, generator=gen)

    t_warm = None
    for i in range(a.warmup):
        tw = time.perf_counter()
        step()
        torch.cuda.synchronize()
        t_warm = time.perf_counter() - tw
        if rank == 0:
            progress(f"warm-up step {i + 1}/{a.warmup} done")
    D.barrier()
    torch.cuda.synchronize()
    # shader clock the chip holds during the timed region (it runs into the package power cap under the convolutions): an
    # idle one-wave probe on its own stream that ends with the region (or after 9 s of it)
    # (skipped with --graphs / --groups > 1: HIP streams can then share a hardware queue with the probe's stream and work
    # queued behind the parked probe kernel would stall until it times out -- ADVICE r3)
    probe = (L.ClockProbe(int(min(9.0, t_warm * a.steps) * 1e6), device)
             if (rank == 0 and t_warm and not a.graphs and a.groups == 1) else None)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        frames = step()
    if probe is not None:
        probe.stop()                                  # stream-ordered behind the last step: the probe never outlives the region
    torch.cuda.synchronize()
    own_elapsed = time.perf_counter() - t0            # this rank's own time, before it waits for the others
    power_w = L.gpu_power_w(device) if rank == 0 else None     # the driver's ~1 s average at the end of the last step
    clock_ghz = probe.ghz() if probe is not None else None
    D.barrier()
    elapsed = D.max_over_ranks(time.perf_counter() - t0, device)
    per_rank_clips = [int(v) for v in D.gather_over_ranks(n_own, device)]
    per_rank = [round(c * 30 * a.steps / t, 3) for c, t in zip(per_rank_clips, D.gather_over_ranks(own_elapsed, device))]
    # the range-event word is a bit mask: OR over the ranks (a sum of N ranks' bit 1 would read as another bit)
    events = 0
    for v in D.gather_over_ranks(L.range_events(), device):
        events |= int(v)
    assert frames.shape == (n_own, 30, 3, 128, 128) and bool(torch.isfinite(frames).all())
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, frames, rank, world)
    seen = int(D.sum_over_ranks(1, device))

    # how much of a step is ELIC key-frame decoding (latency-bound: 10 host round trips per batch)
    torch.cuda.synchronize()
    te = time.perf_counter()
    ys = [[[s_ for f in range(2) for s_ in key_strings[f][0][i][p]] for p in range(2)] for i in range(5)]
    zs = [s_ for f in range(2) for s_ in key_strings[f][1]]
    elic.decompress([ys, zs], shape)
    torch.cuda.synchronize()
    elic_ms = (time.perf_counter() - te) * 1e3

    n_frames = sum(per_rank_clips) * 30 * a.steps
    value = n_frames / elapsed
    fwd_per_chunk = {"DDPM": a.subsample + 1, "DDIM": a.subsample + 1, "FPNDM": 12 + (a.subsample - 3)}[a.sampler]
    flop_per_step_gpu = sum(per_rank_clips) / world * (6 * fwd_per_chunk * FWD_FLOP_PER_SAMPLE + 2 * ELIC_DECODE_FLOP)
    policy = {L.ARITH_F32: "fp32 MFMA (v_mfma_f32_32x32x2_f32) everywhere",
              L.ARITH_BF16X6: "conv products as 6 bf16 MFMAs on an exact 3-way bf16 split of both operands",
              L.ARITH_F16X3: "score-network convolutions and attention: operands scaled by powers of two into fp16 range "
                             "(GroupNorm-ed inputs by 8, raw inputs by a bound from their moments, weights per tensor), 2-way "
                             "fp16 split (22 significand bits), 3 fp16 MFMAs per product; input conv, AdaGN tables, ELIC: exact "
                             "3-way bf16 split, 6 bf16 MFMAs"}[L.bounded_arith()]
    out = {"metric": "decoded frames/sec (128x128x30) at q3", "value": round(value, 4), "unit": "frames/s",
           "n_gpus": world, "ranks_seen": seen, "backend": D.backend_name(),
           "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(elapsed / a.steps * 1e3, 2),
           "higher_is_better": True, "scaling": scaling, "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "arithmetic": "fp32 in / fp32 accumulate, fp32-equivalent products (error vs fp64 <= the f32-MFMA path, "
                         "tests/test_gpu_ops.py): " + policy,
           "config": {"workload": workload,
                      "parallelism": f"clip-sharded dp{world}, no data-path collective; {a.groups} concurrent clip "
                                     f"group(s) per GPU; forwards {'replayed from HIP graphs' if a.graphs else 'launched eagerly'}",
                      "weights": "seeded random, reference architecture (262.1M + ELIC)"},
           "per_rank_value": per_rank, "per_rank_clips": per_rank_clips, "range_events": events,
           "range_events_note": "bitwise OR over the ranks of the sticky EVC_RANGE_* word (include/evc_hip.h); 0 = no NaN / inf in any "
                                "tensor and every GroupNorm-ed or moment-bounded fp16-split operand of the score network provably in range",
           "timed_region_first_9s_shader_clock_ghz": None if clock_ghz is None else round(clock_ghz, 3),
           "timed_region_end_package_power_w": None if power_w is None else round(power_w),
           "whole_path_tflops_per_gpu": round(flop_per_step_gpu * a.steps / elapsed / 1e12, 2),
           "whole_path_frac": round(flop_per_step_gpu * a.steps / elapsed / 1e12 / ARITH_INFO[L.bounded_arith()][1], 4),
           "whole_path_frac_note": "whole-job algorithmic FLOP/s per GPU (forwards + ELIC, everything between the barriers) over the "
                                   "roof of the convolution arithmetic in use (f16x3: 833.3)",
           "elic_keyframe_decode_ms_per_step": round(elic_ms, 1)}
    if rank == 0:
        progress(f"timed region: {elapsed:.2f} s for {a.steps} step(s) -> {value:.2f} frames/s; roofline + HBM probes")
        out["roofline"] = roofline_leg(net, n_own, device)
        out["hbm_classes"] = hbm_classes_leg(n_own, device)
        # the CPU baseline runs at N = 1 only: with more ranks the others would wait in a collective for minutes (under
        # torchrun OMP_NUM_THREADS=1 makes it slower still) while the result line is already known
        out["cpu_baseline"] = None if (a.no_cpu_baseline or world > 1) else cpu_baseline_leg(sd_d, sd_e, a.cpu_baseline_seconds)
        if world > 1:
            out["cpu_baseline_note"] = "measured by the single-rank run only (rank 0 at N = 1)"
        print(json.dumps(out), flush=True)
    D.barrier()


if __name__ == "__main__":
    main()
