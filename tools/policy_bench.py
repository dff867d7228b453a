#!/usr/bin/env python3
"""Throughput of the reference's REAL workload on one MI355X: the sender's policy sweep (city_sender.py:495-607) -- per
video 2 quality indexes x 28 thresholds = 56 (video, q, threshold) jobs, each a receiver loop of key frames and generated
chunks -- through ``evc_amd.policy.run_policy``, which advances all jobs in lockstep and stacks them along the batch axis
of the score-network launches.  The reference runs the 56 jobs one after another (and reloads the 1 GB checkpoint per
chunk).  Synthetic clips, seeded weights of the reference architecture, the PSNR rule (LPIPS needs AlexNet weights that
are not available offline); thresholds are spread over the PSNR range the generated frames actually reach, so that the
sweep contains both accepted chunks and key-frame fall-backs like a real one.

    python tools/policy_bench.py [--videos 1] [--subsample 100] [--max-batch 32] [--noise torch|evc] [--share] > profiles/r03_policy_bench.json

``--noise evc`` runs the sweep on the replayable noise of specification N1 (one HIP launch per sampler step for the whole batch)
instead of one seeded torch.Generator per (job, round, step); the JSON line also reports the host seconds spent drawing noise and
the noise kernel's write rate at B = 32.  ``--share`` runs the sweep with one noise stream per (video, q) and one generated sample
per distinct state of a round (``run_policy(noise_streams="group", share=True)``); ``--noise-streams group`` alone keys the noise
by group without sharing, the control the shared frames are compared with.  ``sample_forwards`` counts samples that went through
the score network, so states under ``--share``.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import evc_amd  # noqa: E402,F401
from evc_amd import lib as L, policy as P, sampler as S, synthetic  # noqa: E402
from evc_amd.config import default_config  # noqa: E402
from evc_amd.decoder import ClipDecoder  # noqa: E402
from evc_amd.elic import ElicModel  # noqa: E402
from evc_amd.scorenet import ScoreNet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=1)
    ap.add_argument("--subsample", type=int, default=100)
    ap.add_argument("--max-batch", type=int, default=32)
    ap.add_argument("--qs", type=int, nargs="+", default=[4, 5])             # city_sender.py:504 q range of the sweep
    ap.add_argument("--n-thresholds", type=int, default=28)                  # city_sender.py:505-508
    ap.add_argument("--noise", choices=["torch", "evc"], default="torch")
    ap.add_argument("--batch-invariant", action="store_true",
                    help="run the sweep in the score network's batch-invariant mode (needs --noise evc)")
    ap.add_argument("--share", action="store_true",
                    help="generate once per distinct state of a round (selects --noise-streams group)")
    ap.add_argument("--noise-streams", choices=["job", "group"], default=None,
                    help="job (default): one noise stream per job; group: one per (video, q)")
    a = ap.parse_args()
    if a.share and a.noise_streams == "job":
        ap.error("--share needs --noise-streams group")
    a.noise_streams = a.noise_streams or ("group" if a.share else "job")
    L.hip_lib()
    cfg = default_config(192, 192, 128, subsample=a.subsample)
    net = ScoreNet(cfg, synthetic.diffusion_state_dict(cfg, 1234))
    models = {q: ElicModel(synthetic.elic_state_dict(q)) for q in a.qs}
    dec = ClipDecoder(net, models[a.qs[0]], cfg, S.get_sampler("DDPM"))
    clips = {v: torch.from_numpy(synthetic.make_clips(1, seed=200 + v)[0].astype(np.float32) / 255.0) for v in range(a.videos)}
    # probe: one all-accepting job at 10 sampler steps to find the PSNR range generated frames reach on this data
    probe_cfg = default_config(192, 192, 128, subsample=10)
    pdec = ClipDecoder(net, models[a.qs[0]], probe_cfg, S.get_sampler("DDPM"))
    r = P.run_policy(pdec, models, {0: clips[0]}, a.qs[:1], [-1e9], P.PsnrMetric(), max_batch=a.max_batch)
    x = r[(0, a.qs[0])][0]["x"]
    ps = [P.cal_psnr(x[f], clips[0][f].numpy()) for f in range(2, 30)]
    lo, hi = float(np.min(ps)) - 1.0, float(np.max(ps)) + 1.0
    thresholds = [float(t) for t in np.linspace(lo, hi, a.n_thresholds)]
    torch.cuda.synchronize()
    stats = {}
    t0 = time.perf_counter()
    res = P.run_policy(dec, models, clips, a.qs, thresholds, P.PsnrMetric(), max_batch=a.max_batch, stats=stats, noise=a.noise,
                       batch_invariant=a.batch_invariant, noise_streams=a.noise_streams, share=a.share,
                       log=lambda m: print(f"[policy_bench {time.strftime('%H:%M:%S')}] {m}", file=sys.stderr, flush=True))
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    # the noise kernel alone: one sampler step of a full launch, B = 32 samples of 15 x 128 x 128 (31 MB written)
    keys = L.noise_keys([(i, 2) for i in range(32)], "cuda")
    buf = torch.empty((32, 15, 128, 128), device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(5):
        L.noise_normal(keys, buf.shape, 1234, 1, out=buf)
    ev[0].record()
    for i in range(100):
        L.noise_normal(keys, buf.shape, 1234, i, out=buf)
    ev[1].record()
    torch.cuda.synchronize()
    noise_us = ev[0].elapsed_time(ev[1]) * 1e3 / 100
    jobs = a.videos * len(a.qs) * len(thresholds)
    kept = sum(len(v) for v in res.values())
    gen = sum(int((r_["d"] == 0).sum()) for v in res.values() for r_ in v)
    launches = sum(stats["launch_sizes"].values())
    fwd = launches * (a.subsample + 1)
    samples = sum(k * n for k, n in stats["launch_sizes"].items()) * (a.subsample + 1)
    print(json.dumps({
        "workload": f"{a.videos} video(s) x q {a.qs} x {len(thresholds)} PSNR thresholds = {jobs} sender jobs of 30 frames "
                    f"(city_sender.py:495-607), DDPM-{a.subsample}, full-size network, synthetic clips / seeded weights",
        "noise": a.noise, "batch_invariant": a.batch_invariant, "share": a.share, "noise_streams": a.noise_streams,
        "seconds": round(el, 2), "noise_host_seconds": round(stats.get("noise_host_seconds", 0.0), 3),
        "noise_kernel_b32_us": round(noise_us, 2), "noise_kernel_b32_tb_per_s": round(buf.numel() * 4 / noise_us / 1e6, 3),
        "jobs": jobs, "jobs_per_s": round(jobs / el, 3),
        "decoded_frames_per_s": round(jobs * 30 / el, 2),
        "jobs_below_1bpp": kept, "generated_frames_kept": gen,
        "generation_rounds": stats.get("rounds"), "generation_launches": launches,
        "launch_size_histogram": {str(k): v for k, v in sorted(stats["launch_sizes"].items())},
        "states_per_round": stats["states"], "jobs_served_per_round": stats["jobs_served"],
        "score_network_forwards": fwd, "sample_forwards": samples,
        "sample_forwards_per_s": round(samples / el, 1),
        "key_frames_coded": stats.get("key_frames_coded"),
        "thresholds_psnr_db": [round(t, 2) for t in thresholds],
        "range_events": L.range_events(),
        "note": "the reference would run these jobs one at a time at B=1 per launch; here up to max_batch jobs share a launch"}))


if __name__ == "__main__":
    main()
