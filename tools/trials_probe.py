#!/usr/bin/env python3
"""Rate against the number of noise trials, and the sender's metric on the device against the host (one MI355X).

    python tools/trials_probe.py [--full] [--videos 1] [--subsample N] [--n-thresholds 8] [--max-batch 32] > profiles/trials_probe.json

Part 1: one policy sweep (``policy.run_policy``, batch-invariant, shared rounds, PSNR rule on ``PsnrDeviceMetric``) per K in
1, 2, 4, 8 over ONE threshold grid -- spread over the PSNR range an all-accepting K = 1 job reaches -- on seeded random weights:
the reduced network of the tests (ngf 32, DDPM-2) by default, the reference architecture with ``--full`` (DDPM-``--subsample``,
default 10).  Per K: key frames coded, mean bpp including the trial bits, generated samples, sender seconds.  The generators
are random-weight stand-ins: the figures show the mechanism and its cost, they say nothing about the real checkpoints.

Part 2: ``PsnrDeviceMetric.values`` against ``PsnrMetric.values`` on n = 160 candidate frames of 3 x 128 x 128 (one 32-sample
launch of 5 frames): wall-clock seconds per call including the read-back, median of 20 calls after 3 warm-up calls.

Prints one JSON line; a table of part 1 goes to stderr."""
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

KS = (1, 2, 4, 8)


def metric_seconds(metric, pred, gt, calls=20, warmup=3):
    times = []
    for i in range(warmup + calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        metric.values(pred, gt)
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(time.perf_counter() - t0)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--full", action="store_true", help="the reference architecture (ngf 192) instead of the reduced network")
    ap.add_argument("--videos", type=int, default=1)
    ap.add_argument("--subsample", type=int, default=None, help="sampler steps (default: 2 reduced, 10 full)")
    ap.add_argument("--n-thresholds", type=int, default=8)
    ap.add_argument("--max-batch", type=int, default=32)
    ap.add_argument("--q", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    a = ap.parse_args()
    L.hip_lib()
    steps = a.subsample or (10 if a.full else 2)
    if a.full:
        cfg = default_config(192, 192, 128, subsample=steps)
        net = ScoreNet(cfg, synthetic.diffusion_state_dict(cfg, 1234))
    else:
        from oracle import scorenet as ON
        cfg = default_config(32, 32, 128, subsample=steps)
        net = ScoreNet(cfg, ON.seeded_params(ON.Dims(ngf=32, n_head_channels=32, image_size=128), 3))
    models = {a.q: ElicModel(synthetic.elic_state_dict(a.q))}
    dec = ClipDecoder(net, None, cfg, S.get_sampler("DDPM"))
    clips = {v: torch.from_numpy(synthetic.make_clips(v + 1, seed=11)[v].astype(np.float32) / 255) for v in range(a.videos)}
    common = dict(max_batch=a.max_batch, seed=a.seed, bpp_limit=1e9, noise="evc", batch_invariant=True, noise_streams="group",
                  share=True)
    probe = P.run_policy(dec, models, {0: clips[0]}, [a.q], [-1e9], P.PsnrDeviceMetric(), **common)
    ps = [P.cal_psnr(probe[(0, a.q)][0]["x"][t], clips[0][t].numpy()) for t in range(2, 30)]
    thresholds = [float(t) for t in np.linspace(min(ps) - 0.02, float(np.percentile(ps, 60)), a.n_thresholds)]
    rows = []
    for k in KS:
        stats = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = P.run_policy(dec, models, clips, [a.q], thresholds, P.PsnrDeviceMetric(), stats=stats, trials=k, **common)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        jobs = [r for lst in res.values() for r in lst]
        rows.append({"trials": k, "key_frames": sum(int(r["d"].sum()) for r in jobs),
                     "key_frames_coded": stats["key_frames_coded"],
                     "mean_bpp": float(np.mean([r["bpp"] for r in jobs])),
                     "trial_bits": sum(r["trial_bits"] for r in jobs),
                     "generated_samples": sum(n * c for n, c in stats["launch_sizes"].items()),
                     "sender_seconds": round(el, 3)})
    print(f"{'K':>2} {'key frames':>10} {'coded once':>10} {'mean bpp':>9} {'trial bits':>10} {'samples':>8} {'seconds':>8}",
          file=sys.stderr)
    for r in rows:
        print(f"{r['trials']:>2} {r['key_frames']:>10} {r['key_frames_coded']:>10} {r['mean_bpp']:>9.5f} {r['trial_bits']:>10} "
              f"{r['generated_samples']:>8} {r['sender_seconds']:>8.2f}", file=sys.stderr)
    g = torch.Generator(device="cuda").manual_seed(1)
    gt = torch.rand((160, 3, 128, 128), device="cuda", generator=g)
    pred = (gt + 0.05 * torch.randn(gt.shape, device="cuda", generator=g)).clamp(0, 1)
    dev_s, host_s = metric_seconds(P.PsnrDeviceMetric(), pred, gt), metric_seconds(P.PsnrMetric(), pred, gt)
    gap = float(np.abs(P.PsnrDeviceMetric().values(pred, gt) - P.PsnrMetric().values(pred, gt)).max())
    print(f"metric on 160 frames of 3x128x128: device {dev_s * 1e6:.0f} us, host {host_s * 1e6:.0f} us, max |dB gap| {gap:.2e}",
          file=sys.stderr)
    print(json.dumps({
        "workload": f"{a.videos} video(s) x q {a.q} x {len(thresholds)} PSNR thresholds, DDPM-{steps}, "
                    f"{'full-size' if a.full else 'reduced (ngf 32)'} network, seeded random weights, batch-invariant, shared rounds",
        "thresholds_psnr_db": [round(t, 3) for t in thresholds], "per_trials": rows,
        "metric_n160": {"device_seconds": dev_s, "host_seconds": host_s, "max_abs_db_gap": gap},
        "range_events": L.range_events(),
        "note": "random-weight generators: these rate figures say nothing about the real checkpoints"}))


if __name__ == "__main__":
    main()
