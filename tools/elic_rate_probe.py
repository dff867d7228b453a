"""Estimated against coded rate of ELIC key frames, and what each path costs: the synthetic q3 checkpoint (with its density), 8
key frames of 128x128 per batch.  Prints per frame the estimated bits (ElicModel.estimate: sum of -log2 likelihood) beside the
coded bits (8 x string lengths), and the wall time per key frame of ``policy.coded_batch`` and ``policy.estimated_batch``: host
clock around calls that end synchronised (both read their result back), the two paths alternating inside every round, the
median over the rounds after a warm-up.  One JSON line at the end.

    python tools/elic_rate_probe.py [--q 3] [--frames 8] [--rounds 9] [--calls 5]
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
from evc_amd import lib as L, policy as P, synthetic  # noqa: E402
from evc_amd.elic import ElicModel  # noqa: E402


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--q", type=int, default=3)
    p.add_argument("--frames", type=int, default=8)
    p.add_argument("--rounds", type=int, default=9)
    p.add_argument("--calls", type=int, default=5, help="calls of each path per round")
    a = p.parse_args()
    L.hip_lib()
    model = ElicModel(synthetic.elic_state_dict_with_density(a.q))
    clip = synthetic.make_clips(1, seed=0)[0]
    x = torch.from_numpy(clip[:a.frames].astype(np.float32) / 255.0).cuda()
    coded = lambda: P.coded_batch(model, x, 64)
    estimated = lambda: P.estimated_batch(model, x, 64)
    xc, bits_c, _, _ = coded()
    xe, bits_e, _, _ = estimated()
    assert torch.equal(xc, xe), "the two paths decode different frames"
    for f, (c, e) in enumerate(zip(bits_c, bits_e)):
        print(f"frame {f}: estimated {e:.2f} bits, coded {c} bits, coded - estimated {c - e:+.2f} ({(c - e) / e:+.2%})", flush=True)
    for _ in range(2):                                   # warm-up of both paths
        timed(coded, a.calls), timed(estimated, a.calls)
    tc, te = [], []
    for _ in range(a.rounds):                            # alternate inside every round: drift hits both alike
        tc.append(timed(coded, a.calls))
        te.append(timed(estimated, a.calls))
    med = lambda v: sorted(v)[len(v) // 2]
    n = x.shape[0]
    print(json.dumps({
        "q": a.q, "frames_per_batch": n, "rounds": a.rounds, "calls_per_round": a.calls,
        "estimated_bits_per_frame": [round(b, 3) for b in bits_e], "coded_bits_per_frame": [int(b) for b in bits_c],
        "coded_over_estimated": round(sum(bits_c) / sum(bits_e), 5),
        "coded_ms_per_frame_median": round(1e3 * med(tc) / n, 4), "coded_ms_per_frame_min_max": [round(1e3 * min(tc) / n, 4), round(1e3 * max(tc) / n, 4)],
        "estimated_ms_per_frame_median": round(1e3 * med(te) / n, 4), "estimated_ms_per_frame_min_max": [round(1e3 * min(te) / n, 4), round(1e3 * max(te) / n, 4)],
        "coded_over_estimated_time": round(med(tc) / med(te), 3)}), flush=True)


if __name__ == "__main__":
    main()
