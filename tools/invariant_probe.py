#!/usr/bin/env python3
"""Full-size score-network forwards in the default and in the batch-invariant mode, one MI355X.

    python tools/invariant_probe.py [--batches 1 2 9 32] [--reps 20] [--table-batch 9] > profiles/invariant_probe.json

Per batch size: the median and the spread (min .. max) of ``--reps`` warm forwards in each mode, timed with HIP events; then THE BAR of the mode -- the invariant forward at B = 9 against nine
default-mode B = 1 forwards, which is the only other way to get batch-independent bits, with the shader clock the chip held meanwhile
(``lib.ClockProbe``) -- and, at ``--table-batch``, the
per-layer table of both modes from the profiled-convolution path (``lib.CONV_PROFILE``): one line per distinct convolution
configuration with its launches, kernel and the summed time of the convolution kernel + its split-K combine, sorted by what
the invariant plan loses.  One JSON line on stdout, the table on stderr.

``--default-only`` times the default mode alone and uses nothing this mode added, so the same file also runs on a checkout
of an earlier commit (copy it there): that is how the parent-commit leg of the bar in profiles/NOTES.md was measured, in
the same session on the same machine.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import evc_amd  # noqa: E402,F401
from evc_amd import lib as L, synthetic  # noqa: E402
from evc_amd.config import default_config  # noqa: E402
from evc_amd.scorenet import ScoreNet  # noqa: E402


def timed(net, x, c, reps, n_forwards=1):
    """Milliseconds of ``reps`` repetitions of ``n_forwards`` back-to-back forwards (HIP events), after 3 warm-up runs."""
    for _ in range(3):
        net.forward_label(x, 500, c)
    torch.cuda.current_stream().synchronize()      # (not the device: the clock probe idles on a stream of its own)
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n_forwards):
            net.forward_label(x, 500, c)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def summary(ms):
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(float(np.min(ms)), 3), max_ms=round(float(np.max(ms)), 3))


def layer_table(net, x, c):
    net.forward_label(x, 500, c)
    prof = []
    L.CONV_PROFILE = prof
    try:
        net.forward_label(x, 500, c)
    finally:
        L.CONV_PROFILE = None
    torch.cuda.synchronize()
    rows = {}
    for r in prof:
        k = r["call"]
        key = (k["H"], k["W"], k["C0"] + k["C1"], k["Co"], k["K"], k["x2"])
        e = rows.setdefault(key, dict(n=0, us=0.0, kernel=r["kernel"], split=r["split"]))
        e["n"] += 1
        e["us"] += r["e0"].elapsed_time(r["e1"]) * 1e3
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 9, 32])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--table-batch", type=int, default=9)
    ap.add_argument("--default-only", action="store_true", help="default mode only (also runs on an earlier commit)")
    a = ap.parse_args()
    L.hip_lib()
    cfg = default_config()
    net = ScoreNet(cfg, synthetic.diffusion_state_dict(cfg, 1234))
    g = torch.Generator(device="cuda").manual_seed(1)
    if a.default_only:
        res = {"forward": {}}
        for B in a.batches:
            x = torch.randn(B, 15, 128, 128, device="cuda", generator=g)
            c = torch.randn(B, 6, 128, 128, device="cuda", generator=g)
            res["forward"][str(B)] = {"default": summary(timed(net, x, c, a.reps))}
        x1, c1 = torch.randn(1, 15, 128, 128, device="cuda", generator=g), torch.randn(1, 6, 128, 128, device="cuda", generator=g)
        res["bar"] = {"nine_default_b1_forwards": summary(timed(net, x1, c1, a.reps, n_forwards=9))}
        print(json.dumps(res))
        return
    inv = net.invariant_view()
    res = {"revision": L.invariant_plan_revision(), "forward": {}}
    for B in a.batches:
        x = torch.randn(B, 15, 128, 128, device="cuda", generator=g)
        c = torch.randn(B, 6, 128, 128, device="cuda", generator=g)
        res["forward"][str(B)] = {"default": summary(timed(net, x, c, a.reps)), "invariant": summary(timed(inv, x, c, a.reps))}
        d, i = res["forward"][str(B)]["default"]["median_ms"], res["forward"][str(B)]["invariant"]["median_ms"]
        res["forward"][str(B)]["invariant_over_default"] = round(i / d, 3)
    # the bar: one invariant B = 9 forward against nine default B = 1 forwards
    x1, c1 = torch.randn(1, 15, 128, 128, device="cuda", generator=g), torch.randn(1, 6, 128, 128, device="cuda", generator=g)
    x9, c9 = torch.randn(9, 15, 128, 128, device="cuda", generator=g), torch.randn(9, 6, 128, 128, device="cuda", generator=g)
    probe = L.ClockProbe(10_000_000)             # the shader clock held during the two sides of the bar
    nine = summary(timed(net, x1, c1, a.reps, n_forwards=9))
    one9 = summary(timed(inv, x9, c9, a.reps))
    res["bar"] = {"nine_default_b1_forwards": nine, "one_invariant_b9_forward": one9,
                  "met": bool(one9["max_ms"] < nine["min_ms"])}
    probe.stop()
    ghz = probe.ghz()
    res["clock_ghz"] = None if ghz is None else round(ghz, 3)
    xb = torch.randn(a.table_batch, 15, 128, 128, device="cuda", generator=g)
    cb = torch.randn(a.table_batch, 6, 128, 128, device="cuda", generator=g)
    td, ti = layer_table(net, xb, cb), layer_table(inv, xb, cb)
    # fuse decisions can differ between the modes (8 x 8): compare by resolution and filter, list per configuration
    print(f"per-layer table at B = {a.table_batch}: H W Cin Co K x2 | launches | default us (kernel) | invariant us (kernel)",
          file=sys.stderr)
    keys = sorted(set(td) | set(ti), key=lambda k: -(ti.get(k, {"us": 0})["us"] - td.get(k, {"us": 0})["us"]))
    table = []
    for k in keys:
        d, i = td.get(k), ti.get(k)
        line = dict(layer=list(k), launches=(i or d)["n"], default_us=None if d is None else round(d["us"], 1),
                    default_kernel=None if d is None else d["kernel"], invariant_us=None if i is None else round(i["us"], 1),
                    invariant_kernel=None if i is None else i["kernel"])
        table.append(line)
        print(" ".join(f"{v:5d}" for v in k), "|", line["launches"], "|", line["default_us"], line["default_kernel"], "|",
              line["invariant_us"], line["invariant_kernel"], file=sys.stderr)
    res["conv_us_total"] = {"default": round(sum(v["us"] for v in td.values()), 1),
                            "invariant": round(sum(v["us"] for v in ti.values()), 1)}
    res["table"] = table
    print(json.dumps(res))


if __name__ == "__main__":
    main()
