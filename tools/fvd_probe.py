"""Times one I3D forward (evc_amd/fvd.py, seeded weights, 30-frame 128^2 clips) at a few clip counts with HIP events and
prints the time per clip and TFLOP/s against 105.5 GFLOP per clip (2 FLOP per MAC).

    python tools/fvd_probe.py [clip counts ...]        # default 1 4 8
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import evc_amd  # noqa: E402,F401
import i3d_recipe as R  # noqa: E402
from evc_amd import fvd, lib as L  # noqa: E402

counts = [int(a) for a in sys.argv[1:]] or [1, 4, 8]
net = fvd.I3d(R.seeded_state_dict(), device="cuda:0", max_clips=max(counts))
clips = torch.from_numpy(np.random.default_rng(0).random((max(counts), 30, 3, 128, 128), dtype=np.float32)).cuda()
probe = L.ClockProbe(2000000)
for n in counts:
    x = clips[:n].contiguous()
    for _ in range(2):
        net(x)
    reps = 5
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        net(x)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    print(f"clips {n}: {ms:.2f} ms per forward, {ms / n:.2f} ms per clip, "
          f"{fvd.FLOPS_PER_CLIP_30 * n / (ms * 1e-3) / 1e12:.1f} TFLOP/s", flush=True)
probe.stop()
torch.cuda.synchronize()
print(f"shader clock during the probe: {probe.ghz():.2f} GHz")
