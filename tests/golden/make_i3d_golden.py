#!/usr/bin/env python3
"""Generate tests/golden/i3d_fvd.npz by running the REFERENCE's own I3D and FVD code on CPU.

Runs ONLY in the build container, where the reference is mounted read-only at /root/reference (it does not exist on the GPU
box).  Nothing from the reference is copied: this script imports models/fvd/pytorch_i3d.py and models/fvd/fvd.py, builds
InceptionI3d(400), fills it with the seeded recipe of tests/i3d_recipe.py, and runs preprocess_single + forward on the seeded
clips of that module and frechet_distance on the resulting logits.  It stores seeds, logits, end-point checksums and FVD
values only (no weights, no videos); the tests rebuild weights and clips from the same recipe.  It also checks that the
torch restatement in tests/i3d_recipe.py (the GPU tests' CPU reference) computes what the reference module computes.

    python tests/golden/make_i3d_golden.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REF = "/root/reference/models/fvd"
sys.path.insert(0, TESTS)

import i3d_recipe as R  # noqa: E402  (seed recipe shared with the tests)


def load(name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(REF, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    pi3d, rfvd = load("pytorch_i3d"), load("fvd")
    net = pi3d.InceptionI3d(400, in_channels=3).eval()
    sd = R.seeded_state_dict()
    ref_keys = {k for k in net.state_dict() if not k.endswith("num_batches_tracked")}
    assert ref_keys == set(sd), sorted(ref_keys ^ set(sd))
    net.load_state_dict(sd, strict=False)

    logits, sums = [], {}
    for i, (seed, T, H, W) in enumerate(R.CLIPS):
        v = R.clip(seed, T, H, W)
        with torch.no_grad():
            # get_logits: i3d(preprocess_single(video).unsqueeze(0)), video (C, T, H, W)
            out = net(rfvd.preprocess_single(v.permute(1, 0, 2, 3)).unsqueeze(0))
        mine, eps = R.forward(sd, v[None])
        err = float((mine - out).abs().max() / out.abs().max())
        print(f"clip {i} (T={T}, {H}x{W}): |logit| max {float(out.abs().max()):.4f}, restatement rel err {err:.2e}")
        assert err < 1e-5, err
        logits.append(out[0].numpy().astype(np.float64))
        if i in (0, len(R.CLIPS) - 1):
            sums[i] = np.stack([R.checksums(eps[e]) for e in R.END_POINTS])
    f = np.stack(logits)
    fvd_rep2 = rfvd.frechet_distance(np.stack([f[0], f[0]]), np.stack([f[1], f[1]]))   # city_sender.py:575-577 pairing
    fvd_set = rfvd.frechet_distance(f[[0, 1, 2]], f[[3, 4, 5]])
    print(f"fvd repeat-2 {fvd_rep2:.6f}  (|mu diff|^2 {np.square(f[0] - f[1]).sum():.6f}), fvd 3 vs 3 {fvd_set:.6f}")
    np.savez_compressed(os.path.join(HERE, "i3d_fvd.npz"), weight_seed=np.int64(R.WEIGHT_SEED),
                        clips=np.array(R.CLIPS, dtype=np.int64), logits=f, end_points=np.array(R.END_POINTS),
                        checksums_first=sums[0], checksums_last=sums[len(R.CLIPS) - 1],
                        fvd_rep2=np.float64(fvd_rep2), fvd_set=np.float64(fvd_set),
                        set_a=np.array([0, 1, 2]), set_b=np.array([3, 4, 5]))


if __name__ == "__main__":
    main()
