#!/usr/bin/env python3
"""Generate tests/golden/fid_pr.npz by running the REFERENCE's own precision / recall code on the CPU.

Nothing from the reference is copied: this script loads its evaluation/pr.py by path (that file imports only torch), runs
calculate_precision_recall -- the full and the part form -- on the seeded feature sets of tests/fid_recipe.py and stores the
seeds, shapes, k and the two values (``reference``: as the reference returns them, the fp32 mean of the flags; ``values``: the
same multiples of 1 / m and 1 / n in float64).  A feature set enters the golden only if, in float64, no distance lies within 1e-3 relative
of the radius it is compared with (fid_recipe.min_gap): the reference's fp32 cdist is good to about 1e-6, so its decisions are
then those of exact arithmetic.  The tests rebuild the sets from the same recipe and re-assert the condition.

    python tests/golden/make_fid_golden.py REFERENCE_DIR
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import fid_recipe as R  # noqa: E402  (seed recipe shared with the tests)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    spec = importlib.util.spec_from_file_location("ref_pr", os.path.join(sys.argv[1], "evaluation", "pr.py"))
    pr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pr)
    sets, values, reference = [], [], []
    for seed, n, m, d, shift, k in R.PR_SETS:
        real, gen = R.feature_sets(seed, n, m, d, shift)
        gap = R.min_gap(real, gen, k)
        assert gap > R.GAP_BAR, (seed, n, m, d, shift, gap)
        tr, tg = torch.from_numpy(real), torch.from_numpy(gen)
        full = pr.calculate_precision_recall(tr, tg, device=torch.device("cpu"), k=k)
        part = pr.calculate_precision_recall(tr, tg, device=torch.device("cpu"), k=k, save_cpu_ram=True)
        f64 = R.precision_recall(real, gen, k)
        assert tuple(full) == tuple(part) and np.allclose(full, f64, rtol=0, atol=1e-7), (full, part, f64)
        print(f"seed {seed} n {n} m {m} d {d} shift {shift} k {k}: gap {gap:.2e} precision {full[0]:.6f} recall {full[1]:.6f}")
        sets.append([seed, n, m, d, k])
        values.append([shift, f64[0], f64[1], gap])
        reference.append([full[0], full[1], part[0], part[1]])
    np.savez(os.path.join(HERE, "fid_pr.npz"), sets=np.asarray(sets, dtype=np.int64), values=np.asarray(values, dtype=np.float64),
             reference=np.asarray(reference, dtype=np.float64))


if __name__ == "__main__":
    main()
