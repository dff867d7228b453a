"""Dump every answer of the convolution planner's query entry points over a fixed sweep of argument sets: one deterministic
text line per set.  CPU only (no device, no launch).  For dispatch refactors: the dump of a change must equal the dump of its
parent, which is taken with the same script against the parent's library:

    python tools/conv_plan_dump.py > change.txt
    EVC_HIP_SO=<in-tree path of the parent's libevc_hip.so> python tools/conv_plan_dump.py > parent.txt
    python tools/conv_plan_dump.py --compare parent.txt change.txt      # differing rows (the first 20, or --all), status 1 if any

The sweep:
  - FULL_SIZE_CONVS x B = 1..64 x {own arithmetic, bf16x6, f32} x invariant {0, 1} x forced splits {0, 1, 2, 3, 7}, with the
    listed fused channels and with 0;
  - the same at B in {1, 2, 8, 9, 32} with each of the six evc_conv_set_option switches turned off in turn;
  - every conv_ledger.CASES and conv_ledger.NAMED entry;
  - the on-load grid (coefficients yes / no x activation none / SiLU / ReLU) on one 3x3 and one 1x1 shape per image size.
"""
import ctypes
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

OPTIONS = ("wide_tiles", "row_reuse", "tail_split", "wide256", "wide_mid", "wide_cut")
F32, BF16 = 0, 1


def row(L, H, tag, B, Hh, W, C0, C1, Co, K, arith, coef, act, splits, x2, inv):
    """One line: the arguments, then every query's return code and answer."""
    a = L.conv_query_args(B, Hh, W, C0, C1, Co, K, K, arith, coef=bool(coef), act_in=act, splits=splits, x2_ci=x2,
                          invariant=bool(inv))
    ref = ctypes.byref(a)
    plan = L.ConvPlan()
    rc = H.evc_conv_plan_query(ref, ctypes.byref(plan))
    fields = "" if rc else ":%s,%d,%d,%d,%d,%d,%d,%d,%d,%d" % (
        plan.kernel.decode(), plan.tile_m, plan.tile_n, plan.splits, plan.steps_per_split, plan.cut_chunk, plan.tail_tiles,
        plan.tail_splits, plan.stats_runs, plan.fused_1x1)
    buf = ctypes.create_string_buffer(96)
    n = H.evc_conv_kernel_name(ref, buf, 96)
    name = "%d:%s" % (n, buf.value.decode()) if n >= 0 else str(n)
    return "%s %d %d %d %d %d %d %d a%d c%d t%d s%d x%d i%d | plan=%d%s | splits=%d | name=%s | stats=%d | ws=%d | fused=%d" % (
        tag, B, Hh, W, C0, C1, Co, K, arith, bool(coef), act, splits, x2, bool(inv), rc, fields, H.evc_conv_choose_splits(ref),
        name, H.evc_conv_stats_splits(ref), H.evc_conv_workspace_bytes(ref), H.evc_conv_fused_1x1_supported(ref))


def product(L, H, tag, batches):
    from test_invariant_plan import FULL_SIZE_CONVS
    for (Hh, W, C0, C1, Co, K, ar, coef, act, x2, _bound) in FULL_SIZE_CONVS:
        for arith in (ar, BF16, F32):
            for inv in (0, 1):
                for splits in (0, 1, 2, 3, 7):
                    for x2_ci in sorted({x2, 0}):
                        for B in batches:
                            yield row(L, H, tag, B, Hh, W, C0, C1, Co, K, arith, coef, act, splits, x2_ci, inv)


def dump():
    import evc_amd  # noqa: F401
    from evc_amd import lib as L
    import conv_ledger as ledger
    from test_invariant_plan import FULL_SIZE_CONVS
    H = L.hip_lib(require_device=False)
    yield from product(L, H, "default", range(1, 65))
    for opt in OPTIONS:
        L.conv_set_option(opt, 0)
        try:
            yield from product(L, H, "no_" + opt, (1, 2, 8, 9, 32))
        finally:
            L.conv_set_option(opt, 1)
    for c in ledger.CASES:
        yield row(L, H, "case", c.B, c.H, c.W, c.C0, c.C1, c.Co, c.K, c.arith, c.coef, c.act, c.splits, c.x2, c.invariant)
    for n in ledger.NAMED:
        yield row(L, H, "named", n.B, n.H, n.W, n.C0, n.C1, n.Co, n.K, n.arith, n.coef, n.act, n.splits, n.x2, 0)
    seen = set()
    for (Hh, W, C0, C1, Co, K, ar, _coef, _act, _x2, _bound) in FULL_SIZE_CONVS:
        if (Hh, W, K) in seen:
            continue
        seen.add((Hh, W, K))
        for coef in (0, 1):
            for act in (L.ACT_NONE, L.ACT_SILU, L.ACT_RELU):
                for inv in (0, 1):
                    for B in (1, 9):
                        yield row(L, H, "onload", B, Hh, W, C0, C1, Co, K, ar, coef, act, 0, 0, inv)


def compare(parent, change):
    a, b = (open(p).read().splitlines() for p in (parent, change))
    diff = [(x, y) for x, y in zip(a, b) if x != y]
    for x, y in diff[:None if "--all" in sys.argv else 20]:
        print("- " + x + "\n+ " + y)
    refused = sum(1 for _, y in diff if re.search(r"plan=(-\d+) \| splits=\1 \| name=\1 \| stats=0 \| ws=\1 \| fused=0$", y))
    print(f"{len(a)} / {len(b)} rows, {len(diff)} differ, {refused} of them refused by every query of the second dump")
    return int(bool(diff) or len(a) != len(b))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--compare"]:
        sys.exit(compare(*sys.argv[2:4]))
    sys.stdout.write("".join(line + "\n" for line in dump()))
