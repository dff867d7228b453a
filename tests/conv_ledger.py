"""The ledger of convolution plan classes: which kernel instance, split kind and tile geometry every op-level parity case
reaches, and which of them the full-size network launches.  A plain module (no fixtures): tests/test_conv_ledger_host.py checks
the table against the planner on the CPU, tests/test_gpu_conv_ledger.py runs every entry against an fp64 reference.

A plan class is the tuple

    (kernel instance, split kind, partial last pixel tile, (image width, tile spans images) or None, fused 1x1 operand,
     batch-invariant plan)

- kernel instance: the name ``evc_conv_kernel_name`` reports, on-load mode included (the last template argument; the first of
  conv_wide_kernel);
- split kind: "none", "z" (uniform K split over blockIdx.z + combine), "tail" (K-split tail of the partial last round) or
  "cut" (two unequal K pieces of conv_wide_kernel);
- the batch-invariant flag is part of the class: the same kernel instance then reads one bound word per sample;
- the width field is set for the kernels whose tiles are made of whole image rows (row-reuse and wide), None otherwise.

``python tests/conv_ledger.py`` searches the planner for the cheapest case of every class the product reaches and prints the
``CASES`` table; run it again when the planner moves a class and paste the result.
"""
from collections import namedtuple

from test_invariant_plan import FULL_SIZE_CONVS

F32, BF16, F16 = 0, 1, 2          # lib.ARITH_F32 / ARITH_BF16X6 / ARITH_F16X3
NONE, SILU = 0, 1                 # lib.ACT_NONE / ACT_SILU
ROW_KERNELS = ("conv_split_rr_kernel", "conv_wide_kernel")
SPLIT_KINDS = ("none", "z", "tail", "cut")

# shape, arithmetic, on-load mode (GroupNorm coefficients, activation), forced splits, channels of the fused 1x1 operand, the
# batch-invariant flag, whether the raw operand carries an element bound, and the class the planner must map it to
Case = namedtuple("Case", "B H W C0 C1 Co K arith coef act splits x2 invariant bound cls")


def lib():
    import evc_amd  # noqa: F401
    from evc_amd import lib as L
    L.hip_lib(require_device=False)
    return L


def classify(p, B, H, W, x2_ci, invariant=False):
    """The class tuple of a plan dict of ``lib.conv_plan``."""
    kind = "tail" if p["tail_tiles"] else "cut" if p["cut_chunk"] else "z" if p["splits"] > 1 else "none"
    bm = p["tile"][0]
    rows = (W, (H * W) % bm != 0) if p["kernel"].split("<")[0] in ROW_KERNELS else None
    return (p["kernel"], kind, (B * H * W) % bm != 0, rows, bool(x2_ci), bool(invariant))


def plan_class(B, H, W, C0, C1, Co, K, arith, coef, act_in, splits, x2_ci, invariant, L=None):
    L = L or lib()
    p = L.conv_plan(B, H, W, C0, C1, Co, K, arith, coef=bool(coef), act_in=act_in, x2_ci=x2_ci, invariant=bool(invariant),
                    splits=splits)
    return classify(p, B, H, W, x2_ci, invariant)


def case_class(c, L=None):
    return plan_class(c.B, c.H, c.W, c.C0, c.C1, c.Co, c.K, c.arith, c.coef, c.act, c.splits, c.x2, c.invariant, L)


def ignore_mode(cls):
    """The class with the on-load mode left out: the last template argument of the kernel, the first of conv_wide_kernel."""
    name, args = cls[0].rstrip(">").split("<")
    args = args.split(", ")
    args = args[1:] if name == "conv_wide_kernel" else args[:-1]
    return (f"{name}<{', '.join(args)}>",) + tuple(cls[1:])


def product_launches(L=None):
    """Every (Case without class) the full-size forward launches: FULL_SIZE_CONVS x B = 1..32 (default mode) or B in {1, 2, 9, 32}
    (invariant mode) x {the layer's own arithmetic, bf16x6}.  The fused 1x1 operand exists on the fp16 split only; where the
    plan refuses it (64-pixel tiles) the network launches the 3x3 convolution without it and the 1x1 skip convolution on its own."""
    L = L or lib()
    for invariant, batches in ((False, range(1, 33)), (True, (1, 2, 9, 32))):
        for (H, W, C0, C1, Co, K, ar, coef, act, x2, bound) in FULL_SIZE_CONVS:
            for arith in sorted({ar, BF16}):
                for B in batches:
                    x2_ci = x2 if arith == F16 else 0
                    if x2_ci and not L.conv_plan(B, H, W, C0, C1, Co, K, arith, coef=bool(coef), act_in=act, x2_ci=x2_ci,
                                                 invariant=invariant)["fused_1x1"]:
                        yield Case(B, H, W, x2_ci, 0, Co, 1, arith, 0, NONE, 0, 0, invariant, 1, None)
                        x2_ci = 0
                    yield Case(B, H, W, C0, C1, Co, K, arith, coef, act, 0, x2_ci, invariant, int(bound and arith == F16), None)


def product_classes(L=None):
    L = L or lib()
    return {case_class(c, L) for c in product_launches(L)}


def macs(c):
    return c.B * c.H * c.W * c.Co * (c.K * c.K * (c.C0 + c.C1) + c.x2)


# One case per plan class the product reaches (``product_classes``), the cheapest the planner maps to it, then the cases the
# older tests promise but no longer run: the row-reuse kernel at W = 4 and W = 8 x 129 images under both split arithmetics.
CASES = [
    Case(1, 32, 32, 16, 0, 192, 1, 1, 0, 0, 0, 0, False, 0,
         ('conv_split_kernel<1, 3, 0>', 'none', False, None, False, False)),
    Case(2, 32, 32, 16, 0, 192, 1, 1, 0, 0, 0, 0, True, 0,
         ('conv_split_kernel<1, 3, 0>', 'none', False, None, False, True)),
    Case(1, 8, 8, 176, 16, 192, 1, 1, 0, 0, 0, 0, False, 0,
         ('conv_split_kernel<1, 3, 0>', 'z', False, None, False, False)),
    Case(2, 8, 8, 176, 16, 192, 1, 1, 0, 0, 0, 0, True, 0,
         ('conv_split_kernel<1, 3, 0>', 'z', False, None, False, True)),
    Case(1, 32, 32, 16, 0, 192, 1, 1, 1, 0, 0, 0, False, 0,
         ('conv_split_kernel<1, 3, 1>', 'none', False, None, False, False)),
    Case(2, 16, 16, 16, 0, 192, 1, 1, 1, 0, 0, 0, True, 0,
         ('conv_split_kernel<1, 3, 1>', 'none', False, None, False, True)),
    Case(1, 8, 8, 176, 16, 192, 1, 1, 1, 0, 0, 0, False, 0,
         ('conv_split_kernel<1, 3, 1>', 'z', False, None, False, False)),
    Case(2, 8, 8, 176, 16, 192, 1, 1, 1, 0, 0, 0, True, 0,
         ('conv_split_kernel<1, 3, 1>', 'z', False, None, False, True)),
    Case(1, 8, 8, 16, 16, 192, 3, 1, 1, 1, 0, 0, False, 0,
         ('conv_split_kernel<1, 3, 2>', 'z', False, None, False, False)),
    Case(33, 32, 32, 16, 0, 192, 1, 1, 0, 0, 0, 0, False, 0,
         ('conv_split_kernel<2, 3, 0>', 'none', False, None, False, False)),
    Case(11, 32, 32, 16, 0, 576, 1, 1, 1, 0, 0, 0, False, 0,
         ('conv_split_kernel<2, 3, 1>', 'none', False, None, False, False)),
    Case(2, 32, 32, 16, 0, 768, 1, 1, 1, 0, 0, 0, True, 0,
         ('conv_split_kernel<2, 3, 1>', 'none', False, None, False, True)),
    Case(22, 8, 8, 656, 16, 2304, 1, 1, 1, 0, 0, 0, False, 0,
         ('conv_split_kernel<2, 3, 1>', 'z', False, None, False, False)),
    Case(257, 8, 8, 656, 16, 192, 1, 1, 1, 0, 0, 0, False, 0,
         ('conv_split_kernel<2, 3, 1>', 'z', True, None, False, False)),
    Case(2, 128, 128, 16, 0, 15, 3, 2, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<2, 2, 1, 2>', 'none', False, (128, False), False, False)),
    Case(2, 128, 128, 16, 0, 15, 3, 2, 1, 1, 0, 0, True, 0,
         ('conv_split_rr_kernel<2, 2, 1, 2>', 'none', False, (128, False), False, True)),
    Case(5, 128, 128, 80, 16, 15, 3, 2, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<2, 2, 1, 2>', 'tail', False, (128, False), False, False)),
    Case(1, 128, 128, 32, 16, 15, 3, 2, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<2, 2, 1, 2>', 'z', False, (128, False), False, False)),
    Case(17, 16, 16, 64, 16, 192, 3, 2, 0, 0, 0, 0, False, 0,
         ('conv_split_rr_kernel<2, 2, 3, 0>', 'z', False, (16, False), False, False)),
    Case(2, 16, 16, 64, 16, 384, 3, 2, 0, 0, 0, 0, True, 0,
         ('conv_split_rr_kernel<2, 2, 3, 0>', 'z', False, (16, False), False, True)),
    Case(3, 32, 32, 112, 16, 192, 3, 2, 0, 0, 0, 0, False, 0,
         ('conv_split_rr_kernel<2, 2, 3, 0>', 'z', False, (32, False), False, False)),
    Case(2, 32, 32, 32, 16, 192, 3, 2, 0, 0, 0, 0, True, 0,
         ('conv_split_rr_kernel<2, 2, 3, 0>', 'z', False, (32, False), False, True)),
    Case(1, 64, 64, 96, 16, 192, 3, 2, 0, 0, 0, 0, False, 0,
         ('conv_split_rr_kernel<2, 2, 3, 0>', 'z', False, (64, False), False, False)),
    Case(22, 8, 8, 64, 16, 576, 3, 2, 0, 0, 0, 0, False, 0,
         ('conv_split_rr_kernel<2, 2, 3, 0>', 'z', False, (8, True), False, False)),
    Case(2, 8, 8, 336, 16, 384, 3, 2, 0, 0, 0, 0, True, 0,
         ('conv_split_rr_kernel<2, 2, 3, 0>', 'z', False, (8, True), False, True)),
    Case(65, 8, 8, 64, 16, 192, 3, 2, 0, 0, 0, 0, False, 0,
         ('conv_split_rr_kernel<2, 2, 3, 0>', 'z', True, (8, True), False, False)),
    Case(3, 8, 8, 336, 16, 384, 3, 2, 0, 0, 0, 0, True, 0,
         ('conv_split_rr_kernel<2, 2, 3, 0>', 'z', True, (8, True), False, True)),
    Case(17, 16, 16, 64, 16, 192, 3, 2, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<2, 2, 3, 2>', 'z', False, (16, False), False, False)),
    Case(2, 16, 16, 64, 16, 384, 3, 2, 1, 1, 0, 0, True, 0,
         ('conv_split_rr_kernel<2, 2, 3, 2>', 'z', False, (16, False), False, True)),
    Case(11, 16, 16, 112, 16, 192, 3, 2, 1, 1, 0, 80, False, 0,
         ('conv_split_rr_kernel<2, 2, 3, 2>', 'z', False, (16, False), True, False)),
    Case(2, 16, 16, 64, 16, 384, 3, 2, 1, 1, 0, 80, True, 0,
         ('conv_split_rr_kernel<2, 2, 3, 2>', 'z', False, (16, False), True, True)),
    Case(3, 32, 32, 112, 16, 192, 3, 2, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<2, 2, 3, 2>', 'z', False, (32, False), False, False)),
    Case(3, 32, 32, 112, 16, 192, 3, 2, 1, 1, 0, 80, False, 0,
         ('conv_split_rr_kernel<2, 2, 3, 2>', 'z', False, (32, False), True, False)),
    Case(2, 32, 32, 32, 16, 192, 3, 2, 1, 1, 0, 80, True, 0,
         ('conv_split_rr_kernel<2, 2, 3, 2>', 'z', False, (32, False), True, True)),
    Case(1, 64, 64, 96, 16, 192, 3, 2, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<2, 2, 3, 2>', 'z', False, (64, False), False, False)),
    Case(1, 64, 64, 96, 16, 192, 3, 2, 1, 1, 0, 80, False, 0,
         ('conv_split_rr_kernel<2, 2, 3, 2>', 'z', False, (64, False), True, False)),
    Case(22, 8, 8, 64, 16, 576, 3, 2, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<2, 2, 3, 2>', 'z', False, (8, True), False, False)),
    Case(2, 8, 8, 336, 16, 384, 3, 2, 1, 1, 0, 0, True, 0,
         ('conv_split_rr_kernel<2, 2, 3, 2>', 'z', False, (8, True), False, True)),
    Case(65, 8, 8, 64, 16, 192, 3, 2, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<2, 2, 3, 2>', 'z', True, (8, True), False, False)),
    Case(3, 8, 8, 336, 16, 384, 3, 2, 1, 1, 0, 0, True, 0,
         ('conv_split_rr_kernel<2, 2, 3, 2>', 'z', True, (8, True), False, True)),
    Case(8, 128, 128, 16, 0, 15, 3, 2, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<2, 4, 1, 2>', 'none', False, (128, False), False, False)),
    Case(3, 128, 128, 16, 0, 15, 3, 1, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 1, 2>', 'none', False, (128, False), False, False)),
    Case(5, 128, 128, 80, 16, 15, 3, 1, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 1, 2>', 'tail', False, (128, False), False, False)),
    Case(1, 128, 128, 16, 16, 15, 3, 1, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 1, 2>', 'z', False, (128, False), False, False)),
    Case(2, 128, 128, 96, 16, 15, 3, 1, 1, 1, 0, 0, True, 0,
         ('conv_split_rr_kernel<3, 2, 1, 2>', 'z', False, (128, False), False, True)),
    Case(3, 128, 128, 16, 0, 192, 3, 1, 0, 0, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 0>', 'none', False, (128, False), False, False)),
    Case(2, 128, 128, 16, 0, 192, 3, 1, 0, 0, 0, 0, True, 0,
         ('conv_split_rr_kernel<3, 2, 3, 0>', 'none', False, (128, False), False, True)),
    Case(11, 32, 32, 16, 0, 576, 3, 1, 0, 0, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 0>', 'none', False, (32, False), False, False)),
    Case(9, 64, 64, 16, 0, 192, 3, 1, 0, 0, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 0>', 'none', False, (64, False), False, False)),
    Case(5, 128, 128, 80, 16, 192, 3, 1, 0, 0, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 0>', 'tail', False, (128, False), False, False)),
    Case(65, 32, 32, 80, 16, 192, 3, 1, 0, 0, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 0>', 'tail', False, (32, False), False, False)),
    Case(17, 64, 64, 80, 16, 192, 3, 1, 0, 0, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 0>', 'tail', False, (64, False), False, False)),
    Case(1, 128, 128, 16, 16, 192, 3, 1, 0, 0, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 0>', 'z', False, (128, False), False, False)),
    Case(11, 16, 16, 112, 16, 192, 3, 1, 0, 0, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 0>', 'z', False, (16, False), False, False)),
    Case(2, 16, 16, 160, 16, 192, 3, 1, 0, 0, 0, 0, True, 0,
         ('conv_split_rr_kernel<3, 2, 3, 0>', 'z', False, (16, False), False, True)),
    Case(11, 32, 32, 16, 16, 192, 3, 1, 0, 0, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 0>', 'z', False, (32, False), False, False)),
    Case(2, 32, 32, 32, 16, 192, 3, 1, 0, 0, 0, 0, True, 0,
         ('conv_split_rr_kernel<3, 2, 3, 0>', 'z', False, (32, False), False, True)),
    Case(3, 64, 64, 16, 16, 192, 3, 1, 0, 0, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 0>', 'z', False, (64, False), False, False)),
    Case(2, 64, 64, 64, 16, 192, 3, 1, 0, 0, 0, 0, True, 0,
         ('conv_split_rr_kernel<3, 2, 3, 0>', 'z', False, (64, False), False, True)),
    Case(22, 8, 8, 112, 16, 384, 3, 1, 0, 0, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 0>', 'z', False, (8, True), False, False)),
    Case(2, 8, 8, 224, 16, 576, 3, 1, 0, 0, 0, 0, True, 0,
         ('conv_split_rr_kernel<3, 2, 3, 0>', 'z', False, (8, True), False, True)),
    Case(29, 8, 8, 48, 16, 576, 3, 1, 0, 0, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 0>', 'z', True, (8, True), False, False)),
    Case(3, 8, 8, 224, 16, 576, 3, 1, 0, 0, 0, 0, True, 0,
         ('conv_split_rr_kernel<3, 2, 3, 0>', 'z', True, (8, True), False, True)),
    Case(3, 128, 128, 16, 0, 192, 3, 1, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 2>', 'none', False, (128, False), False, False)),
    Case(2, 128, 128, 16, 0, 192, 3, 1, 1, 1, 0, 0, True, 0,
         ('conv_split_rr_kernel<3, 2, 3, 2>', 'none', False, (128, False), False, True)),
    Case(33, 32, 32, 16, 0, 192, 3, 1, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 2>', 'none', False, (32, False), False, False)),
    Case(9, 64, 64, 16, 0, 192, 3, 1, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 2>', 'none', False, (64, False), False, False)),
    Case(5, 128, 128, 80, 16, 192, 3, 1, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 2>', 'tail', False, (128, False), False, False)),
    Case(65, 32, 32, 80, 16, 192, 3, 1, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 2>', 'tail', False, (32, False), False, False)),
    Case(17, 64, 64, 80, 16, 192, 3, 1, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 2>', 'tail', False, (64, False), False, False)),
    Case(1, 128, 128, 16, 16, 192, 3, 1, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 2>', 'z', False, (128, False), False, False)),
    Case(11, 16, 16, 112, 16, 192, 3, 1, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 2>', 'z', False, (16, False), False, False)),
    Case(2, 16, 16, 160, 16, 192, 3, 1, 1, 1, 0, 0, True, 0,
         ('conv_split_rr_kernel<3, 2, 3, 2>', 'z', False, (16, False), False, True)),
    Case(11, 32, 32, 16, 16, 192, 3, 1, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 2>', 'z', False, (32, False), False, False)),
    Case(2, 32, 32, 32, 16, 192, 3, 1, 1, 1, 0, 0, True, 0,
         ('conv_split_rr_kernel<3, 2, 3, 2>', 'z', False, (32, False), False, True)),
    Case(3, 64, 64, 16, 16, 192, 3, 1, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 2>', 'z', False, (64, False), False, False)),
    Case(2, 64, 64, 64, 16, 192, 3, 1, 1, 1, 0, 0, True, 0,
         ('conv_split_rr_kernel<3, 2, 3, 2>', 'z', False, (64, False), False, True)),
    Case(22, 8, 8, 112, 16, 384, 3, 1, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 2>', 'z', False, (8, True), False, False)),
    Case(2, 8, 8, 224, 16, 576, 3, 1, 1, 1, 0, 0, True, 0,
         ('conv_split_rr_kernel<3, 2, 3, 2>', 'z', False, (8, True), False, True)),
    Case(29, 8, 8, 48, 16, 576, 3, 1, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 2>', 'z', True, (8, True), False, False)),
    Case(3, 8, 8, 224, 16, 576, 3, 1, 1, 1, 0, 0, True, 0,
         ('conv_split_rr_kernel<3, 2, 3, 2>', 'z', True, (8, True), False, True)),
    Case(8, 128, 128, 16, 0, 15, 3, 1, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 4, 1, 2>', 'none', False, (128, False), False, False)),
    Case(8, 128, 128, 16, 0, 192, 3, 1, 0, 0, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 4, 3, 0>', 'none', False, (128, False), False, False)),
    Case(32, 64, 64, 16, 0, 192, 3, 1, 0, 0, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 4, 3, 0>', 'none', False, (64, False), False, False)),
    Case(8, 128, 128, 16, 0, 192, 3, 1, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 4, 3, 2>', 'none', False, (128, False), False, False)),
    Case(32, 64, 64, 16, 0, 192, 3, 1, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 4, 3, 2>', 'none', False, (64, False), False, False)),
    Case(1, 32, 32, 16, 0, 192, 1, 2, 0, 0, 0, 0, False, 1,
         ('conv_splitn_kernel<2, 1, 3, 0>', 'none', False, None, False, False)),
    Case(2, 32, 32, 16, 0, 192, 1, 2, 0, 0, 0, 0, True, 1,
         ('conv_splitn_kernel<2, 1, 3, 0>', 'none', False, None, False, True)),
    Case(1, 8, 8, 176, 16, 192, 1, 2, 0, 0, 0, 0, False, 1,
         ('conv_splitn_kernel<2, 1, 3, 0>', 'z', False, None, False, False)),
    Case(2, 8, 8, 176, 16, 192, 1, 2, 0, 0, 0, 0, True, 1,
         ('conv_splitn_kernel<2, 1, 3, 0>', 'z', False, None, False, True)),
    Case(1, 32, 32, 16, 0, 192, 1, 2, 1, 0, 0, 0, False, 0,
         ('conv_splitn_kernel<2, 1, 3, 1>', 'none', False, None, False, False)),
    Case(2, 16, 16, 16, 0, 192, 1, 2, 1, 0, 0, 0, True, 0,
         ('conv_splitn_kernel<2, 1, 3, 1>', 'none', False, None, False, True)),
    Case(1, 8, 8, 176, 16, 192, 1, 2, 1, 0, 0, 0, False, 0,
         ('conv_splitn_kernel<2, 1, 3, 1>', 'z', False, None, False, False)),
    Case(2, 8, 8, 176, 16, 192, 1, 2, 1, 0, 0, 0, True, 0,
         ('conv_splitn_kernel<2, 1, 3, 1>', 'z', False, None, False, True)),
    Case(1, 8, 8, 16, 16, 192, 3, 2, 1, 1, 0, 0, False, 0,
         ('conv_splitn_kernel<2, 1, 3, 2>', 'z', False, None, False, False)),
    Case(33, 32, 32, 16, 0, 192, 1, 2, 0, 0, 0, 0, False, 1,
         ('conv_splitn_kernel<2, 2, 3, 0>', 'none', False, None, False, False)),
    Case(11, 32, 32, 16, 0, 576, 1, 2, 1, 0, 0, 0, False, 0,
         ('conv_splitn_kernel<2, 2, 3, 1>', 'none', False, None, False, False)),
    Case(2, 32, 32, 16, 0, 768, 1, 2, 1, 0, 0, 0, True, 0,
         ('conv_splitn_kernel<2, 2, 3, 1>', 'none', False, None, False, True)),
    Case(22, 8, 8, 656, 16, 2304, 1, 2, 1, 0, 0, 0, False, 0,
         ('conv_splitn_kernel<2, 2, 3, 1>', 'z', False, None, False, False)),
    Case(257, 8, 8, 656, 16, 192, 1, 2, 1, 0, 0, 0, False, 0,
         ('conv_splitn_kernel<2, 2, 3, 1>', 'z', True, None, False, False)),
    Case(11, 32, 32, 352, 16, 576, 3, 2, 0, 0, 0, 0, False, 0,
         ('conv_wide_kernel<0, 3, false>', 'cut', False, (32, False), False, False)),
    Case(32, 32, 32, 16, 0, 384, 3, 2, 0, 0, 0, 0, False, 0,
         ('conv_wide_kernel<0, 3, false>', 'none', False, (32, False), False, False)),
    Case(16, 64, 64, 16, 0, 192, 3, 2, 0, 0, 0, 0, False, 0,
         ('conv_wide_kernel<0, 3, false>', 'none', False, (64, False), False, False)),
    Case(2, 64, 64, 48, 16, 192, 3, 2, 0, 0, 0, 0, True, 0,
         ('conv_wide_kernel<0, 3, false>', 'none', False, (64, False), False, True)),
    Case(65, 32, 32, 80, 16, 192, 3, 2, 0, 0, 0, 0, False, 0,
         ('conv_wide_kernel<0, 3, false>', 'tail', False, (32, False), False, False)),
    Case(17, 64, 64, 80, 16, 192, 3, 2, 0, 0, 0, 0, False, 0,
         ('conv_wide_kernel<0, 3, false>', 'tail', False, (64, False), False, False)),
    Case(16, 16, 16, 240, 16, 384, 3, 2, 0, 0, 0, 0, False, 0,
         ('conv_wide_kernel<0, 3, false>', 'z', False, (16, False), False, False)),
    Case(2, 16, 16, 240, 16, 768, 3, 2, 0, 0, 0, 0, True, 0,
         ('conv_wide_kernel<0, 3, false>', 'z', False, (16, False), False, True)),
    Case(16, 32, 32, 112, 16, 192, 3, 2, 0, 0, 0, 0, False, 0,
         ('conv_wide_kernel<0, 3, false>', 'z', False, (32, False), False, False)),
    Case(2, 32, 32, 240, 16, 192, 3, 2, 0, 0, 0, 0, True, 0,
         ('conv_wide_kernel<0, 3, false>', 'z', False, (32, False), False, True)),
    Case(4, 64, 64, 112, 16, 192, 3, 2, 0, 0, 0, 0, False, 0,
         ('conv_wide_kernel<0, 3, false>', 'z', False, (64, False), False, False)),
    Case(4, 128, 128, 16, 0, 192, 3, 2, 0, 0, 0, 0, False, 0,
         ('conv_wide_kernel<0, 4, false>', 'none', False, (128, False), False, False)),
    Case(2, 128, 128, 16, 0, 192, 3, 2, 0, 0, 0, 0, True, 0,
         ('conv_wide_kernel<0, 4, false>', 'none', False, (128, False), False, True)),
    Case(5, 128, 128, 80, 16, 192, 3, 2, 0, 0, 0, 0, False, 0,
         ('conv_wide_kernel<0, 4, false>', 'tail', False, (128, False), False, False)),
    Case(1, 128, 128, 112, 16, 192, 3, 2, 0, 0, 0, 0, False, 0,
         ('conv_wide_kernel<0, 4, false>', 'z', False, (128, False), False, False)),
    Case(33, 32, 32, 352, 16, 192, 3, 2, 1, 1, 0, 0, False, 0,
         ('conv_wide_kernel<2, 3, false>', 'cut', False, (32, False), False, False)),
    Case(9, 64, 64, 352, 16, 192, 3, 2, 1, 1, 0, 0, False, 0,
         ('conv_wide_kernel<2, 3, false>', 'cut', False, (64, False), False, False)),
    Case(2, 64, 64, 352, 16, 192, 3, 2, 1, 1, 0, 0, True, 0,
         ('conv_wide_kernel<2, 3, false>', 'cut', False, (64, False), False, True)),
    Case(32, 32, 32, 16, 0, 384, 3, 2, 1, 1, 0, 0, False, 0,
         ('conv_wide_kernel<2, 3, false>', 'none', False, (32, False), False, False)),
    Case(16, 64, 64, 16, 0, 192, 3, 2, 1, 1, 0, 0, False, 0,
         ('conv_wide_kernel<2, 3, false>', 'none', False, (64, False), False, False)),
    Case(2, 64, 64, 48, 16, 192, 3, 2, 1, 1, 0, 0, True, 0,
         ('conv_wide_kernel<2, 3, false>', 'none', False, (64, False), False, True)),
    Case(17, 64, 64, 80, 16, 192, 3, 2, 1, 1, 0, 0, False, 0,
         ('conv_wide_kernel<2, 3, false>', 'tail', False, (64, False), False, False)),
    Case(16, 16, 16, 240, 16, 384, 3, 2, 1, 1, 0, 0, False, 0,
         ('conv_wide_kernel<2, 3, false>', 'z', False, (16, False), False, False)),
    Case(8, 32, 32, 112, 16, 384, 3, 2, 1, 1, 0, 0, False, 0,
         ('conv_wide_kernel<2, 3, false>', 'z', False, (32, False), False, False)),
    Case(2, 32, 32, 112, 16, 384, 3, 2, 1, 1, 0, 0, True, 0,
         ('conv_wide_kernel<2, 3, false>', 'z', False, (32, False), False, True)),
    Case(4, 64, 64, 112, 16, 192, 3, 2, 1, 1, 0, 0, False, 0,
         ('conv_wide_kernel<2, 3, false>', 'z', False, (64, False), False, False)),
    Case(33, 32, 32, 352, 16, 192, 3, 2, 1, 1, 0, 80, False, 0,
         ('conv_wide_kernel<2, 3, true>', 'cut', False, (32, False), True, False)),
    Case(32, 32, 32, 16, 0, 384, 3, 2, 1, 1, 0, 80, False, 0,
         ('conv_wide_kernel<2, 3, true>', 'none', False, (32, False), True, False)),
    Case(16, 64, 64, 16, 0, 192, 3, 2, 1, 1, 0, 80, False, 0,
         ('conv_wide_kernel<2, 3, true>', 'none', False, (64, False), True, False)),
    Case(2, 64, 64, 48, 16, 192, 3, 2, 1, 1, 0, 80, True, 0,
         ('conv_wide_kernel<2, 3, true>', 'none', False, (64, False), True, True)),
    Case(65, 32, 32, 80, 16, 192, 3, 2, 1, 1, 0, 80, False, 0,
         ('conv_wide_kernel<2, 3, true>', 'tail', False, (32, False), True, False)),
    Case(17, 64, 64, 80, 16, 192, 3, 2, 1, 1, 0, 80, False, 0,
         ('conv_wide_kernel<2, 3, true>', 'tail', False, (64, False), True, False)),
    Case(16, 16, 16, 240, 16, 384, 3, 2, 1, 1, 0, 80, False, 0,
         ('conv_wide_kernel<2, 3, true>', 'z', False, (16, False), True, False)),
    Case(2, 16, 16, 240, 16, 768, 3, 2, 1, 1, 0, 80, True, 0,
         ('conv_wide_kernel<2, 3, true>', 'z', False, (16, False), True, True)),
    Case(16, 32, 32, 112, 16, 192, 3, 2, 1, 1, 0, 80, False, 0,
         ('conv_wide_kernel<2, 3, true>', 'z', False, (32, False), True, False)),
    Case(2, 32, 32, 240, 16, 192, 3, 2, 1, 1, 0, 80, True, 0,
         ('conv_wide_kernel<2, 3, true>', 'z', False, (32, False), True, True)),
    Case(4, 64, 64, 112, 16, 192, 3, 2, 1, 1, 0, 80, False, 0,
         ('conv_wide_kernel<2, 3, true>', 'z', False, (64, False), True, False)),
    Case(4, 128, 128, 16, 0, 192, 3, 2, 1, 1, 0, 0, False, 0,
         ('conv_wide_kernel<2, 4, false>', 'none', False, (128, False), False, False)),
    Case(2, 128, 128, 16, 0, 192, 3, 2, 1, 1, 0, 0, True, 0,
         ('conv_wide_kernel<2, 4, false>', 'none', False, (128, False), False, True)),
    Case(5, 128, 128, 80, 16, 192, 3, 2, 1, 1, 0, 0, False, 0,
         ('conv_wide_kernel<2, 4, false>', 'tail', False, (128, False), False, False)),
    Case(1, 128, 128, 112, 16, 192, 3, 2, 1, 1, 0, 0, False, 0,
         ('conv_wide_kernel<2, 4, false>', 'z', False, (128, False), False, False)),
    Case(4, 128, 128, 16, 0, 192, 3, 2, 1, 1, 0, 80, False, 0,
         ('conv_wide_kernel<2, 4, true>', 'none', False, (128, False), True, False)),
    Case(2, 128, 128, 16, 0, 192, 3, 2, 1, 1, 0, 80, True, 0,
         ('conv_wide_kernel<2, 4, true>', 'none', False, (128, False), True, True)),
    Case(5, 128, 128, 80, 16, 192, 3, 2, 1, 1, 0, 80, False, 0,
         ('conv_wide_kernel<2, 4, true>', 'tail', False, (128, False), True, False)),
    Case(1, 128, 128, 112, 16, 192, 3, 2, 1, 1, 0, 80, False, 0,
         ('conv_wide_kernel<2, 4, true>', 'z', False, (128, False), True, False)),
    Case(257, 4, 4, 80, 16, 15, 3, 1, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 1, 2>', 'z', True, (4, True), False, False)),
    Case(129, 8, 8, 32, 16, 192, 3, 1, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<3, 2, 3, 2>', 'z', True, (8, True), False, False)),
    Case(257, 4, 4, 64, 16, 15, 3, 2, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<2, 2, 1, 2>', 'z', True, (4, True), False, False)),
    Case(129, 8, 8, 32, 16, 192, 3, 2, 1, 1, 0, 0, False, 0,
         ('conv_split_rr_kernel<2, 2, 3, 2>', 'z', True, (8, True), False, False)),
]

def case_id(c):
    kernel, kind, partial, rows, x2, inv = c.cls
    name = kernel.replace("conv_", "").replace("_kernel", "").replace(" ", "")
    return "-".join([name, kind] + ["partial"] * partial + ([f"w{rows[0]}" + "span" * rows[1]] if rows else []) + ["x2"] * x2 +
                    ["inv"] * inv + [f"b{c.B}"])


# ---- the older parity tests that name a kernel path ---------------------------------------------------------------------
# How to read one parametrize tuple of each of them: -> (B, H, W, C0, C1, Co, K, splits, x2 channels, on-load coefficients,
# activation), and the arithmetics the test runs under (its fixture).  The launch meant is the test's first one.
NAMED_TESTS = {
    ("test_gpu_ops", "test_conv3x3_row_reuse_shapes"):
        (lambda B, H, W, C0, C1, Co, splits: (B, H, W, C0, C1, Co, 3, splits, 0, 1, SILU), (BF16, F16)),
    ("test_gpu_ops", "test_conv3x3_k_split_tail"):
        (lambda B, H, W, C0, C1, Co: (B, H, W, C0, C1, Co, 3, 0, 0, 1, SILU), (BF16, F16)),
    ("test_gpu_ops", "test_conv_split_k_is_deterministic_and_matches_unsplit"):
        (lambda B, H, W, C0, C1, Co, K, splits: (B, H, W, C0, C1, Co, K, splits, 0, 1, SILU), (F32, BF16, F16)),
    ("test_gpu_ops", "test_conv3x3_with_fused_1x1_operand"):
        (lambda B, H, W, C, Co, C2a, C2b, splits: (B, H, W, C, 0, Co, 3, splits, C2a + C2b, 1, SILU), (F16,)),
    ("test_gpu_ops", "test_conv_wide_kernel_against_torch_and_the_row_reuse_kernel"):
        (lambda B, H, W, C0, C1, Co, mode, what: (B, H, W, C0, C1, Co, 3, 0, 0) + ((1, SILU) if mode == "gn" else (0, NONE)), (F16,)),
    ("test_gpu_nonfinite", "test_conv_nonfinite_footprint"):
        (lambda B, H, W, C0, C1, Co, K, arith, splits, knames, nsplit, ws, what: (B, H, W, C0, C1, Co, K, splits, 0, 1, SILU, arith),
         None),
}
Named = namedtuple("Named", "test B H W C0 C1 Co K arith coef act splits x2 cls")


def named_launches(module, test):
    """The launches a test's parametrize list stands for today (read from the test module itself): Named tuples without class."""
    import importlib
    read, ariths = NAMED_TESTS[(module, test)]
    marks = [m for m in getattr(importlib.import_module(module), test).pytestmark if m.name == "parametrize"]
    assert len(marks) == 1, (module, test)
    for params in marks[0].args[1]:
        v = read(*params)
        for arith in ((v[11],) if ariths is None else ariths):
            B, H, W, C0, C1, Co, K, splits, x2, coef, act = v[:11]
            yield Named(test, B, H, W, C0, C1, Co, K, arith, coef, act, splits, x2, None)


def named_class(test, B, H, W, C0, C1, Co, K, arith, coef, act, splits, x2):
    """The class ``NAMED`` states for one launch of an older test (KeyError: the test has a case the table does not know)."""
    key = Named(test, B, H, W, C0, C1, Co, K, arith, coef, act, splits, x2, None)
    for n in NAMED:
        if n._replace(cls=None) == key:
            return n.cls
    raise KeyError(key)


# The class every launch of those tests reaches today.  tests/test_conv_ledger_host.py fails, naming the test, when the planner
# moves one of them; the GPU tests assert the kernel of their own entry.
NAMED = [
    Named('test_conv3x3_row_reuse_shapes', 3, 8, 8, 32, 16, 192, 3, 1, 1, 1, 0, 0,
          ('conv_split_kernel<1, 3, 2>', 'z', False, None, False, False)),
    Named('test_conv3x3_row_reuse_shapes', 3, 8, 8, 32, 16, 192, 3, 2, 1, 1, 0, 0,
          ('conv_splitn_kernel<2, 1, 3, 2>', 'z', False, None, False, False)),
    Named('test_conv3x3_row_reuse_shapes', 3, 8, 8, 32, 16, 192, 3, 1, 1, 1, 3, 0,
          ('conv_split_kernel<1, 3, 2>', 'z', False, None, False, False)),
    Named('test_conv3x3_row_reuse_shapes', 3, 8, 8, 32, 16, 192, 3, 2, 1, 1, 3, 0,
          ('conv_splitn_kernel<2, 1, 3, 2>', 'z', False, None, False, False)),
    Named('test_conv3x3_row_reuse_shapes', 2, 16, 16, 48, 0, 192, 3, 1, 1, 1, 2, 0,
          ('conv_split_kernel<1, 3, 2>', 'z', False, None, False, False)),
    Named('test_conv3x3_row_reuse_shapes', 2, 16, 16, 48, 0, 192, 3, 2, 1, 1, 2, 0,
          ('conv_splitn_kernel<2, 1, 3, 2>', 'z', False, None, False, False)),
    Named('test_conv3x3_row_reuse_shapes', 2, 32, 32, 16, 32, 64, 3, 1, 1, 1, 0, 0,
          ('conv_split_kernel<1, 1, 2>', 'z', False, None, False, False)),
    Named('test_conv3x3_row_reuse_shapes', 2, 32, 32, 16, 32, 64, 3, 2, 1, 1, 0, 0,
          ('conv_splitn_kernel<2, 1, 1, 2>', 'z', False, None, False, False)),
    Named('test_conv3x3_row_reuse_shapes', 1, 64, 64, 16, 0, 128, 3, 1, 1, 1, 0, 0,
          ('conv_split_kernel<1, 2, 2>', 'none', False, None, False, False)),
    Named('test_conv3x3_row_reuse_shapes', 1, 64, 64, 16, 0, 128, 3, 2, 1, 1, 0, 0,
          ('conv_splitn_kernel<2, 1, 2, 2>', 'none', False, None, False, False)),
    Named('test_conv3x3_row_reuse_shapes', 1, 128, 128, 16, 16, 192, 3, 1, 1, 1, 0, 0,
          ('conv_split_rr_kernel<3, 2, 3, 2>', 'z', False, (128, False), False, False)),
    Named('test_conv3x3_row_reuse_shapes', 1, 128, 128, 16, 16, 192, 3, 2, 1, 1, 0, 0,
          ('conv_splitn_kernel<2, 1, 3, 2>', 'none', False, None, False, False)),
    Named('test_conv3x3_row_reuse_shapes', 1, 4, 4, 16, 0, 192, 3, 1, 1, 1, 0, 0,
          ('conv_split_kernel<1, 3, 2>', 'none', True, None, False, False)),
    Named('test_conv3x3_row_reuse_shapes', 1, 4, 4, 16, 0, 192, 3, 2, 1, 1, 0, 0,
          ('conv_splitn_kernel<2, 1, 3, 2>', 'none', True, None, False, False)),
    Named('test_conv3x3_row_reuse_shapes', 8, 128, 128, 16, 16, 64, 3, 1, 1, 1, 0, 0,
          ('conv_split_rr_kernel<3, 4, 1, 2>', 'none', False, (128, False), False, False)),
    Named('test_conv3x3_row_reuse_shapes', 8, 128, 128, 16, 16, 64, 3, 2, 1, 1, 0, 0,
          ('conv_split_rr_kernel<2, 4, 1, 2>', 'none', False, (128, False), False, False)),
    Named('test_conv3x3_k_split_tail', 9, 64, 64, 64, 32, 384, 3, 1, 1, 1, 0, 0,
          ('conv_split_rr_kernel<3, 2, 3, 2>', 'tail', False, (64, False), False, False)),
    Named('test_conv3x3_k_split_tail', 9, 64, 64, 64, 32, 384, 3, 2, 1, 1, 0, 0,
          ('conv_wide_kernel<2, 3, false>', 'tail', False, (64, False), False, False)),
    Named('test_conv3x3_k_split_tail', 5, 128, 128, 96, 0, 192, 3, 1, 1, 1, 0, 0,
          ('conv_split_rr_kernel<3, 2, 3, 2>', 'tail', False, (128, False), False, False)),
    Named('test_conv3x3_k_split_tail', 5, 128, 128, 96, 0, 192, 3, 2, 1, 1, 0, 0,
          ('conv_wide_kernel<2, 4, false>', 'tail', False, (128, False), False, False)),
    Named('test_conv3x3_k_split_tail', 5, 128, 128, 48, 48, 128, 3, 1, 1, 1, 0, 0,
          ('conv_split_rr_kernel<3, 2, 2, 2>', 'tail', False, (128, False), False, False)),
    Named('test_conv3x3_k_split_tail', 5, 128, 128, 48, 48, 128, 3, 2, 1, 1, 0, 0,
          ('conv_split_rr_kernel<2, 2, 2, 2>', 'tail', False, (128, False), False, False)),
    Named('test_conv_split_k_is_deterministic_and_matches_unsplit', 2, 32, 32, 32, 16, 192, 3, 0, 1, 1, 2, 0,
          ('conv_igemm_kernel<1, 3, 2>', 'z', False, None, False, False)),
    Named('test_conv_split_k_is_deterministic_and_matches_unsplit', 2, 32, 32, 32, 16, 192, 3, 1, 1, 1, 2, 0,
          ('conv_split_kernel<1, 3, 2>', 'z', False, None, False, False)),
    Named('test_conv_split_k_is_deterministic_and_matches_unsplit', 2, 32, 32, 32, 16, 192, 3, 2, 1, 1, 2, 0,
          ('conv_splitn_kernel<2, 1, 3, 2>', 'z', False, None, False, False)),
    Named('test_conv_split_k_is_deterministic_and_matches_unsplit', 3, 8, 8, 64, 0, 192, 3, 0, 1, 1, 4, 0,
          ('conv_igemm_kernel<1, 3, 2>', 'z', False, None, False, False)),
    Named('test_conv_split_k_is_deterministic_and_matches_unsplit', 3, 8, 8, 64, 0, 192, 3, 1, 1, 1, 4, 0,
          ('conv_split_kernel<1, 3, 2>', 'z', False, None, False, False)),
    Named('test_conv_split_k_is_deterministic_and_matches_unsplit', 3, 8, 8, 64, 0, 192, 3, 2, 1, 1, 4, 0,
          ('conv_splitn_kernel<2, 1, 3, 2>', 'z', False, None, False, False)),
    Named('test_conv_split_k_is_deterministic_and_matches_unsplit', 2, 16, 16, 96, 32, 384, 1, 0, 1, 1, 3, 0,
          ('conv_igemm_kernel<1, 3, 2>', 'z', False, None, False, False)),
    Named('test_conv_split_k_is_deterministic_and_matches_unsplit', 2, 16, 16, 96, 32, 384, 1, 1, 1, 1, 3, 0,
          ('conv_split_kernel<1, 3, 2>', 'z', False, None, False, False)),
    Named('test_conv_split_k_is_deterministic_and_matches_unsplit', 2, 16, 16, 96, 32, 384, 1, 2, 1, 1, 3, 0,
          ('conv_splitn_kernel<2, 1, 3, 2>', 'z', False, None, False, False)),
    Named('test_conv_split_k_is_deterministic_and_matches_unsplit', 9, 64, 64, 32, 0, 192, 3, 0, 1, 1, 0, 0,
          ('conv_igemm_kernel<2, 3, 2>', 'z', False, None, False, False)),
    Named('test_conv_split_k_is_deterministic_and_matches_unsplit', 9, 64, 64, 32, 0, 192, 3, 1, 1, 1, 0, 0,
          ('conv_split_rr_kernel<3, 2, 3, 2>', 'none', False, (64, False), False, False)),
    Named('test_conv_split_k_is_deterministic_and_matches_unsplit', 9, 64, 64, 32, 0, 192, 3, 2, 1, 1, 0, 0,
          ('conv_split_rr_kernel<2, 2, 3, 2>', 'none', False, (64, False), False, False)),
    Named('test_conv_split_k_is_deterministic_and_matches_unsplit', 5, 128, 128, 16, 16, 192, 3, 0, 1, 1, 0, 0,
          ('conv_igemm_kernel<2, 3, 2>', 'none', False, None, False, False)),
    Named('test_conv_split_k_is_deterministic_and_matches_unsplit', 5, 128, 128, 16, 16, 192, 3, 1, 1, 1, 0, 0,
          ('conv_split_rr_kernel<3, 2, 3, 2>', 'none', False, (128, False), False, False)),
    Named('test_conv_split_k_is_deterministic_and_matches_unsplit', 5, 128, 128, 16, 16, 192, 3, 2, 1, 1, 0, 0,
          ('conv_wide_kernel<2, 4, false>', 'none', False, (128, False), False, False)),
    Named('test_conv3x3_with_fused_1x1_operand', 9, 32, 32, 192, 0, 192, 3, 2, 1, 1, 0, 128,
          ('conv_split_rr_kernel<2, 2, 3, 2>', 'z', False, (32, False), True, False)),
    Named('test_conv3x3_with_fused_1x1_operand', 9, 32, 32, 64, 0, 192, 3, 2, 1, 1, 3, 48,
          ('conv_split_rr_kernel<2, 2, 3, 2>', 'z', False, (32, False), True, False)),
    Named('test_conv3x3_with_fused_1x1_operand', 9, 8, 8, 384, 0, 384, 3, 2, 1, 1, 0, 160,
          ('conv_split_rr_kernel<2, 2, 3, 2>', 'z', True, (8, True), True, False)),
    Named('test_conv3x3_with_fused_1x1_operand', 9, 16, 16, 192, 0, 384, 3, 2, 1, 1, 0, 128,
          ('conv_split_rr_kernel<2, 2, 3, 2>', 'z', False, (16, False), True, False)),
    Named('test_conv3x3_with_fused_1x1_operand', 5, 128, 128, 96, 0, 192, 3, 2, 1, 1, 0, 64,
          ('conv_wide_kernel<2, 4, true>', 'tail', False, (128, False), True, False)),
    Named('test_conv3x3_with_fused_1x1_operand', 9, 64, 64, 192, 0, 192, 3, 2, 1, 1, 0, 384,
          ('conv_wide_kernel<2, 3, true>', 'none', False, (64, False), True, False)),
    Named('test_conv3x3_with_fused_1x1_operand', 8, 64, 64, 64, 0, 128, 3, 2, 1, 1, 0, 16,
          ('conv_split_rr_kernel<2, 2, 2, 2>', 'none', False, (64, False), True, False)),
    Named('test_conv_wide_kernel_against_torch_and_the_row_reuse_kernel', 4, 128, 128, 32, 16, 192, 3, 2, 1, 1, 0, 0,
          ('conv_wide_kernel<2, 4, false>', 'none', False, (128, False), False, False)),
    Named('test_conv_wide_kernel_against_torch_and_the_row_reuse_kernel', 5, 128, 128, 192, 0, 192, 3, 2, 1, 1, 0, 0,
          ('conv_wide_kernel<2, 4, false>', 'tail', False, (128, False), False, False)),
    Named('test_conv_wide_kernel_against_torch_and_the_row_reuse_kernel', 5, 128, 128, 48, 0, 192, 3, 2, 0, 0, 0, 0,
          ('conv_wide_kernel<0, 4, false>', 'none', False, (128, False), False, False)),
    Named('test_conv_wide_kernel_against_torch_and_the_row_reuse_kernel', 9, 64, 64, 96, 0, 384, 3, 2, 1, 1, 0, 0,
          ('conv_wide_kernel<2, 3, false>', 'tail', False, (64, False), False, False)),
    Named('test_conv_wide_kernel_against_torch_and_the_row_reuse_kernel', 9, 64, 64, 64, 0, 192, 3, 2, 0, 0, 0, 0,
          ('conv_wide_kernel<0, 3, false>', 'none', False, (64, False), False, False)),
    Named('test_conv_wide_kernel_against_torch_and_the_row_reuse_kernel', 9, 64, 64, 128, 64, 192, 3, 2, 1, 1, 0, 0,
          ('conv_wide_kernel<2, 3, false>', 'none', False, (64, False), False, False)),
    Named('test_conv_wide_kernel_against_torch_and_the_row_reuse_kernel', 9, 32, 32, 128, 64, 384, 3, 2, 1, 1, 0, 0,
          ('conv_wide_kernel<2, 3, false>', 'z', False, (32, False), False, False)),
    Named('test_conv_wide_kernel_against_torch_and_the_row_reuse_kernel', 64, 16, 16, 64, 0, 384, 3, 2, 1, 1, 0, 0,
          ('conv_wide_kernel<2, 3, false>', 'none', False, (16, False), False, False)),
    Named('test_conv_nonfinite_footprint', 2, 6, 7, 32, 16, 48, 3, 0, 1, 1, 0, 0,
          ('conv_igemm_kernel<1, 1, 2>', 'z', True, None, False, False)),
    Named('test_conv_nonfinite_footprint', 2, 64, 64, 32, 16, 64, 3, 0, 1, 1, 0, 0,
          ('conv_igemm_kernel<2, 1, 2>', 'z', False, None, False, False)),
    Named('test_conv_nonfinite_footprint', 3, 8, 8, 96, 32, 128, 1, 1, 1, 1, 0, 0,
          ('conv_split_kernel<1, 2, 2>', 'none', False, None, False, False)),
    Named('test_conv_nonfinite_footprint', 3, 8, 8, 96, 32, 128, 1, 2, 1, 1, 0, 0,
          ('conv_splitn_kernel<2, 1, 2, 2>', 'none', False, None, False, False)),
    Named('test_conv_nonfinite_footprint', 256, 8, 8, 32, 16, 192, 3, 2, 1, 1, 0, 0,
          ('conv_split_rr_kernel<2, 2, 3, 2>', 'z', False, (8, True), False, False)),
    Named('test_conv_nonfinite_footprint', 8, 128, 128, 16, 16, 64, 3, 2, 1, 1, 0, 0,
          ('conv_split_rr_kernel<2, 4, 1, 2>', 'none', False, (128, False), False, False)),
    Named('test_conv_nonfinite_footprint', 5, 128, 128, 96, 32, 128, 3, 2, 1, 1, 0, 0,
          ('conv_split_rr_kernel<2, 2, 2, 2>', 'tail', False, (128, False), False, False)),
    Named('test_conv_nonfinite_footprint', 4, 128, 128, 32, 16, 192, 3, 2, 1, 1, 0, 0,
          ('conv_wide_kernel<2, 4, false>', 'none', False, (128, False), False, False)),
    Named('test_conv_nonfinite_footprint', 5, 128, 128, 192, 0, 192, 3, 2, 1, 1, 0, 0,
          ('conv_wide_kernel<2, 4, false>', 'tail', False, (128, False), False, False)),
    Named('test_conv_nonfinite_footprint', 9, 32, 32, 128, 64, 384, 3, 2, 1, 1, 0, 0,
          ('conv_wide_kernel<2, 3, false>', 'z', False, (32, False), False, False)),
    Named('test_conv_nonfinite_footprint', 9, 64, 64, 256, 128, 192, 3, 2, 1, 1, 0, 0,
          ('conv_wide_kernel<2, 3, false>', 'cut', False, (64, False), False, False)),
    Named('test_conv_nonfinite_footprint', 3, 8, 8, 32, 16, 192, 3, 2, 1, 1, 3, 0,
          ('conv_splitn_kernel<2, 1, 3, 2>', 'z', False, None, False, False)),
]


# ---- the search that wrote CASES -------------------------------------------------------------------------------------

_CO = (15, 64, 128, 192, 384, 576, 768, 1152, 1728, 2304)
_BATCHES = tuple(range(1, 33)) + (33, 64, 65, 128, 129, 256, 257)


def _with_two_sources(c):
    """Move 16 channels into a second concat source (the planner sees C0 + C1 only), so that every case with more than one
    chunk also reads across a source boundary."""
    return c._replace(C0=c.C0 - 16, C1=16) if c.C1 == 0 and c.C0 >= 32 else c


def cheapest(want, seed, L):
    """The case with the fewest MACs whose class satisfies ``want``: the seed launch's image size, filter, arithmetic and
    on-load mode; batch, input and output channels shrunk (the fused operand to 80 channels: five chunks, so that no split count
    divides them).  Invariant cases keep two samples at least (one bound word per sample), and a fused operand must be one
    the plan accepts."""
    best = None
    for B in _BATCHES:
        if seed.invariant and B < 2:
            continue
        for Co in _CO:
            if Co > seed.Co:
                break
            for C in range(16, seed.C0 + seed.C1 + 1, 16):
                c = seed._replace(B=B, C0=C, C1=0, Co=Co, x2=min(seed.x2, 80))
                if best is not None and macs(c) >= macs(best):
                    break
                cls = case_class(c, L)
                if want(cls) and (not c.x2 or L.conv_plan(c.B, c.H, c.W, c.C0, 0, c.Co, c.K, c.arith, coef=bool(c.coef), act_in=c.act,
                                                          x2_ci=c.x2, invariant=c.invariant)["fused_1x1"]):
                    best = c._replace(cls=cls)
                    break
    return None if best is None else _with_two_sources(best)


def search():
    """One case per class of the product, then the row-reuse kernel at W = 4 and the W = 8 case of 129 images (a partial last
    tile, every tile spanning two images, z-splits) under both split arithmetics: neither is a shape of the network."""
    L = lib()
    seeds = {}
    for c in product_launches(L):
        cls = case_class(c, L)
        if cls not in seeds or macs(c) < macs(seeds[cls]):
            seeds[cls] = c
    out = []
    for cls in sorted(seeds, key=lambda k: (k[0].split("<")[0], str(k))):
        out.append(cheapest(lambda k: k == cls, seeds[cls], L) or seeds[cls]._replace(cls=cls))
    for arith in (BF16, F16):
        seed = Case(1, 4, 4, 192, 0, 192, 3, arith, 1, SILU, 0, 0, False, 0, None)
        out.append(cheapest(lambda k: k[0].startswith("conv_split_rr_kernel") and k[3] == (4, True), seed, L))
        c = Case(129, 8, 8, 32, 16, 192, 3, arith, 1, SILU, 0, 0, False, 0, None)
        out.append(c._replace(cls=case_class(c, L)))
    return out


def _fmt(c):
    return (f"    Case({c.B}, {c.H}, {c.W}, {c.C0}, {c.C1}, {c.Co}, {c.K}, {c.arith}, {c.coef}, {c.act}, {c.splits}, {c.x2}, "
            f"{c.invariant!s}, {c.bound},\n         {c.cls!r}),")


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("CASES = [")
    for c in search():
        print(_fmt(c))
    print("]\n\nNAMED = [")
    L = lib()
    for module, test in NAMED_TESTS:
        for n in named_launches(module, test):
            cls = plan_class(*n[1:8], n.arith, n.coef, n.act, n.splits, n.x2, False, L)
            print(f"    Named({n.test!r}, {', '.join(str(v) for v in n[1:13])},\n          {cls!r}),")
    print("]")
