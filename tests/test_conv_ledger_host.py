"""CPU tests of the convolution ledger (tests/conv_ledger.py): the planner is queried without a GPU (``lib.conv_plan``), so a
change of ``conv_tile_cfg_at`` that moves a shape to another kernel, split kind or tile geometry fails HERE, naming the parity
case that lost its kernel -- not months later in a whole-network golden.  The GPU side is tests/test_gpu_conv_ledger.py."""
import pytest

import conv_ledger as ledger

# Plan classes of the product that no entry of CASES runs, each with its reason.  Covering every class is a condition, so the
# list is empty and is asserted literally: any growth shows in a diff.
NOT_COVERED = []


@pytest.fixture(scope="module")
def L():
    return ledger.lib()


def test_every_case_plans_to_its_stated_class(L):
    moved = [(ledger.case_id(c), ledger.case_class(c, L)) for c in ledger.CASES if ledger.case_class(c, L) != c.cls]
    assert not moved, moved
    assert len({ledger.case_id(c) for c in ledger.CASES}) == len(ledger.CASES)
    for c in ledger.CASES:
        assert c.cls[1] in ledger.SPLIT_KINDS and (c.cls[3] is None) == (c.cls[0].split("<")[0] not in ledger.ROW_KERNELS)
        if c.x2:       # a fused operand the plan accepts, on the fp16 split only
            assert c.arith == ledger.F16
            assert L.conv_plan(c.B, c.H, c.W, c.C0, c.C1, c.Co, c.K, c.arith, coef=bool(c.coef), act_in=c.act, x2_ci=c.x2,
                               invariant=c.invariant, splits=c.splits)["fused_1x1"], ledger.case_id(c)
        assert not c.bound or c.arith == ledger.F16           # only the fp16 split scales its operand
        assert not c.invariant or c.B >= 2                    # one bound word per sample means something from two samples on


def test_every_class_the_network_launches_has_a_case(L):
    """FULL_SIZE_CONVS x B = 1..32 (invariant: 1, 2, 9, 32) x {own arithmetic, bf16x6}: classes of the product <= classes of
    CASES, nothing excluded."""
    assert NOT_COVERED == []
    product = ledger.product_classes(L)
    assert len(product) >= 100, len(product)          # the enumeration itself did not collapse
    missing = product - {c.cls for c in ledger.CASES} - set(NOT_COVERED)
    assert not missing, sorted(missing, key=str)


def test_the_older_tables_alone_do_not_cover_the_product(L):
    """The same subset check against the launches of the older parity tests only (NAMED): it fails, which is why the ledger
    exists.  With the on-load mode ignored they reach 21 of the 63 classes of the default-mode product."""
    product = {ledger.ignore_mode(k)[:5] for k in ledger.product_classes(L) if not k[5]}
    old = {ledger.ignore_mode(n.cls)[:5] for n in ledger.NAMED}
    print(f"older tables: {len(product & old)} of {len(product)} default-mode classes (on-load mode ignored)")
    assert len(product & old) < len(product) // 2


@pytest.mark.parametrize("module,test", sorted(ledger.NAMED_TESTS), ids=[t for _, t in sorted(ledger.NAMED_TESTS)])
def test_named_parity_cases_still_reach_their_kernel(L, module, test):
    """Every parametrized case of tests/test_gpu_ops.py and tests/test_gpu_nonfinite.py whose comment or id names a kernel path:
    the class of its launch is the one written in ``NAMED``, and the table knows every case the test has today."""
    launches = list(ledger.named_launches(module, test))
    assert launches
    for n in launches:
        want = ledger.named_class(*n[:13])              # KeyError: a case was added to the test but not to the table
        got = ledger.plan_class(*n[1:8], n.arith, n.coef, n.act, n.splits, n.x2, False, L)
        assert got == want, (f"{module}::{test}", n[1:13], got, want)
    table = [n for n in ledger.NAMED if n.test == test]
    assert len(table) == len(launches), (test, len(table), len(launches))     # no stale rows either


def _queries(L, a):
    """Every query entry point's answer for one ``ConvArgs``: (plan_query's code, its plan, {query: answer})."""
    import ctypes
    H = L.hip_lib(require_device=False)
    ref, plan, buf = ctypes.byref(a), L.ConvPlan(), ctypes.create_string_buffer(96)
    rc = H.evc_conv_plan_query(ref, ctypes.byref(plan))
    n = H.evc_conv_kernel_name(ref, buf, 96)
    return rc, plan, dict(name=buf.value.decode() if n >= 0 else n, splits=H.evc_conv_choose_splits(ref),
                          stats=H.evc_conv_stats_splits(ref), ws=H.evc_conv_workspace_bytes(ref),
                          fused=H.evc_conv_fused_1x1_supported(ref))


def test_single_answer_queries_agree_with_the_plan(L):
    """Every launch of the product and every ledger case: the five single-answer queries say what evc_conv_plan_query says,
    and the workspace is the one the plan's fields imply (tail slabs, else split-K slabs, else none)."""
    cases = list(ledger.product_launches(L)) + ledger.CASES
    assert len(cases) > 1000
    for c in cases:
        a = L.conv_query_args(c.B, c.H, c.W, c.C0, c.C1, c.Co, c.K, c.K, c.arith, coef=bool(c.coef), act_in=c.act,
                              splits=c.splits, x2_ci=c.x2, invariant=c.invariant)
        rc, p, q = _queries(L, a)
        assert rc == 0, c
        if p.tail_tiles:
            ws = p.tail_splits * p.tail_tiles * p.tile_m * c.Co * 4
        else:
            ws = p.splits * c.B * c.H * c.W * c.Co * 4 if p.splits > 1 else 0
        assert q == dict(name=p.kernel.decode(), splits=p.splits, stats=p.stats_runs, ws=ws, fused=p.fused_1x1), (c, q)


def test_refused_arguments_are_refused_by_every_query(L):
    """What the launch refuses no query describes: GroupNorm coefficients with ReLU on load (no such load mode), and a fused 1x1
    operand on a shape whose plan cannot carry it (1 x 8 x 8, 576 -> 576, f16x3: 64-pixel tiles).  The four queries with an
    error channel return the launch's code (EVC_EUNSUPPORTED), the two yes / no questions say 0."""
    relu = L.conv_query_args(1, 32, 32, 192, 0, 192, 3, 3, ledger.F16, coef=True, act_in=L.ACT_RELU)
    assert not L.conv_plan(1, 8, 8, 576, 0, 576, 3, ledger.F16)["fused_1x1"]
    fused = L.conv_query_args(1, 8, 8, 576, 0, 576, 3, 3, ledger.F16, x2_ci=576)
    for a in (relu, fused):
        rc, _, q = _queries(L, a)
        assert rc == -2 and q == dict(name=-2, splits=-2, stats=0, ws=-2, fused=0), (rc, q)


def test_the_promised_row_reuse_cases_are_in_the_ledger():
    """What test_conv3x3_row_reuse_shapes and test_conv_split_k_... describe and the planner no longer gives their shapes: the
    row-reuse kernel at every image width under both split arithmetics, a partial last tile with tiles spanning images at
    W = 8 and an odd batch >= 129, a z-split, and a genuine K-split tail per arithmetic."""
    for planes in (3, 2):                                 # bf16x6 / f16x3
        rr = [c for c in ledger.CASES if c.cls[0].startswith(f"conv_split_rr_kernel<{planes},")]
        assert {c.W for c in rr} >= {4, 8, 16, 32, 64, 128}, planes
        assert any(c.W == 8 and c.B >= 129 and c.B % 2 and c.cls[2] and c.cls[3] == (8, True) for c in rr), planes
        assert any(c.cls[1] == "z" for c in rr) and any(c.cls[1] == "tail" for c in rr), planes
