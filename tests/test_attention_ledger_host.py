"""CPU tests of the attention ledger (tests/attention_ledger.py): the planner is queried without a GPU
(``lib.attention_plan``), so a change of ``attention_plan`` / ``attention_plan_f16`` / ``attention_resolve`` or of one of their
constants that moves a shape to another kernel instance or across the key split fails HERE, naming the parity case that lost
its kernel.  The GPU side is tests/test_gpu_attention_ledger.py."""
import ctypes
import os

import pytest

import attention_ledger as ledger

# Plan classes of the product that no entry of CASES runs, each with its reason.  Covering every class is a condition, so the
# list is empty and is asserted literally: any growth shows in a diff.
NOT_COVERED = []

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "extreme-video-compression-with-prediction-using-pre-trainded-diffusion-models-_amd")


@pytest.fixture(scope="module")
def L():
    return ledger.lib()


def test_every_case_plans_to_its_stated_class(L):
    moved = [(ledger.case_id(c), ledger.case_class(c, L)) for c in ledger.CASES if ledger.case_class(c, L) != c.cls]
    assert not moved, moved
    assert len({ledger.case_id(c) for c in ledger.CASES}) == len(ledger.CASES)
    for c in ledger.CASES:
        p = ledger.case_plan(c, L)
        assert ledger.family(c.cls) in ledger.FAMILIES and c.ws in ledger.HAVE_WS
        assert set(c.options) <= set(ledger.DEFAULTS) and not (c.invariant and (c.options or c.ws != "auto"))
        assert not c.invariant or c.B >= 2                    # one triple of bound words per sample means something from two on
        assert c.cls[1] == bool(p["merge"]) and p["waves"] == ledger.waves_of(c.cls)
        assert ("f16" in c.cls[0]) <= bool(c.f16)             # the fp16-split kernels only with bound words


def test_every_class_the_network_launches_has_a_case(L):
    """SITES x B = 1..32 (invariant: 1, 2, 9, 32) x {bound words, none}: classes of the product <= classes of CASES, nothing
    excluded."""
    assert NOT_COVERED == []
    product = ledger.product_classes(L)
    assert len(product) >= 35, len(product)           # the enumeration itself did not collapse
    missing = product - {c.cls for c in ledger.CASES} - set(NOT_COVERED)
    assert not missing, sorted(missing, key=str)


def test_every_instantiation_is_run_or_listed_unreachable():
    """The kernel instances of csrc/attention.hip: 4 + 4 short-sequence ones, attention_kernel<D, 1|2|4> for five head widths,
    attention_f16_kernel<D, 1|2|4> and <D, 4, pre> for four."""
    f16_widths = [d for d in ledger.WIDTHS if d <= 192]
    want = {f"attention_short_kernel<{d}>" for d in f16_widths} | {f"attention_short_f16_kernel<{d}>" for d in f16_widths} | \
        {f"attention_kernel<{d},{w}>" for d in ledger.WIDTHS for w in (1, 2, 4)} | \
        {f"attention_f16_kernel<{d},{w}>" for d in f16_widths for w in (1, 2, 4)} | \
        {f"attention_f16_kernel<{d},4,pre>" for d in f16_widths}
    assert {c.cls[0] for c in ledger.CASES} == want
    assert all(len(reason) > 20 for _, reason in ledger.UNREACHABLE)
    assert not {name for name, _ in ledger.UNREACHABLE} & want


def _edges(c, p):
    ntiles = (c.N + 31) // 32
    qrows = 32 if p["short_seq"] else 32 * p["waves"]           # queries per workgroup
    e = set()
    if c.N <= 32 and (p["short_seq"] or p["waves"] == 1):
        e.add("one key tile")
    if c.N % 32 and ntiles > 1:
        e.add("ragged last key tile")
    if c.N % qrows and c.N > qrows:
        e.add("ragged last query block")
    if p["kparts"] >= 2 and ntiles - (p["kparts"] - 1) * p["tiles_per_part"] == 1 and c.N % 32:
        e.add("last key part a single ragged tile")
    if p["kparts"] >= 3:
        e.add("three key parts or more")
    return e


def test_the_edges_of_every_kernel_family_are_in_the_ledger(L):
    """Whatever the classes are, the cases of a family together show: one key tile (short-sequence and 1-wave kernels), a ragged
    last key tile behind full ones, a ragged last query block behind full ones, and where the family splits the keys an uneven
    split whose last part is one ragged tile (200 keys in 3 parts: 3, 3, 1 tiles) and a split in three parts or more; every head
    width the family instantiates."""
    common = {"one key tile", "ragged last key tile", "ragged last query block"}
    split = {"last key part a single ragged tile", "three key parts or more"}
    need = {"attention_short_kernel": (common, 4), "attention_short_f16_kernel": (common, 4),
            "attention_kernel": (common | split, 5), "attention_f16_kernel": (common | split, 4),
            "attention_f16_kernel,pre": ((common | split) - {"one key tile"}, 4)}       # the pre-pass starts at 512 keys
    for fam, (edges, widths) in need.items():
        cases = [c for c in ledger.CASES if ledger.family(c.cls) == fam]
        seen = set().union(*(_edges(c, ledger.case_plan(c, L)) for c in cases))
        assert seen >= edges, (fam, edges - seen)
        assert len({c.D for c in cases}) == widths, fam
    inv = [c for c in ledger.CASES if c.invariant and c.f16 and c.N == 200]        # the example above, in the receivers' mode
    assert inv and all((p["kparts"], p["tiles_per_part"]) == (3, 3) for p in (ledger.case_plan(c, L) for c in inv))


@pytest.mark.parametrize("module,test", sorted(ledger.NAMED_TESTS), ids=[t for _, t in sorted(ledger.NAMED_TESTS)])
def test_named_parity_cases_still_reach_their_kernel(L, module, test):
    """Every launch of the older attention parity tests: its class is the one written in ``NAMED``, and the table knows every
    case the test has today."""
    launches = list(ledger.named_launches(module, test))
    assert launches
    for n in launches:
        want = ledger.named_class(n)                    # KeyError: a case was added to the test but not to the table
        got = ledger.classify(ledger.plan(L, n.B, n.heads, n.N, n.D, n.f16, False, n.options, n.ws), False)
        assert got == want, (f"{module}::{test}", n[1:8], got, want)
    table = [n for n in ledger.NAMED if n.test == test]
    assert len(table) == len(launches), (test, len(table), len(launches))     # no stale rows either


def test_the_sites_are_the_calls_of_the_shipped_architectures():
    """SITES against the code: the line named holds the call, and the (heads, N, D) of the score networks are those of the
    default configuration's program."""
    import evc_amd  # noqa: F401
    from evc_amd import config, scorenet, unet_ddpm
    for s in ledger.SITES:
        name, line = s.where.split(":")
        with open(os.path.join(PKG, name)) as f:
            assert "attention(" in f.read().splitlines()[int(line) - 1], s.where
    d = scorenet.dims_from_config(config.default_config())
    size, got = d.image_size, set()
    res = [size // 2 ** i for i in range(len(d.ch_mult))]
    for lvl, mult in enumerate(d.ch_mult):
        if res[lvl] in d.attn_resolutions:
            C = d.ngf * mult
            got.add((1 if C < d.n_head_channels else C // d.n_head_channels, res[lvl] ** 2, min(C, d.n_head_channels)))
    assert {m["ch"] for m in scorenet.build_program(d) if m["kind"] == "attn"} == {h * D for h, _, D in got}
    for arch in ("unetmore", "unetmore-spade", "unetmorepseudo3d"):
        assert {(s.heads, s.N, s.D) for s in ledger.SITES if s.arch == arch} == got, arch
    assert {s.D for s in ledger.SITES if s.arch == "unet_ddpm"} == set(unet_ddpm.ATTENTION_WIDTHS)
    assert all(s.heads == 1 and s.N in ((size // 2) ** 2, (size // 8) ** 2) for s in ledger.SITES if s.arch == "unet_ddpm")


def test_workspace_queries_agree_with_the_plan(L):
    """Every launch of the product and every ledger case: evc_attention_workspace_bytes / evc_attention_invariant_workspace_bytes
    say what the plan's ``ws_bytes`` says, and that is the key-part buffers plus the K / V tile images, both as the plan states
    them: ``parts_bytes``, and one image of the fp16-split kernel's LDS layout per (sample, head, 32-key tile) from 128 keys on."""
    H = L.hip_lib(require_device=False)
    cases = list(ledger.product_launches()) + ledger.CASES
    assert len(cases) > 500
    for c in cases:
        p = ledger.case_plan(c, L)
        size = (H.evc_attention_invariant_workspace_bytes if c.invariant else H.evc_attention_workspace_bytes)
        assert size(c.B, c.heads, c.N, c.D) == p["ws_bytes"], c
        tile = 2 * 32 * (2 * c.D + 16) + 2 * c.D * 80
        planes = c.B * c.heads * ((c.N + 31) // 32) * tile if c.N >= 128 and c.D <= 192 else 0
        assert p["ws_bytes"] == p["parts_bytes"] + planes, (c, p)
        assert p["parts_bytes"] % 16 == 0
        if p["merge"]:        # the launch's own parts (o: D floats, m and l: 2 floats per query, head and part) fit the buffers
            assert p["kparts"] * c.B * c.N * c.heads * (c.D + 2) * 4 <= p["parts_bytes"], (c, p)
        if "f16" in p["kernel"] and not p["short_seq"]:
            assert p["lds_bytes"] == tile * (2 if p["kv_planes"] else 1), (c, p)
        assert p["kv_planes"] == p["kernel"].endswith(",pre>") and (not p["kv_planes"] or planes > 0)
        assert p["kparts"] * p["tiles_per_part"] >= (c.N + 31) // 32 > (p["kparts"] - 1) * p["tiles_per_part"], (c, p)   # no empty part


def test_refusals_agree_with_the_launch(L):
    """What the launch refuses the query refuses with the same code: a head width without kernels (EVC_EUNSUPPORTED), sizes
    <= 0 and a plan that needs a workspace queried without one (EVC_EINVAL)."""
    H = L.hip_lib(require_device=False)
    out = L.AttentionPlan()
    q = lambda *a: H.evc_attention_plan_query(*a, ctypes.byref(out))       # noqa: E731
    for D in (96, 16, 0, 512):
        assert q(2, 2, 256, D, 0, 1, 0) == -2 and q(2, 2, 256, D, 1, 1, 1) == -2, D
    assert q(0, 2, 256, 64, 0, 1, 0) == -1 and q(2, 0, 256, 64, 0, 1, 0) == -1 and q(2, 2, 0, 64, 0, 1, 0) == -1
    assert H.evc_attention_plan_query(2, 2, 256, 64, 0, 1, 0, None) == -1
    # (9, 2, 1024, 192) splits the keys in both arithmetics and both modes: no answer without a workspace ...
    assert q(9, 2, 1024, 192, 1, 1, 1) == 0 and out.kparts > 1
    assert q(9, 2, 1024, 192, 1, 0, 1) == -1 and q(9, 2, 1024, 192, 0, 0, 1) == -1 and q(9, 2, 1024, 192, 1, 0, 0) == -1
    # ... except from evc_attention_f32, which never splits
    assert q(9, 2, 1024, 192, 0, 0, 0) == 0 and out.kparts == 1 and out.merge == 0
    with pytest.raises(L.EvcKernelError):
        L.attention_plan(2, 2, 256, 96)


def test_the_query_follows_the_options_in_default_mode_only(L):
    base = L.attention_plan(9, 4, 64, 192, with_bounds=True)
    inv = L.attention_plan(9, 4, 64, 192, with_bounds=True, invariant=True)
    assert base["kernel"] == "attention_short_kernel<192>" and inv["kernel"] == "attention_kernel<192,1>"
    with ledger.options(L, {"short_seq": 0, "f16_min_keys": 1, "kv_planes": 0}):
        assert L.attention_plan(9, 4, 64, 192, with_bounds=True)["kernel"].startswith("attention_f16_kernel<192,")
        assert L.attention_plan(9, 4, 64, 192, with_bounds=True, invariant=True) == inv
        assert not L.attention_plan(9, 2, 1024, 192, with_bounds=True)["kv_planes"]
        assert L.attention_plan(9, 2, 1024, 192, with_bounds=True, invariant=True)["kv_planes"]
    assert L.attention_plan(9, 4, 64, 192, with_bounds=True) == base
