"""The ledger of attention plan classes: which kernel instance every op-level parity case reaches, with or without a key
split, and which of them the shipped architectures launch.  A plain module (no fixtures): tests/test_attention_ledger_host.py
checks the table against the planner on the CPU (``lib.attention_plan`` = ``evc_attention_plan_query``),
tests/test_gpu_attention_ledger.py runs every entry against a float64 reference.

A plan class is the tuple

    (kernel instance, key split, batch-invariant plan)

- kernel instance: the name ``evc_attention_plan_query`` reports ("attention_kernel<192,4>", "attention_f16_kernel<192,4,pre>",
  "attention_short_f16_kernel<64>": head width, waves per workgroup, the K / V pre-pass);
- key split: kparts > 1, i.e. partial results in the workspace and attention_merge_kernel after the attention kernel;
- the batch-invariant flag is part of the class: the same kernel instance then reads one triple of bound words per sample.

``python tests/attention_ledger.py`` searches the planner for the cheapest case of every class the product reaches and prints
the ``CASES`` and ``NAMED`` tables; run it again when the planner moves a class and paste the result.
"""
from collections import namedtuple

DEFAULTS = {"kv_planes": 1, "f16_min_keys": 128, "short_seq": 1}          # evc_attention_set_option
WIDTHS = (32, 64, 128, 192, 256)
FAMILIES = ("attention_short_kernel", "attention_short_f16_kernel", "attention_kernel", "attention_f16_kernel",
            "attention_f16_kernel,pre")

# ``f16``: bound words are passed (the fp16-split arithmetic where the plan uses it).  ``options``: attention_set_option values
# other than the defaults.  ``ws``: "auto" -- a workspace exactly where the workspace size is not 0, as ``lib.attention`` and the
# networks call it; "none" -- evc_attention_f32, the entry point without one; "given" -- a workspace although the size is 0
# (the C entry points take one at any shape, and plan with it).
Case = namedtuple("Case", "B heads N D f16 invariant options cls ws", defaults=("auto",))

# Every L.attention call of the shipped architectures at full size (configs/mine.yml: 128 x 128 frames, ngf 192, 192-wide
# heads): (architecture, file:line of the call, heads, N, D, bounds passed on the fp16-split arithmetic, images per sample,
# batch-invariant mode exists).  The pseudo-3-D network attends over the pixels of every frame: 7 images per sample going down
# (5 frames + 2 of the condition), 5 going up.  unet_ddpm.py attends in one head as wide as the layer, at 64 x 64 and 16 x 16,
# for every ngf its constructor accepts.
Site = namedtuple("Site", "arch where heads N D with_bounds images invariant")
_SCORE = "scorenet.py:657"
SITES = [Site("unetmore", _SCORE, h, n, 192, True, (1,), True) for h, n in ((2, 1024), (3, 256), (4, 64))] + \
        [Site("unetmore-spade", _SCORE, h, n, 192, True, (1,), False) for h, n in ((2, 1024), (3, 256), (4, 64))] + \
        [Site("unetmorepseudo3d", _SCORE, h, n, 192, True, (5, 7), False) for h, n in ((2, 1024), (3, 256), (4, 64))] + \
        [Site("unet_ddpm", "unet_ddpm.py:230", 1, n, d, True, (1,), False) for d in WIDTHS for n in (4096, 256)]

BATCHES = tuple(range(1, 33))
INVARIANT_BATCHES = (1, 2, 9, 32)          # the batches of the conv ledger


def lib():
    import evc_amd  # noqa: F401
    from evc_amd import lib as L
    L.hip_lib(require_device=False)
    return L


class options:
    """``with options(L, {...}):`` -- the attention options for the block, the defaults again afterwards."""

    def __init__(self, L, values):
        self.L, self.values = L, dict(values)

    def __enter__(self):
        for k, v in self.values.items():
            self.L.attention_set_option(k, v)

    def __exit__(self, *exc):
        for k, v in DEFAULTS.items():
            self.L.attention_set_option(k, v)


HAVE_WS = {"auto": None, "none": False, "given": True}


def plan(L, B, heads, N, D, f16, invariant, opts=(), ws="auto"):
    with options(L, dict(opts)):
        return L.attention_plan(B, heads, N, D, with_bounds=bool(f16), have_ws=HAVE_WS[ws], invariant=bool(invariant))


def classify(p, invariant):
    return (p["kernel"], p["kparts"] > 1, bool(invariant))


def case_plan(c, L=None):
    return plan(L or lib(), c.B, c.heads, c.N, c.D, c.f16, c.invariant, c.options, c.ws)


def case_class(c, L=None):
    return classify(case_plan(c, L), c.invariant)


def family(cls):
    """The kernel family of a class: one of FAMILIES."""
    name, args = cls[0].rstrip(">").split("<")
    return name + (",pre" if args.endswith(",pre") else "")


def waves_of(cls):
    args = cls[0].rstrip(">").split("<")[1].split(",")
    return int(args[1]) if len(args) > 1 else 4


def product_launches():
    """Every (Case without class) the shipped architectures launch: SITES x B = 1..32 (default mode) or B in {1, 2, 9, 32}
    (invariant mode, where the architecture has one), with bound words and without (a model on bf16x6 passes none), options at
    their defaults."""
    for s in SITES:
        for invariant, batches in ((False, BATCHES), (True, INVARIANT_BATCHES)):
            if invariant and not s.invariant:
                continue
            for f16 in sorted({False, bool(s.with_bounds)}):
                for B in batches:
                    for images in s.images:
                        yield Case(B * images, s.heads, s.N, s.D, f16, invariant, {}, None)


def product_classes(L=None):
    L = L or lib()
    return {case_class(c, L) for c in product_launches()}


def cost(c):
    return c.B * c.heads * c.N * c.N * c.D


def case_id(c):
    kernel, split, inv = c.cls
    name = kernel.replace("attention_", "").replace("_kernel", "").replace("kernel", "f32").replace("<", "-").replace(">", "") \
        .replace(",", "-")
    return "-".join([name] + ["split"] * split + ["inv"] * inv + [f"b{c.B}h{c.heads}n{c.N}"] +
                    [f"{k}{v}" for k, v in sorted(c.options.items())] + ([c.ws] if c.ws != "auto" else []))


# One case per plan class the product reaches (``product_classes``), the cheapest the planner maps to it (invariant cases keep
# two samples: one triple of bound words per sample means something from two on); then EXTRA.
CASES = [
    Case(1, 1, 8, 128, False, False, {}, ('attention_short_kernel<128>', False, False)),
    Case(1, 1, 8, 192, False, False, {}, ('attention_short_kernel<192>', False, False)),
    Case(1, 1, 8, 32, False, False, {}, ('attention_short_kernel<32>', False, False)),
    Case(1, 1, 8, 64, False, False, {}, ('attention_short_kernel<64>', False, False)),
    Case(1, 1, 128, 128, True, False, {}, ('attention_short_f16_kernel<128>', False, False)),
    Case(1, 1, 128, 192, True, False, {}, ('attention_short_f16_kernel<192>', False, False)),
    Case(1, 1, 128, 32, True, False, {}, ('attention_short_f16_kernel<32>', False, False)),
    Case(1, 1, 128, 64, True, False, {}, ('attention_short_f16_kernel<64>', False, False)),
    Case(1, 1, 264, 128, False, False, {}, ('attention_kernel<128,1>', True, False)),
    Case(26, 1, 264, 128, False, False, {}, ('attention_kernel<128,2>', True, False)),
    Case(45, 4, 264, 128, False, False, {}, ('attention_kernel<128,4>', False, False)),
    Case(22, 2, 264, 128, False, False, {}, ('attention_kernel<128,4>', True, False)),
    Case(2, 1, 40, 192, False, True, {}, ('attention_kernel<192,1>', False, True)),
    Case(1, 1, 264, 192, False, False, {}, ('attention_kernel<192,1>', True, False)),
    Case(2, 1, 104, 192, False, True, {}, ('attention_kernel<192,1>', True, True)),
    Case(26, 1, 264, 192, False, False, {}, ('attention_kernel<192,2>', True, False)),
    Case(45, 4, 264, 192, False, False, {}, ('attention_kernel<192,4>', False, False)),
    Case(22, 2, 264, 192, False, False, {}, ('attention_kernel<192,4>', True, False)),
    Case(2, 4, 392, 192, False, True, {}, ('attention_kernel<192,4>', True, True)),
    Case(1, 1, 104, 256, False, False, {}, ('attention_kernel<256,1>', True, False)),
    Case(128, 1, 104, 256, False, False, {}, ('attention_kernel<256,2>', True, False)),
    Case(256, 1, 8, 256, False, False, {}, ('attention_kernel<256,4>', False, False)),
    Case(128, 1, 136, 256, False, False, {}, ('attention_kernel<256,4>', True, False)),
    Case(1, 1, 264, 32, False, False, {}, ('attention_kernel<32,1>', True, False)),
    Case(26, 1, 264, 32, False, False, {}, ('attention_kernel<32,2>', True, False)),
    Case(45, 4, 264, 32, False, False, {}, ('attention_kernel<32,4>', False, False)),
    Case(22, 2, 264, 32, False, False, {}, ('attention_kernel<32,4>', True, False)),
    Case(1, 1, 264, 64, False, False, {}, ('attention_kernel<64,1>', True, False)),
    Case(26, 1, 264, 64, False, False, {}, ('attention_kernel<64,2>', True, False)),
    Case(45, 4, 264, 64, False, False, {}, ('attention_kernel<64,4>', False, False)),
    Case(22, 2, 264, 64, False, False, {}, ('attention_kernel<64,4>', True, False)),
    Case(2, 1, 128, 192, True, True, {}, ('attention_f16_kernel<192,4>', True, True)),
    Case(29, 3, 520, 128, True, False, {}, ('attention_f16_kernel<128,4,pre>', False, False)),
    Case(1, 1, 512, 128, True, False, {}, ('attention_f16_kernel<128,4,pre>', True, False)),
    Case(29, 3, 520, 192, True, False, {}, ('attention_f16_kernel<192,4,pre>', False, False)),
    Case(1, 1, 512, 192, True, False, {}, ('attention_f16_kernel<192,4,pre>', True, False)),
    Case(2, 1, 512, 192, True, True, {}, ('attention_f16_kernel<192,4,pre>', True, True)),
    Case(29, 3, 520, 32, True, False, {}, ('attention_f16_kernel<32,4,pre>', False, False)),
    Case(1, 1, 512, 32, True, False, {}, ('attention_f16_kernel<32,4,pre>', True, False)),
    Case(29, 3, 520, 64, True, False, {}, ('attention_f16_kernel<64,4,pre>', False, False)),
    Case(1, 1, 512, 64, True, False, {}, ('attention_f16_kernel<64,4,pre>', True, False)),
]

# Every other template instantiation the public API reaches, and the edges each kernel family must show whatever its classes
# are: one key tile, a ragged last key tile, a ragged last query block, an uneven key split whose last part is one ragged tile,
# three key parts or more, every head width of the family (test_the_edges_of_every_kernel_family_are_in_the_ledger).  Kept by
# hand, each the cheapest found for its purpose; ``python tests/attention_ledger.py`` prints them with the class they plan to now.
# The fp16-split kernel at 1 or 2 waves never splits the keys: attention_plan_f16 gives 4 waves from 128 keys on, and below that
# there are at most 3 key tiles, too few for two parts of 2.
EXTRA = [
    # the fp16-split kernel without the K / V pre-pass, every head width at 1, 2 and 4 waves (the product reaches <192,4> only)
    Case(1, 1, 8, 128, True, False, {'short_seq': 0, 'f16_min_keys': 1}, ('attention_f16_kernel<128,1>', False, False)),
    Case(1, 1, 64, 128, True, False, {'short_seq': 0, 'f16_min_keys': 1}, ('attention_f16_kernel<128,2>', False, False), 'given'),
    Case(1, 1, 128, 128, True, False, {'short_seq': 0}, ('attention_f16_kernel<128,4>', True, False)),
    Case(1, 1, 8, 192, True, False, {'short_seq': 0, 'f16_min_keys': 1}, ('attention_f16_kernel<192,1>', False, False)),
    Case(1, 1, 64, 192, True, False, {'short_seq': 0, 'f16_min_keys': 1}, ('attention_f16_kernel<192,2>', False, False), 'given'),
    Case(1, 1, 8, 32, True, False, {'short_seq': 0, 'f16_min_keys': 1}, ('attention_f16_kernel<32,1>', False, False)),
    Case(1, 1, 64, 32, True, False, {'short_seq': 0, 'f16_min_keys': 1}, ('attention_f16_kernel<32,2>', False, False), 'given'),
    Case(1, 1, 128, 32, True, False, {'short_seq': 0}, ('attention_f16_kernel<32,4>', True, False)),
    Case(1, 1, 8, 64, True, False, {'short_seq': 0, 'f16_min_keys': 1}, ('attention_f16_kernel<64,1>', False, False)),
    Case(1, 1, 64, 64, True, False, {'short_seq': 0, 'f16_min_keys': 1}, ('attention_f16_kernel<64,2>', False, False), 'given'),
    Case(1, 1, 128, 64, True, False, {'short_seq': 0}, ('attention_f16_kernel<64,4>', True, False)),
    # edges of the families
    Case(1, 1, 40, 32, False, False, {}, ('attention_short_kernel<32>', False, False)),
    Case(1, 1, 8, 32, True, False, {'f16_min_keys': 1}, ('attention_short_f16_kernel<32>', False, False)),
    Case(1, 1, 40, 32, True, False, {'f16_min_keys': 1}, ('attention_short_f16_kernel<32>', False, False)),
    Case(1, 1, 8, 32, False, False, {'short_seq': 0}, ('attention_kernel<32,1>', False, False)),
    Case(1, 1, 40, 32, True, False, {'short_seq': 0, 'f16_min_keys': 1}, ('attention_f16_kernel<32,1>', False, False)),
    Case(1, 1, 200, 32, True, False, {'short_seq': 0}, ('attention_f16_kernel<32,4>', True, False)),
    Case(1, 1, 584, 32, True, False, {}, ('attention_f16_kernel<32,4,pre>', True, False)),
    Case(2, 2, 32, 64, False, False, {}, ('attention_short_kernel<64>', False, False)),
    Case(2, 2, 32, 64, True, False, {'f16_min_keys': 1}, ('attention_short_f16_kernel<64>', False, False)),
    Case(3, 1, 200, 128, False, False, {}, ('attention_short_kernel<128>', False, False)),
    Case(3, 1, 200, 128, True, False, {}, ('attention_short_f16_kernel<128>', False, False)),
    Case(1, 1, 296, 64, False, False, {}, ('attention_kernel<64,1>', True, False)),
    Case(2, 2, 200, 192, True, True, {}, ('attention_f16_kernel<192,4>', True, True)),
    Case(2, 3, 200, 64, False, True, {}, ('attention_kernel<64,1>', True, True)),
    Case(256, 1, 64, 32, True, False, {'short_seq': 0, 'f16_min_keys': 1}, ('attention_f16_kernel<32,4>', False, False)),
    Case(2, 1, 1000, 128, True, False, {}, ('attention_f16_kernel<128,4,pre>', True, False)),
    # the no-workspace plans of evc_attention_f32 (waves by EVC_ATTN_MIN_WG, never a key split) at 1, 2 and 4 waves
    Case(1, 1, 264, 32, False, False, {}, ('attention_kernel<32,1>', False, False), 'none'),
    Case(32, 2, 264, 32, False, False, {}, ('attention_kernel<32,2>', False, False), 'none'),
    Case(128, 1, 264, 32, False, False, {}, ('attention_kernel<32,4>', False, False), 'none'),
    # kv_planes = 0: the 4-wave fp16-split kernel converting every tile itself from 512 keys on
    Case(1, 1, 512, 32, True, False, {'kv_planes': 0}, ('attention_f16_kernel<32,4>', True, False)),
]
CASES = CASES + EXTRA

# Template instantiations of csrc/attention.hip that no call of the public API reaches, each with its reason.
UNREACHABLE = [
    ("attention_short_kernel<256>", "launch<256> never takes the short-sequence path (it sits behind `if constexpr (F16_OK)`, "
                                    "D <= 192, and attention_resolve asks the same), so the template is not instantiated"),
    ("attention_short_f16_kernel<256>", "as above, and the fp16-split form keeps Q and O in registers: no head width above 192"),
    ("attention_f16_kernel<256,*>", "head widths above 192 stay on the f32 kernel (F16_OK in launch<D>): not instantiated"),
    ("attention_kv_planes_kernel<256>", "only the fp16-split kernel reads the K / V tile images"),
    ("attention_f16_kernel<*,1,pre> / <*,2,pre>", "the pre-pass is taken with 4 waves only (attention_resolve); the launch names "
                                                  "<D,4,true> alone, so these are not instantiated"),
]


# ---- the older parity tests -----------------------------------------------------------------------------------------------
# The launches each of them makes per parametrize tuple: -> [(B, heads, N, D, f16, options, ws)], both forms of the test's
# arithmetic fixture.
_F16_ANY = {"f16_min_keys": 1}         # test_gpu_attention_short.run: the fp16 form at every key count
KEY_SPLIT_SHAPES = ((1, 2, 200, 192), (2, 1, 1024, 64), (9, 2, 1024, 192))      # the loop of test_attention_key_split_...


def _ops_both(B, heads, N, D):
    return [(B, heads, N, D, f16, {}, "auto") for f16 in (False, True)]


def _short_both(B, heads, N, D):
    return [(B, heads, N, D, False, {}, "auto"), (B, heads, N, D, True, _F16_ANY, "auto")]


NAMED_TESTS = {
    ("test_gpu_ops", "test_attention"): _ops_both,
    ("test_gpu_ops", "test_attention_peaked_scores_exercise_the_rescale"): None,        # not parametrized: one shape
    ("test_gpu_ops", "test_attention_key_split_matches_single_pass"): None,             # not parametrized: KEY_SPLIT_SHAPES
    ("test_gpu_ops", "test_attention_kv_planes_equal_the_in_kernel_conversion"):
        lambda B, heads, N, D: [(B, heads, N, D, True, {"kv_planes": 0}, "auto"), (B, heads, N, D, True, {}, "auto")],
    ("test_gpu_attention_short", "test_parity_with_float64"): _short_both,
    ("test_gpu_attention_short", "test_dispatch_boundary"): lambda N: _short_both(1, 2, N, 64),
}
Named = namedtuple("Named", "test B heads N D f16 options ws cls")


def named_launches(module, test):
    """The launches a test stands for today, read from the test module itself: Named tuples without class."""
    import importlib
    import inspect
    fn = getattr(importlib.import_module(module), test)
    read = NAMED_TESTS[(module, test)]
    if test == "test_attention_peaked_scores_exercise_the_rescale":
        assert "B, heads, N, D = 1, 1, 128, 32" in inspect.getsource(fn)
        rows = _ops_both(1, 1, 128, 32)
    elif test == "test_attention_key_split_matches_single_pass":
        assert f"in {KEY_SPLIT_SHAPES!r}:" in inspect.getsource(fn)
        rows = []
        for s in KEY_SPLIT_SHAPES:        # evc_attention_ws_f32, evc_attention_f32, evc_attention_f16x3_f32 on one workspace
            rows += [s + (False, {}, "auto"), s + (False, {}, "none"), s + (True, {}, "auto")]
    else:
        marks = [m for m in fn.pytestmark if m.name == "parametrize"]
        assert len(marks) == 1, (module, test)
        rows = []
        for params in marks[0].args[1]:
            rows += read(*(params if isinstance(params, (tuple, list)) else (params,)))
    for r in rows:
        yield Named(test, *r, None)


def named_class(n):
    """The class ``NAMED`` states for one launch of an older test (KeyError: the test has a case the table does not know)."""
    for m in NAMED:
        if m._replace(cls=None) == n._replace(cls=None):
            return m.cls
    raise KeyError(n)


# The class every launch of those tests reaches today.  tests/test_attention_ledger_host.py fails, naming the test, when the
# planner moves one of them.
NAMED = [
    Named('test_attention', 2, 2, 1024, 192, False, {}, 'auto',
          ('attention_kernel<192,1>', True, False)),
    Named('test_attention', 2, 2, 1024, 192, True, {}, 'auto',
          ('attention_f16_kernel<192,4,pre>', True, False)),
    Named('test_attention', 1, 4, 64, 192, False, {}, 'auto',
          ('attention_short_kernel<192>', False, False)),
    Named('test_attention', 1, 4, 64, 192, True, {}, 'auto',
          ('attention_short_kernel<192>', False, False)),
    Named('test_attention', 2, 3, 256, 192, False, {}, 'auto',
          ('attention_short_kernel<192>', False, False)),
    Named('test_attention', 2, 3, 256, 192, True, {}, 'auto',
          ('attention_short_f16_kernel<192>', False, False)),
    Named('test_attention', 2, 2, 96, 32, False, {}, 'auto',
          ('attention_short_kernel<32>', False, False)),
    Named('test_attention', 2, 2, 96, 32, True, {}, 'auto',
          ('attention_short_kernel<32>', False, False)),
    Named('test_attention', 1, 1, 64, 64, False, {}, 'auto',
          ('attention_short_kernel<64>', False, False)),
    Named('test_attention', 1, 1, 64, 64, True, {}, 'auto',
          ('attention_short_kernel<64>', False, False)),
    Named('test_attention', 2, 1, 256, 128, False, {}, 'auto',
          ('attention_short_kernel<128>', False, False)),
    Named('test_attention', 2, 1, 256, 128, True, {}, 'auto',
          ('attention_short_f16_kernel<128>', False, False)),
    Named('test_attention', 1, 2, 64, 128, False, {}, 'auto',
          ('attention_short_kernel<128>', False, False)),
    Named('test_attention', 1, 2, 64, 128, True, {}, 'auto',
          ('attention_short_kernel<128>', False, False)),
    Named('test_attention', 2, 1, 256, 256, False, {}, 'auto',
          ('attention_kernel<256,1>', True, False)),
    Named('test_attention', 2, 1, 256, 256, True, {}, 'auto',
          ('attention_kernel<256,1>', True, False)),
    Named('test_attention', 1, 1, 100, 256, False, {}, 'auto',
          ('attention_kernel<256,1>', True, False)),
    Named('test_attention', 1, 1, 100, 256, True, {}, 'auto',
          ('attention_kernel<256,1>', True, False)),
    Named('test_attention_peaked_scores_exercise_the_rescale', 1, 1, 128, 32, False, {}, 'auto',
          ('attention_short_kernel<32>', False, False)),
    Named('test_attention_peaked_scores_exercise_the_rescale', 1, 1, 128, 32, True, {}, 'auto',
          ('attention_short_f16_kernel<32>', False, False)),
    Named('test_attention_key_split_matches_single_pass', 1, 2, 200, 192, False, {}, 'auto',
          ('attention_short_kernel<192>', False, False)),
    Named('test_attention_key_split_matches_single_pass', 1, 2, 200, 192, False, {}, 'none',
          ('attention_short_kernel<192>', False, False)),
    Named('test_attention_key_split_matches_single_pass', 1, 2, 200, 192, True, {}, 'auto',
          ('attention_short_f16_kernel<192>', False, False)),
    Named('test_attention_key_split_matches_single_pass', 2, 1, 1024, 64, False, {}, 'auto',
          ('attention_kernel<64,1>', True, False)),
    Named('test_attention_key_split_matches_single_pass', 2, 1, 1024, 64, False, {}, 'none',
          ('attention_kernel<64,1>', False, False)),
    Named('test_attention_key_split_matches_single_pass', 2, 1, 1024, 64, True, {}, 'auto',
          ('attention_f16_kernel<64,4,pre>', True, False)),
    Named('test_attention_key_split_matches_single_pass', 9, 2, 1024, 192, False, {}, 'auto',
          ('attention_kernel<192,4>', True, False)),
    Named('test_attention_key_split_matches_single_pass', 9, 2, 1024, 192, False, {}, 'none',
          ('attention_kernel<192,2>', False, False)),
    Named('test_attention_key_split_matches_single_pass', 9, 2, 1024, 192, True, {}, 'auto',
          ('attention_f16_kernel<192,4,pre>', True, False)),
    Named('test_attention_kv_planes_equal_the_in_kernel_conversion', 9, 2, 1024, 192, True, {'kv_planes': 0}, 'auto',
          ('attention_f16_kernel<192,4>', True, False)),
    Named('test_attention_kv_planes_equal_the_in_kernel_conversion', 9, 2, 1024, 192, True, {}, 'auto',
          ('attention_f16_kernel<192,4,pre>', True, False)),
    Named('test_attention_kv_planes_equal_the_in_kernel_conversion', 2, 3, 576, 192, True, {'kv_planes': 0}, 'auto',
          ('attention_f16_kernel<192,4>', True, False)),
    Named('test_attention_kv_planes_equal_the_in_kernel_conversion', 2, 3, 576, 192, True, {}, 'auto',
          ('attention_f16_kernel<192,4,pre>', True, False)),
    Named('test_attention_kv_planes_equal_the_in_kernel_conversion', 1, 2, 1000, 192, True, {'kv_planes': 0}, 'auto',
          ('attention_f16_kernel<192,4>', True, False)),
    Named('test_attention_kv_planes_equal_the_in_kernel_conversion', 1, 2, 1000, 192, True, {}, 'auto',
          ('attention_f16_kernel<192,4,pre>', True, False)),
    Named('test_attention_kv_planes_equal_the_in_kernel_conversion', 2, 1, 512, 128, True, {'kv_planes': 0}, 'auto',
          ('attention_f16_kernel<128,4>', True, False)),
    Named('test_attention_kv_planes_equal_the_in_kernel_conversion', 2, 1, 512, 128, True, {}, 'auto',
          ('attention_f16_kernel<128,4,pre>', True, False)),
    Named('test_attention_kv_planes_equal_the_in_kernel_conversion', 3, 2, 640, 64, True, {'kv_planes': 0}, 'auto',
          ('attention_f16_kernel<64,4>', True, False)),
    Named('test_attention_kv_planes_equal_the_in_kernel_conversion', 3, 2, 640, 64, True, {}, 'auto',
          ('attention_f16_kernel<64,4,pre>', True, False)),
    Named('test_attention_kv_planes_equal_the_in_kernel_conversion', 2, 4, 520, 32, True, {'kv_planes': 0}, 'auto',
          ('attention_f16_kernel<32,4>', True, False)),
    Named('test_attention_kv_planes_equal_the_in_kernel_conversion', 2, 4, 520, 32, True, {}, 'auto',
          ('attention_f16_kernel<32,4,pre>', True, False)),
    Named('test_attention_kv_planes_equal_the_in_kernel_conversion', 2, 3, 256, 192, True, {'kv_planes': 0}, 'auto',
          ('attention_short_f16_kernel<192>', False, False)),
    Named('test_attention_kv_planes_equal_the_in_kernel_conversion', 2, 3, 256, 192, True, {}, 'auto',
          ('attention_short_f16_kernel<192>', False, False)),
    Named('test_parity_with_float64', 1, 1, 32, 32, False, {}, 'auto',
          ('attention_short_kernel<32>', False, False)),
    Named('test_parity_with_float64', 1, 1, 32, 32, True, {'f16_min_keys': 1}, 'auto',
          ('attention_short_f16_kernel<32>', False, False)),
    Named('test_parity_with_float64', 1, 4, 64, 192, False, {}, 'auto',
          ('attention_short_kernel<192>', False, False)),
    Named('test_parity_with_float64', 1, 4, 64, 192, True, {'f16_min_keys': 1}, 'auto',
          ('attention_short_f16_kernel<192>', False, False)),
    Named('test_parity_with_float64', 2, 2, 64, 192, False, {}, 'auto',
          ('attention_short_kernel<192>', False, False)),
    Named('test_parity_with_float64', 2, 2, 64, 192, True, {'f16_min_keys': 1}, 'auto',
          ('attention_short_f16_kernel<192>', False, False)),
    Named('test_parity_with_float64', 2, 3, 256, 192, False, {}, 'auto',
          ('attention_short_kernel<192>', False, False)),
    Named('test_parity_with_float64', 2, 3, 256, 192, True, {'f16_min_keys': 1}, 'auto',
          ('attention_short_f16_kernel<192>', False, False)),
    Named('test_parity_with_float64', 1, 1, 40, 64, False, {}, 'auto',
          ('attention_short_kernel<64>', False, False)),
    Named('test_parity_with_float64', 1, 1, 40, 64, True, {'f16_min_keys': 1}, 'auto',
          ('attention_short_f16_kernel<64>', False, False)),
    Named('test_parity_with_float64', 3, 1, 200, 128, False, {}, 'auto',
          ('attention_short_kernel<128>', False, False)),
    Named('test_parity_with_float64', 3, 1, 200, 128, True, {'f16_min_keys': 1}, 'auto',
          ('attention_short_f16_kernel<128>', False, False)),
    Named('test_parity_with_float64', 2, 2, 96, 32, False, {}, 'auto',
          ('attention_short_kernel<32>', False, False)),
    Named('test_parity_with_float64', 2, 2, 96, 32, True, {'f16_min_keys': 1}, 'auto',
          ('attention_short_f16_kernel<32>', False, False)),
    Named('test_parity_with_float64', 1, 2, 256, 32, False, {}, 'auto',
          ('attention_short_kernel<32>', False, False)),
    Named('test_parity_with_float64', 1, 2, 256, 32, True, {'f16_min_keys': 1}, 'auto',
          ('attention_short_f16_kernel<32>', False, False)),
    Named('test_dispatch_boundary', 1, 2, 256, 64, False, {}, 'auto',
          ('attention_short_kernel<64>', False, False)),
    Named('test_dispatch_boundary', 1, 2, 256, 64, True, {'f16_min_keys': 1}, 'auto',
          ('attention_short_f16_kernel<64>', False, False)),
    Named('test_dispatch_boundary', 1, 2, 288, 64, False, {}, 'auto',
          ('attention_kernel<64,1>', True, False)),
    Named('test_dispatch_boundary', 1, 2, 288, 64, True, {'f16_min_keys': 1}, 'auto',
          ('attention_f16_kernel<64,4>', True, False)),
]


# ---- the search that wrote CASES ------------------------------------------------------------------------------------------

_SEARCH_N = tuple(range(8, 1025, 8)) + (2048, 4096)
_SEARCH_B = tuple(range(1, 33)) + (35, 40, 45, 63, 64, 70, 128, 160, 224, 256)


def search():
    """The cheapest case (B * heads * N^2 * D) of every class of the product, options at their defaults, as the networks call."""
    L = lib()
    want = product_classes(L)
    best = {}
    for invariant in (False, True):
        for f16 in (False, True):
            for D in WIDTHS:
                for heads in (1, 2, 3, 4):
                    for N in _SEARCH_N:
                        for B in ((2,) if invariant else _SEARCH_B):        # the invariant plan does not depend on B
                            c = Case(B, heads, N, D, f16, invariant, {}, None)
                            try:
                                cls = case_class(c, L)
                            except L.EvcKernelError:
                                continue
                            if cls in want and (cls not in best or cost(c) < cost(best[cls])):
                                best[cls] = c._replace(cls=cls)
    assert set(best) == want, want - set(best)
    return [best[k] for k in sorted(best, key=lambda k: (FAMILIES.index(family(k)), str(k)))]


def _fmt(c):
    tail = "" if c.ws == "auto" else f", {c.ws!r}"
    return f"    Case({c.B}, {c.heads}, {c.N}, {c.D}, {c.f16!s}, {c.invariant!s}, {c.options!r}, {c.cls!r}{tail}),"


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("CASES = [")
    for c in search():
        print(_fmt(c))
    print("]\n\nEXTRA = [")
    L = lib()
    for c in EXTRA:
        print(_fmt(c._replace(cls=case_class(c, L))))
    print("]\n\nNAMED = [")
    for module, test in NAMED_TESTS:
        for n in named_launches(module, test):
            cls = classify(plan(L, n.B, n.heads, n.N, n.D, n.f16, False, n.options, n.ws), False)
            print(f"    Named({n.test!r}, {n.B}, {n.heads}, {n.N}, {n.D}, {n.f16!s}, {n.options!r}, {n.ws!r},\n          {cls!r}),")
    print("]")
