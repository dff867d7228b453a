"""CPU tests of batch-invariant mode: the convolution planner queried without a GPU
(``lib.conv_plan`` -> ``evc_conv_plan_query``, as tests/test_host_logic.py queries the default planner), container format 4,
and what the mode refuses.  The GPU side -- bitwise equality of a sample alone and inside any batch -- is
tests/test_gpu_batch_invariant.py, which also checks that FULL_SIZE_CONVS below is what a real forward launches."""
import struct

import numpy as np
import pytest

from test_job_stream_host import N_KEY, SEGMENTS, packed

F16, BF16 = 2, 1        # lib.ARITH_F16X3 / ARITH_BF16X6
SILU = 1

# Every distinct convolution launch of the full-size (ngf 192, 128 x 128) forward in batch-invariant mode:
# (H, W, C0, C1, Co, K, arith, GroupNorm coefficients on load, activation on load, channels of a fused 1x1 operand,
# whether the launch carries an element bound of its raw operand: the `bound` field ``lib.CONV_PROFILE`` records).
FULL_SIZE_CONVS = [
    (8, 8, 576, 0, 576, 1, 2, 0, 0, 0, 1),
    (8, 8, 576, 0, 576, 3, 2, 0, 0, 0, 0),
    (8, 8, 576, 0, 576, 3, 2, 1, 1, 0, 0),
    (8, 8, 576, 0, 768, 1, 2, 0, 0, 0, 1),
    (8, 8, 576, 0, 768, 3, 2, 1, 1, 0, 0),
    (8, 8, 768, 0, 768, 1, 2, 0, 0, 0, 1),
    (8, 8, 768, 0, 768, 3, 2, 1, 1, 0, 0),
    (8, 8, 768, 0, 2304, 1, 2, 1, 0, 0, 0),
    (8, 8, 768, 576, 768, 1, 2, 0, 0, 0, 1),
    (8, 8, 768, 576, 768, 3, 2, 1, 1, 0, 0),
    (8, 8, 768, 768, 768, 1, 2, 0, 0, 0, 1),
    (8, 8, 768, 768, 768, 3, 2, 1, 1, 0, 0),
    (16, 16, 384, 0, 384, 3, 2, 0, 0, 0, 0),
    (16, 16, 384, 0, 384, 3, 2, 1, 1, 384, 0),
    (16, 16, 384, 0, 576, 3, 2, 1, 1, 0, 0),
    (16, 16, 576, 0, 576, 1, 2, 0, 0, 0, 1),
    (16, 16, 576, 0, 576, 3, 2, 1, 1, 0, 0),
    (16, 16, 576, 0, 576, 3, 2, 1, 1, 384, 0),
    (16, 16, 576, 0, 576, 3, 2, 1, 1, 960, 0),
    (16, 16, 576, 0, 576, 3, 2, 1, 1, 1152, 0),
    (16, 16, 576, 0, 576, 3, 2, 1, 1, 1344, 0),
    (16, 16, 576, 0, 1728, 1, 2, 1, 0, 0, 0),
    (16, 16, 576, 384, 576, 3, 2, 1, 1, 0, 0),
    (16, 16, 576, 576, 576, 3, 2, 1, 1, 0, 0),
    (16, 16, 768, 0, 768, 3, 2, 0, 0, 0, 0),
    (16, 16, 768, 0, 768, 3, 2, 1, 1, 768, 0),
    (16, 16, 768, 576, 576, 3, 2, 1, 1, 0, 0),
    (32, 32, 192, 0, 192, 3, 2, 0, 0, 0, 0),
    (32, 32, 192, 0, 192, 3, 2, 1, 1, 192, 0),
    (32, 32, 192, 0, 384, 3, 2, 1, 1, 0, 0),
    (32, 32, 384, 0, 384, 1, 2, 0, 0, 0, 1),
    (32, 32, 384, 0, 384, 3, 2, 1, 1, 0, 0),
    (32, 32, 384, 0, 384, 3, 2, 1, 1, 192, 0),
    (32, 32, 384, 0, 384, 3, 2, 1, 1, 576, 0),
    (32, 32, 384, 0, 384, 3, 2, 1, 1, 768, 0),
    (32, 32, 384, 0, 384, 3, 2, 1, 1, 960, 0),
    (32, 32, 384, 0, 1152, 1, 2, 1, 0, 0, 0),
    (32, 32, 384, 192, 384, 3, 2, 1, 1, 0, 0),
    (32, 32, 384, 384, 384, 3, 2, 1, 1, 0, 0),
    (32, 32, 576, 0, 576, 3, 2, 0, 0, 0, 0),
    (32, 32, 576, 0, 576, 3, 2, 1, 1, 576, 0),
    (32, 32, 576, 384, 384, 3, 2, 1, 1, 0, 0),
    (64, 64, 192, 0, 192, 3, 2, 0, 0, 0, 0),
    (64, 64, 192, 0, 192, 3, 2, 1, 1, 0, 0),
    (64, 64, 192, 0, 192, 3, 2, 1, 1, 192, 0),
    (64, 64, 192, 0, 192, 3, 2, 1, 1, 384, 0),
    (64, 64, 192, 0, 192, 3, 2, 1, 1, 576, 0),
    (64, 64, 192, 192, 192, 3, 2, 1, 1, 0, 0),
    (64, 64, 384, 0, 384, 3, 2, 0, 0, 0, 0),
    (64, 64, 384, 0, 384, 3, 2, 1, 1, 384, 0),
    (64, 64, 384, 192, 192, 3, 2, 1, 1, 0, 0),
    (128, 128, 32, 0, 192, 3, 1, 0, 0, 0, 0),
    (128, 128, 192, 0, 15, 3, 2, 1, 1, 0, 0),
    (128, 128, 192, 0, 192, 3, 2, 0, 0, 0, 0),
    (128, 128, 192, 0, 192, 3, 2, 1, 1, 0, 0),
    (128, 128, 192, 0, 192, 3, 2, 1, 1, 192, 0),
    (128, 128, 192, 0, 192, 3, 2, 1, 1, 384, 0),
    (128, 128, 192, 192, 192, 3, 2, 1, 1, 0, 0),
]


def lib():
    import evc_amd  # noqa: F401
    from evc_amd import lib as L
    L.hip_lib(require_device=False)
    return L


def plan(L, cfg, B, arith=None, invariant=True):
    H, W, C0, C1, Co, K, ar, coef, act, x2, _bound = cfg
    ar = ar if arith is None else arith
    if ar != F16:
        x2 = 0                                   # the fused 1x1 operand exists on the fp16 split only
    return L.conv_plan(B, H, W, C0, C1, Co, K, ar, coef=bool(coef), act_in=act, x2_ci=x2, invariant=invariant)


@pytest.mark.parametrize("arith", [None, BF16], ids=["f16x3", "bf16x6"])
def test_invariant_plan_is_the_same_for_every_batch(arith):
    """Kernel, tile, split count and boundaries, cut, tail and moment runs of every full-size launch, B = 1 .. 64, under the
    network's own arithmetic and with every layer demoted to bf16x6.

    On the parent commit ``lib.conv_plan`` does not exist; with the mode flag ignored (``invariant=False`` below) the same
    query gives 3 / 1 splits at B = 1 / 32 for 128 x 128 192->192 and plans that differ between B = 1, 2, 9 and 32 for
    nearly every launch of the list (test_default_plan_does_depend_on_the_batch asserts both)."""
    L = lib()
    for cfg in FULL_SIZE_CONVS:
        first = plan(L, cfg, 1, arith)
        assert first["tail_tiles"] == 0 and first["tail_splits"] == 1, (cfg, first)
        for B in range(2, 65):
            assert plan(L, cfg, B, arith) == first, (cfg, B)
        if cfg[9] and arith is None:
            assert first["fused_1x1"], cfg       # the literal list only fuses where the plan accepts it
            assert (cfg[0] * cfg[1]) % first["tile"][0] == 0, cfg


def test_default_plan_does_depend_on_the_batch():
    """The same query without the flag: the parent's planner.  So the test above cannot pass vacuously."""
    L = lib()
    cfg = (128, 128, 192, 0, 192, 3, F16, 1, SILU, 0, 0)
    by_b = {B: plan(L, cfg, B, invariant=False) for B in (1, 2, 9, 32)}
    assert [by_b[B]["splits"] for B in (1, 2, 9, 32)] == [3, 2, 1, 1]
    assert by_b[9]["tail_tiles"] > 0 and by_b[9]["tail_splits"] == 4 and by_b[32]["tail_tiles"] == 0
    assert all(p["kernel"].startswith("conv_wide_kernel") for p in by_b.values())
    # the last row of the issue's table: the moment runs of 16 x 16 576->576 1x1 follow the batch
    one = (16, 16, 576, 0, 576, 1, F16, 0, 0, 0, 1)
    assert [plan(L, one, B, invariant=False)["stats_runs"] for B in (1, 9, 32)] == [4, 4, 8]
    assert [plan(L, one, B, invariant=False)["splits"] for B in (1, 9, 32)] == [9, 4, 1]
    differing = sum(1 for c in FULL_SIZE_CONVS if len({str(plan(L, c, B, invariant=False)) for B in (1, 2, 9, 32)}) > 1)
    assert differing >= 50, differing


def test_invariant_plan_keeps_the_wide_kernel_where_the_default_has_it_at_b9():
    """The f16x3 3x3 layers at 128 x 128, 64 x 64 and 32 x 32 that run conv_wide_kernel by default at B = 9 run it in invariant
    mode at every B, with the default's split count at B = 9 (the measured one) and no tail."""
    L = lib()
    n = 0
    for cfg in FULL_SIZE_CONVS:
        d9 = plan(L, cfg, 9, invariant=False) if not cfg[9] or L.conv_fused_1x1_supported(9, *cfg[:2], cfg[4], cfg[4], F16) \
            else None
        if d9 is None or not d9["kernel"].startswith("conv_wide_kernel"):
            continue
        for B in (1, 9, 32):
            p = plan(L, cfg, B)
            assert p["kernel"] == d9["kernel"] and p["splits"] == d9["splits"] and p["cut_chunk"] == d9["cut_chunk"], (cfg, B)
        n += 1
    assert n >= 25, n


def test_plan_ignores_the_process_wide_switches_in_invariant_mode():
    L = lib()
    cfg = (64, 64, 192, 192, 192, 3, F16, 1, SILU, 0, 0)
    want = plan(L, cfg, 9)
    try:
        for name in ("wide256", "wide_mid", "wide_cut", "tail_split", "row_reuse", "wide_tiles"):
            L.conv_set_option(name, 0)
        assert plan(L, cfg, 9) == want
        assert plan(L, cfg, 9, invariant=False) != want
    finally:
        for name in ("wide256", "wide_mid", "wide_cut", "tail_split", "row_reuse", "wide_tiles"):
            L.conv_set_option(name, 1)


def test_chan_stats_ranges_and_revision():
    L = lib()
    for HW in (16, 64, 256, 1024, 4096, 16384):
        assert len({L.stats_splits(B, HW, invariant=True) for B in range(1, 65)}) == 1
    assert L.stats_splits(1, 16384) != L.stats_splits(32, 16384)          # the default follows B
    assert L.invariant_plan_revision() >= 1


# ---- container format 4 -----------------------------------------------------------------------------------------

def test_format_4_round_trip_and_format_3_unchanged():
    import evc_amd  # noqa: F401
    from evc_amd import container
    x = np.random.default_rng(3).random((29, 3, 8, 8), dtype=np.float32)
    crc = container.frames_crc(x)
    plain = packed()
    assert plain[4] == 3
    blob = packed(plan=(container.PLAN_INVARIANT, 7), crc=crc)
    assert blob[4] == 4 and len(blob) == len(plain) + 7
    job = container.unpack_job(blob, expect_plan_revision=7)
    assert job["format"] == 4 and job["plan"] == (1, 7) and job["crc"] == crc
    old = container.unpack_job(plain, expect_plan_revision=7)
    assert old["format"] == 3 and old["plan"] is None and old["crc"] is None
    for k in ("segments", "key_strings", "seed", "stream_id", "vid", "q", "sampler", "subsample", "denoise", "frames", "shape"):
        assert job[k] == old[k], k
    assert job["segments"] == SEGMENTS and len(job["key_strings"]) == N_KEY
    # format 4 with the plan head cut out again is the format-3 stream, byte for byte
    head = 8 + struct.calcsize(container._JOB_HEAD)
    assert bytes([blob[0], blob[1], blob[2], blob[3], 3]) + blob[5:head] + blob[head + 7:] == plain
    # the CRC is of the float32 bytes: one ulp in one element changes it
    y = x.copy()
    y[5, 1, 2, 3] = np.nextafter(y[5, 1, 2, 3], np.float32(2))
    assert container.frames_crc(y) != crc and container.frames_crc(x.astype(np.float64)) == crc


def test_non_invariant_job_packs_to_todays_bytes():
    """The literal head of a format-3 stream, as the parent commit writes it."""
    import evc_amd  # noqa: F401
    from evc_amd import container
    blob = packed()
    want = b"EVC1" + struct.pack("<BBH", 3, 0, 3) + struct.pack("<BQIIBfBHBHHHHH", 1, (9 << 32) | 1234, 41, 17, 4, 0.29, 0, 100, 1,
                                                              sum(n for _, n in SEGMENTS), 2, 2, N_KEY, len(SEGMENTS))
    assert blob[:len(want)] == want
    assert blob[len(want):len(want) + 2 * len(SEGMENTS)] == b"".join(
        struct.pack("<BB", container.SEGMENT_KINDS.index(k), n) for k, n in SEGMENTS)


def test_unknown_plan_and_other_revision_are_refused():
    import evc_amd  # noqa: F401
    from evc_amd import container
    blob = packed(plan=(container.PLAN_INVARIANT, 7), crc=1)
    with pytest.raises(container.PlanMismatch, match="revision 7"):
        container.unpack_job(blob, expect_plan_revision=8)
    head = 8 + struct.calcsize(container._JOB_HEAD)
    foreign = blob[:head] + bytes([2]) + blob[head + 1:]
    with pytest.raises(container.PlanMismatch, match="plan id 2"):
        container.unpack_job(foreign)
    with pytest.raises(ValueError):
        packed(plan=(2, 7), crc=1)
    with pytest.raises(ValueError):
        packed(plan=(1, 7))                      # no CRC
    with pytest.raises(ValueError, match="truncated"):
        container.unpack_job(blob[:head + 3])
    assert issubclass(container.PlanMismatch, ValueError)


# ---- refusals ---------------------------------------------------------------------------------------------------

class _Net:
    device = "cpu"

    def invariant_view(self):
        return self


def _decoder(**kw):
    import evc_amd  # noqa: F401
    from evc_amd.config import default_config
    from evc_amd.decoder import ClipDecoder
    return ClipDecoder(_Net(), None, default_config(32, 32, 32), None, **kw)


def test_invariant_refuses_range_recovery():
    with pytest.raises(ValueError, match="range recovery"):
        _decoder(range_recovery="layer", batch_invariant=True)
    dec = _decoder(range_recovery="layer")
    with pytest.raises(ValueError, match="range recovery"):
        dec.generate(None, invariant=True)
    import evc_amd  # noqa: F401
    from evc_amd import policy as P
    with pytest.raises(ValueError, match="range recovery"):
        P.run_policy(dec, {}, {}, [3], [0.0], None, noise="evc", batch_invariant=True)


def test_invariant_refuses_torch_noise():
    import evc_amd  # noqa: F401
    from evc_amd import policy as P
    with pytest.raises(ValueError, match="noise='evc'"):
        P.run_policy(_decoder(), {}, {}, [3], [0.0], None, noise="torch", batch_invariant=True)


def test_command_lines_refuse_what_the_mode_refuses(capsys):
    import evc_amd  # noqa: F401
    from evc_amd import cli
    base = ["--policy", "psnr", "--batch-invariant", "--synthetic"]
    for extra, word in ((["--range-recovery", "layer"], "range-recovery"), (["--noise", "torch"], "--noise torch")):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert word in str(e.value), e.value
    with pytest.raises(SystemExit) as e:
        cli.main(["--policy", "mask", "--batch-invariant", "--synthetic"])
    assert "policy" in str(e.value)


def test_other_network_families_refuse_the_flag():
    import evc_amd  # noqa: F401
    from evc_amd.config import default_config
    from evc_amd.scorenet import build_score_network
    from evc_amd.unet_ddpm import UNetDDPM
    cfg = default_config(32, 32, 32)
    with pytest.raises(NotImplementedError, match="batch_invariant"):
        UNetDDPM(cfg, {}, batch_invariant=True)
    cfg.model.arch = "unet"
    with pytest.raises(NotImplementedError, match="batch_invariant"):
        build_score_network(cfg, {}, batch_invariant=True)
    cfg.model.arch, cfg.model.spade = "unetmore", True
    with pytest.raises(NotImplementedError, match="batch_invariant"):
        build_score_network(cfg, {}, batch_invariant=True)
    cfg.model.spade = False
    for arch in ("unetmorepseudo3d", "unetmore3d"):
        cfg.model.arch = arch
        with pytest.raises(NotImplementedError, match="batch_invariant"):
            build_score_network(cfg, {}, batch_invariant=True)
