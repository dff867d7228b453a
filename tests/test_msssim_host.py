"""Host-side tests of MS-SSIM (evc_amd/msssim.py, csrc/msssim.hip): the float64 yardstick of tests/msssim_ref.py against itself
in its two forms and against closed forms, the pooling against torch's, ``combine`` and ``to_db``, the refusals, the flags, the
build list and the C ABI table, and ``Measurer`` / ``Collector`` with a stub backend.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import msssim_ref as M

import evc_amd  # noqa: F401
from evc_amd import build, cli, lib, msssim, receiver, report as R, ssim, stitch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(5, s, k) for s in M.SHAPES5 for k in M.KINDS] + [(n, s, k) for n, s in M.SMALL for k in M.KINDS]


@pytest.mark.parametrize("levels,shape,kind", CASES)
def test_the_two_forms_of_the_yardstick_agree(levels, shape, kind):
    a, b, full = M.case(kind, shape, levels)
    sep = M.ms_ssim_levels(a, b, levels, "separable")
    w = M.WEIGHTS[:levels]
    worst_l, worst_v = float(np.abs(full - sep).max()), float(np.abs(M.combine(full, w) - M.combine(sep, w)).max())
    print(f"{kind} {shape} L={levels}: |full - separable| levels {worst_l:.3e}, values {worst_v:.3e}")
    assert worst_l <= 1e-12 and worst_v <= 1e-12


@pytest.mark.parametrize("form", list(M.FORMS))
def test_identical_planes_give_exactly_one(form):
    for kind in M.KINDS:
        a, _, _ = M.case(kind, (162, 177))
        lv = M.ms_ssim_levels(a[:1], a[:1], 5, form)
        assert (lv == 1.0).all() and (M.combine(lv) == 1.0).all(), kind


@pytest.mark.parametrize("shape", [(176, 176), (192, 352)])
@pytest.mark.parametrize("p,q", [(0.0, 1.0), (0.3, 0.6), (0.5, 0.5), (0.123, 0.987)])
def test_constant_planes_on_even_pyramids_match_the_closed_form(shape, p, q):
    """Every level is the constant pair again (no zero padding on an even pyramid): sigma = 0, cs = 1, and the value is the
    last level's luminance term to the last weight."""
    a, b = np.full(shape, p, dtype=np.float32), np.full(shape, q, dtype=np.float32)
    x, y = float(a[0, 0]), float(b[0, 0])
    want = ((2 * x * y + M.C1) / (x * x + y * y + M.C1)) ** M.WEIGHTS[4]
    for form in M.FORMS:
        lv = M.levels_plane(a, b, 5, form)
        print(f"{shape} ({p}, {q}) {form}: |cs - 1| = {np.abs(lv[:, 1] - 1).max():.3e}, |value - closed form| = {abs(M.combine(lv) - want):.3e}")
        assert np.abs(lv[:, 1] - 1).max() <= 1e-12 and abs(M.combine(lv) - want) <= 1e-12


def test_pooling_of_an_odd_plane_equals_torchs():
    x = np.random.default_rng(5).random((5, 7), dtype=np.float32).astype(np.float64)     # widened floats: the four-term sums are
    want = F.avg_pool2d(torch.from_numpy(x)[None, None], kernel_size=2, padding=(1, 1))[0, 0].numpy()      # exact in any order
    got = M.pool_zero_pad(x)
    assert got.shape == want.shape == (3, 4) and np.array_equal(got, want)
    assert got[0, 0] == 0.25 * x[0, 0] and got[0, 1] == 0.25 * (x[0, 1] + x[0, 2]) and got[1, 0] == 0.25 * (x[1, 0] + x[2, 0])
    assert got[2, 3] == 0.25 * ((x[3, 5] + x[3, 6]) + (x[4, 5] + x[4, 6]))             # the far side needs no padding
    for shape in ((6, 7), (5, 8), (4, 6)):
        y = np.random.default_rng(6).random(shape)
        assert M.pool_zero_pad(y).shape == ((shape[0] + 1) // 2, (shape[1] + 1) // 2)
        assert np.abs(M.pool_zero_pad(y) - M.pool_torch(y)).max() <= 1e-15


def test_combine():
    lv = np.ones((4, 5, 2))
    lv[0, :, 0] = 0.5                                 # ssim of levels 0 .. 3 is not read: only the last one's counts
    lv[1, 2, 1], lv[2, 4, 0], lv[3, 1, 1] = -0.25, -1e-3, np.nan
    got = msssim.combine(lv)
    assert got.shape == (4,) and got[0] == 0.5 ** msssim.WEIGHTS[4]
    assert got[1] == 0.0 and got[2] == 0.0 and np.isnan(got[3])                       # relu: exact 0; NaN kept
    both = lv[3].copy()
    both[0, 1] = -1.0                                 # NaN times a zero factor stays NaN, as torch.prod has it
    assert np.isnan(msssim.combine(both))
    f = np.array([0.9, 0.8, 0.7, 0.6, 0.5])
    lv = np.stack([np.concatenate([np.zeros(4), f[4:]]), np.concatenate([f[:4], np.zeros(1)])], axis=-1)
    assert abs(msssim.combine(lv) - np.prod(f ** np.array(msssim.WEIGHTS))) <= 1e-15
    assert np.array_equal(msssim.combine(lv[None]), M.combine(lv[None]))
    assert msssim.combine(lv[:3], msssim.WEIGHTS[:3]) == M.combine(lv[:3], msssim.WEIGHTS[:3])
    with pytest.raises(ValueError):
        msssim.combine(lv[:4])
    assert msssim.WEIGHTS == M.WEIGHTS == (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
    assert (msssim.C1, msssim.C2) == (ssim.C1, ssim.C2) == (1e-4, 9e-4)


def test_to_db():
    assert msssim.to_db(0.9) == -10 * np.log10(1 - 0.9) and abs(msssim.to_db(0.99) - 20.0) <= 1e-12
    assert msssim.to_db(0.0) == 0.0 and msssim.to_db(1.0) == np.inf
    assert np.array_equal(msssim.to_db(np.array([0.0, 0.9])), [0.0, msssim.to_db(0.9)])


def test_shapes_and_sizes_are_refused_before_the_device():
    assert [msssim.min_side(n) for n in (1, 2, 3, 5)] == [10, 20, 40, 160] and msssim.min_side() == 160
    z = lambda *s: np.zeros(s, dtype=np.float32)  # noqa: E731
    for a, b in ((z(3, 160, 200), z(3, 160, 200)), (z(200, 160), z(200, 160)), (z(3, 161, 161), z(3, 161, 162)), (z(161), z(161))):
        with pytest.raises(ValueError):
            msssim.ms_ssim_levels(a, b)
    with pytest.raises(ValueError, match=r"larger than 160 .*\(3, 128, 128\)"):
        msssim.ms_ssim_planes(z(3, 128, 128), z(3, 128, 128))
    with pytest.raises(ValueError, match="larger than 20"):
        msssim.ms_ssim_levels(z(20, 21), z(20, 21), levels=2)
    for levels in (0, 9):
        with pytest.raises(ValueError):
            msssim.ms_ssim_levels(z(161, 161), z(161, 161), levels=levels)
    with pytest.raises(ValueError):
        msssim.ms_ssim_frames(z(2, 2, 161, 161), z(2, 2, 161, 161))
    empty = msssim.ms_ssim_levels(z(0, 3, 161, 161), z(0, 3, 161, 161))           # nothing to launch: no device either
    assert empty.shape == (0, 3, 5, 2) and empty.dtype == np.float64
    assert msssim.size_message(161, 200) is None
    text = msssim.size_message(128, 144)
    assert "144x128" in text and "> 160" in text and "--yuv-fit joint" in text and "city_stitch.py --ms-ssim" in text


def test_flags_parse_and_default_to_off():
    assert cli.build_parser().parse_args([]).ms_ssim is False
    assert cli.build_parser().parse_args(["--ms-ssim"]).ms_ssim is True
    assert receiver.build_parser().parse_args(["--bitstream-dir", "d"]).ms_ssim is False
    assert receiver.build_parser().parse_args(["--bitstream-dir", "d", "--ms-ssim"]).ms_ssim is True
    need = ["--tiles", "t.json", "--decoded", "d"]
    assert stitch.build_parser().parse_args(need).ms_ssim is False
    assert stitch.build_parser().parse_args(need + ["--ms-ssim"]).ms_ssim is True
    assert "ms_ssim" in cli.OPT_IN_FLAGS          # args.yml of a run without the flag is what it was


def tiles_of(h, w):
    return -(-(h - 10) // 16) * -(-(w - 10) // 16)


def documented_bytes(N, H, W, levels):
    sizes = [(H, W)]
    for _ in range(levels - 1):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    return 8 * N * (2 * sum(h * w for h, w in sizes[1:]) + 2 * sum(tiles_of(h, w) for h, w in sizes))


def test_kernel_is_built_declared_and_bound():
    assert "msssim.hip" in build.HIP_SOURCES and os.path.isfile(os.path.join(build.CSRC, "msssim.hip"))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "evc_hip.h")).read(), flags=re.S)
    for name in ("evc_msssim_workspace_bytes", "evc_msssim_levels_f32"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in lib.HIP_SYMBOLS
    so = lib.hip_lib(require_device=False)
    ws = so.evc_msssim_workspace_bytes
    # 161 -> 81 -> 41 -> 21 -> 11: pyramids 81^2 + 41^2 + 21^2 + 11^2, tiles 100 + 25 + 4 + 1 + 1
    assert documented_bytes(1, 161, 161, 5) == 8 * (2 * (6561 + 1681 + 441 + 121) + 2 * 131)
    assert ws(1, 161, 161, 5) == documented_bytes(1, 161, 161, 5)
    assert ws(90, 288, 352, 5) == documented_bytes(90, 288, 352, 5)
    assert ws(7, 21, 23, 2) == documented_bytes(7, 21, 23, 2) and ws(3, 11, 12, 1) == 8 * 3 * 2
    assert ws(0, 288, 352, 5) == 0
    assert ws(-1, 288, 352, 5) < 0 and ws(1, 288, 352, 0) < 0 and ws(1, 288, 352, 9) < 0
    assert ws(1, 160, 352, 5) < 0 and ws(1, 352, 160, 5) < 0 and ws(1, 20, 21, 2) < 0 and ws(1, 10, 11, 1) < 0
    # the launch export refuses before any launch (no device is needed to hear it)
    f = so.evc_msssim_levels_f32
    none = (None, ssim.C1, ssim.C2, None, None, None)
    assert f(None, None, 1, 160, 352, 5, *none) < 0 and f(None, None, 1, 352, 160, 5, *none) < 0
    assert f(None, None, -1, 288, 352, 5, *none) < 0
    assert f(None, None, 1, 288, 352, 0, *none) < 0 and f(None, None, 1, 4000, 4000, 9, *none) < 0
    assert f(None, None, 1, 288, 352, 5, *none) < 0               # null pointers with N > 0
    assert f(None, None, 0, 288, 352, 5, *none) == 0              # N == 0: EVC_OK with null pointers
    assert f(None, None, 0, 160, 352, 5, *none) < 0               # ... for a size it takes


# ---- Measurer / Collector with a stub backend ------------------------------------------------------------------------

class Stub:
    def __init__(self):
        self.rng, self.log, self.pairs = np.random.default_rng(9), {}, 0

    def _out(self, name, n):
        self.log.setdefault(name, []).append(self.rng.random(n))
        return self.log[name][-1]

    def ssim_frames(self, x, gt):
        return self._out("ssim", len(x))

    def ms_ssim_frames(self, x, gt):
        assert x.dtype == gt.dtype == torch.float32 and x.is_contiguous() and gt.is_contiguous() and x.shape == gt.shape
        return self._out("ms_ssim", len(x))

    def yuv_metric_clips(self, x, gt):
        self.pairs += 1
        return ("pair", self.pairs)

    def psnr_yuv(self, x, gt, clips=None):
        return 30 + self._out("psnr_yuv", len(x))

    def ssim_yuv(self, x, gt, clips=None):
        return self._out("ssim_yuv", len(x))

    def ms_ssim_yuv(self, x, gt, clips=None):
        assert clips == ("pair", self.pairs)              # the pair psnr_yuv and ssim_yuv were handed
        return self._out("ms_ssim_yuv", len(x))


def frames(stem):
    return {f"{stem}_0.npy", f"{stem}_frames_0.npy"}


@pytest.mark.parametrize("flags,extra", [
    (dict(), set()),
    (dict(ssim=True, yuv=True), frames("ssim") | frames("psnr_yuv") | frames("ssim_yuv")),
    (dict(ms_ssim=True), frames("ms_ssim")),
    (dict(ms_ssim=True, yuv=True), frames("ms_ssim") | frames("psnr_yuv") | frames("ms_ssim_yuv")),
    (dict(ssim=True, ms_ssim=True, yuv=True), frames("ssim") | frames("ms_ssim") | frames("psnr_yuv") | frames("ssim_yuv") | frames("ms_ssim_yuv")),
], ids=["none", "ssim+yuv", "ms", "ms+yuv", "all"])
def test_measurer_and_collector_write_the_new_files_only_when_asked(flags, extra, tmp_path):
    s = Stub()
    m = R.Measurer(backend=s, **flags)
    c = R.Collector()
    rng = np.random.default_rng(1)
    gt = rng.random((30, 3, 8, 8)).astype(np.float32)
    bpps = [0.1, 0.3, 0.2]
    for bpp, v in zip(bpps, m.measure_jobs([(0, rng.random((30, 3, 8, 8)).astype(np.float32), gt) for _ in bpps])):
        assert ("ms_ssim" in v) == bool(flags.get("ms_ssim")) and ("ms_ssim_yuv" in v) == bool(flags.get("ms_ssim") and flags.get("yuv"))
        c.add(0, bpp, v)
    c.save(str(tmp_path))
    root = tmp_path / "output_0"
    assert set(os.listdir(root)) == {"bpp_0.npy"} | frames("psnr") | extra
    assert ("ms_ssim" in s.log) == bool(flags.get("ms_ssim"))
    from evc_amd.policy import rd_envelope
    for name in ("ms_ssim", "ms_ssim_yuv"):
        if frames(name) <= extra:
            got = np.load(root / f"{name}_frames_0.npy")
            assert got.shape == (3, 30) and got.dtype == np.float64 and np.array_equal(got, np.asarray(s.log[name]))
            assert np.array_equal(np.load(root / f"{name}_0.npy"), rd_envelope(bpps, got.mean(1), True))


def test_printed_lines():
    v = {"psnr": [30.0] * 30, "ssim": np.full(30, 0.9), "ms_ssim": np.full(30, 0.99), "lpips": np.full(30, 0.125)}
    d = [1, 1] + [0] * 28
    lines = R.sender_lines(v, d, 0.0061, "vgg")
    assert lines[1:] == ["SSIM: 0.90000", "MS-SSIM: 0.99000 (20.00 dB)", "LPIPS(vgg): 0.12500"]
    without = {k: x for k, x in v.items() if k != "ms_ssim"}
    assert R.sender_lines(without, d, 0.0061, "vgg") == lines[:2] + lines[3:]
    assert R.quality_text(v, "vgg") == " PSNR 30.000 SSIM 0.90000 MS-SSIM 0.99000 LPIPS(vgg) 0.12500"
    assert R.quality_text(without, "vgg") == " PSNR 30.000 SSIM 0.90000 LPIPS(vgg) 0.12500"
    assert R.quality_text({"psnr": [30.0], "ms_ssim": [0.5]}) == " PSNR 30.000 MS-SSIM 0.50000"
    assert R.stitcher_line("s", 200, 176, 6, {"psnr": [30.0] * 30, "ms_ssim": np.full(30, 0.75)}) == "s: 200x176, 6 tiles PSNR 30.000 MS-SSIM 0.75000"
    assert ("ms_ssim", "ms_ssim", "frames", True) in R.METRICS and ("ms_ssim_yuv", "ms_ssim_yuv", "frames", True) in R.METRICS


def test_small_frames_end_the_run_with_the_size_message():
    from types import SimpleNamespace
    R.check_ms_ssim_size(SimpleNamespace(ms_ssim=False), 128, 128)
    R.check_ms_ssim_size(SimpleNamespace(ms_ssim=True), 176, 192)
    R.check_ms_ssim_size(SimpleNamespace(), 128, 128)
    with pytest.raises(SystemExit) as e:
        R.check_ms_ssim_size(SimpleNamespace(ms_ssim=True), 128, 128)
    assert "128x128" in str(e.value) and "> 160" in str(e.value) and "--yuv-fit joint" in str(e.value)
