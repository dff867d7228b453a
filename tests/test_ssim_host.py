"""Host-side tests of SSIM (evc_amd/ssim.py, csrc/ssim.hip): the float64 yardstick of tests/ssim_ref.py against itself in two
summation orders and against closed forms, the window taps, the reference's result dict, the flag, the build list and the
C ABI table.  No GPU."""
import os
import re

import numpy as np
import pytest

import ssim_ref as R

import evc_amd  # noqa: F401
from evc_amd import build, cli, lib, receiver, ssim

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(k, s) for s in R.SHAPES for k in R.KINDS]


@pytest.mark.parametrize("kind,shape", CASES)
def test_the_two_forms_of_the_yardstick_agree(kind, shape):
    a, b = R.content(kind, shape)
    full, sep = R.ssim_planes(a, b, R.filter_full), R.ssim_planes(a, b, R.filter_separable)
    worst = float(np.abs(full - sep).max())
    print(f"{kind} {shape}: |121-tap - separable| = {worst:.3e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("filt", [R.filter_full, R.filter_separable])
def test_identical_inputs_give_exactly_one(filt):
    for kind in R.KINDS:
        a, _ = R.content(kind, (34, 70))
        assert (R.ssim_planes(a, a, filt) == 1.0).all(), kind


@pytest.mark.parametrize("c1,c2", [(0.0, 1.0), (0.3, 0.6), (0.5, 0.5), (0.123, 0.987), (1.0, 1.0)])
def test_constant_planes_match_the_closed_form(c1, c2):
    """mu = c, sigma = 0: SSIM = (2 c1 c2 + C1) / (c1^2 + c2^2 + C1)."""
    a, b = np.full((12, 17), c1, dtype=np.float32), np.full((12, 17), c2, dtype=np.float32)
    x, y = float(a[0, 0]), float(b[0, 0])
    want = (2 * x * y + R.C1) / (x * x + y * y + R.C1)
    for filt in (R.filter_full, R.filter_separable):
        assert abs(R.ssim_plane(a, b, filt) - want) <= 1e-12


def test_taps():
    k = ssim.gaussian_taps()
    assert k.dtype == np.float64 and k.shape == (11,)
    assert abs(k.sum() - 1.0) <= 2e-16 and np.array_equal(k, k[::-1]) and k.argmax() == 5
    assert np.array_equal(k, R.taps())
    assert abs(k[4] / k[5] - np.exp(-1 / 4.5)) <= 1e-15            # exp(-(1)^2 / (2 * 1.5^2))
    assert (ssim.C1, ssim.C2) == (0.01 ** 2, 0.03 ** 2)


def test_result_dict_from_a_hand_made_value_array():
    v = np.array([[1.0, 0.5, 0.25, 0.75, 0.0], [0.5, 0.5, 1.0, 0.25, 0.5]])
    d = ssim.ssim_result(v, 2, True, (5, 3, 34, 70))
    assert list(d) == ["ssim", "ssim_std", "ssim_per_frame", "ssim_video_setting", "ssim_video_setting_name"]
    assert list(d["ssim"]) == ["avg[:2]", "avg[:4]", "final"] and list(d["ssim_std"]) == ["std[:2]", "std[:4]", "final"]
    assert d["ssim"]["avg[:2]"] == 0.625 and d["ssim"]["avg[:4]"] == 0.59375 and d["ssim"]["final"] == 0.525
    assert d["ssim_std"]["std[:2]"] == np.std(v[:, :2]) and d["ssim_std"]["final"] == np.std(v)
    assert d["ssim_per_frame"] == 2 and d["ssim_video_setting"] == (5, 3, 34, 70)
    assert d["ssim_video_setting_name"] == "time, channel, heigth, width"
    d = ssim.ssim_result(v, 5, False, (5, 3, 34, 70))
    assert list(d["ssim"]) == ["avg[:5]"] and "final" not in d["ssim_std"]
    assert np.array_equal(ssim.channel_mean(np.array([[1.0, 0.5, 0.0], [0.25, 0.25, 0.25]])), [0.5, 0.25])


def test_shapes_are_refused_before_the_device():
    z = np.zeros
    for a, b in ((z((3, 10, 11)), z((3, 10, 11))), (z((11, 10)), z((11, 10))), (z((3, 11, 11)), z((3, 11, 12))), (z((11,)), z((11,)))):
        with pytest.raises(ValueError):
            ssim.ssim_planes(a.astype(np.float32), b.astype(np.float32))
    with pytest.raises(ValueError):
        ssim.ssim_frames(z((2, 2, 11, 11), dtype=np.float32), z((2, 2, 11, 11), dtype=np.float32))


def test_flag_parses_and_defaults_to_off():
    assert cli.build_parser().parse_args([]).ssim is False
    assert cli.build_parser().parse_args(["--ssim"]).ssim is True
    assert receiver.build_parser().parse_args(["--bitstream-dir", "d"]).ssim is False
    assert receiver.build_parser().parse_args(["--bitstream-dir", "d", "--ssim"]).ssim is True
    assert "ssim" in cli.OPT_IN_FLAGS         # args.yml of a run without the flag is what it was


def test_kernel_is_built_and_declared():
    assert "ssim.hip" in build.HIP_SOURCES and os.path.isfile(os.path.join(build.CSRC, "ssim.hip"))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "evc_hip.h")).read(), flags=re.S)
    for name in ("evc_ssim_workspace_bytes", "evc_ssim_planes_f32"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in lib.HIP_SYMBOLS
    so = lib.hip_lib(require_device=False)
    # the workspace query needs no device: one double per 16x16 tile of the valid region, negative for what is refused
    assert so.evc_ssim_workspace_bytes(90, 128, 128) == 90 * 64 * 8
    assert so.evc_ssim_workspace_bytes(1, 11, 11) == 8 and so.evc_ssim_workspace_bytes(0, 34, 70) == 0
    assert so.evc_ssim_workspace_bytes(1, 10, 128) < 0 and so.evc_ssim_workspace_bytes(1, 128, 10) < 0
    assert so.evc_ssim_workspace_bytes(-1, 128, 128) < 0
    # refusals come before any launch
    assert so.evc_ssim_planes_f32(None, None, 1, 10, 11, None, ssim.C1, ssim.C2, None, None, None) < 0
    assert so.evc_ssim_planes_f32(None, None, 1, 11, 10, None, ssim.C1, ssim.C2, None, None, None) < 0
    assert so.evc_ssim_planes_f32(None, None, -1, 11, 11, None, ssim.C1, ssim.C2, None, None, None) < 0
    assert so.evc_ssim_planes_f32(None, None, 1, 11, 11, None, ssim.C1, ssim.C2, None, None, None) < 0
    assert so.evc_ssim_planes_f32(None, None, 0, 11, 11, None, ssim.C1, ssim.C2, None, None, None) == 0
