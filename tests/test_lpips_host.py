"""Host-side tests of the LPIPS family (evc_amd/lpips.py ``Lpips``, csrc/lpips.hip): the torch restatement of tests/lpips_ref.py
(tap shapes with ceil-mode and odd sizes, d(x, x) = 0), the trained linear layers under tests/golden/, the C ABI table and the
argument checks of the new exports, the flags, and ``load_metric``'s old spec forms.  No GPU."""
import os
import re
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import lpips_ref as R
from conftest import golden

import evc_amd  # noqa: F401
from evc_amd import build, cli, lib, policy, receiver

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference"
NEW_EXPORTS = ("evc_maxpool2d_nhwc_f32", "evc_lpips_map_f32", "evc_lpips_map_mean_f32", "evc_lpips_upsample_add_f32")


def _sd(net, seed=3):
    return R.seeded_state_dict(net, seed, golden(f"lpips_{net}_lin"))


@pytest.mark.parametrize("net,size,taps", [
    ("squeeze", (34, 34), [(16, 16), (8, 8), (4, 4), (2, 2), (2, 2), (2, 2), (2, 2)]),
    ("squeeze", (35, 21), [(17, 10), (8, 5), (4, 2), (2, 1), (2, 1), (2, 1), (2, 1)]),       # ceil mode: 10 -> 5, 5 -> 2, 2 -> 1
    ("squeeze", (17, 17), [(8, 8), (4, 4), (2, 2), (1, 1), (1, 1), (1, 1), (1, 1)]),
    ("vgg", (40, 24), [(40, 24), (20, 12), (10, 6), (5, 3), (2, 1)]),
    ("vgg", (16, 16), [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]),
])
def test_tap_shapes_of_the_restatement_and_the_host_size_rule(net, size, taps):
    from evc_amd import lpips as LP
    x = R.pairs(1, 1, *size)[0]
    got = R.features(net, _sd(net), x)
    assert [tuple(t.shape[2:]) for t in got] == taps
    assert [t.shape[1] for t in got] == list(R.CHANNELS[net]) == list(LP.CHANNELS[net])
    # the output-size rule the host allocates by (lib.pool_out_size) is torch's
    for s in range(1, 41):
        for k, stride, ceil in ((2, 2, False), (3, 2, True), (3, 2, False)):
            want = torch.nn.functional.max_pool2d(torch.zeros(1, 1, s, 5), (k, 1), (stride, 1), ceil_mode=ceil).shape[2] \
                if s >= (k - stride + 1 if ceil else k) else None
            if want is None:
                with pytest.raises(ValueError):
                    lib.pool_out_size(s, k, stride, ceil)
            else:
                assert lib.pool_out_size(s, k, stride, ceil) == want, (s, k, stride, ceil)


@pytest.mark.parametrize("net", R.NETS)
def test_distance_of_an_image_to_itself_is_zero_and_the_key_spellings_agree(net):
    sd = _sd(net)
    a, b = R.pairs(2, 2, 35, 35)
    assert float(R.distance(net, sd, a.double(), a.double()).abs().max()) == 0.0
    assert float(R.spatial_map(net, sd, a.double(), a.double()).abs().max()) == 0.0
    d = R.distance(net, sd, a.double(), b.double())
    assert (d > 1e-5).all()
    # the mean of the up-sampled map is another number than the spatially averaged distance
    m = R.spatial_map(net, sd, a.double(), b.double()).mean((1, 2))
    assert (m > 1e-5).all() and not torch.equal(m, d)
    saved = R.as_saved_module(net, sd)
    assert len(saved) == len(sd) and not set(saved) & set(sd)
    assert all(k.startswith(("net.slice", "lins.")) for k in saved)


@pytest.mark.parametrize("net,count", [("vgg", 1472), ("squeeze", 2240)])
def test_lin_fixtures_hold_the_layers_of_each_network(net, count):
    lin = golden(f"lpips_{net}_lin")
    assert sorted(lin.files) == sorted(f"lin{i}" for i in range(len(R.CHANNELS[net])))
    assert [lin[f"lin{i}"].size for i in range(len(R.CHANNELS[net]))] == list(R.CHANNELS[net])
    assert sum(lin[k].size for k in lin.files) == count and all(lin[k].dtype == np.float32 for k in lin.files)


@pytest.mark.parametrize("net", ["vgg", "squeeze"])
def test_lin_fixtures_equal_the_references_files_where_it_is_present(net):
    lin = golden(f"lpips_{net}_lin")
    path = os.path.join(REFERENCE, "weights", "v0.1", f"{net}.pth")
    if not os.path.isfile(path):
        pytest.skip("the reference tree is not present")
    sd = torch.load(path, map_location="cpu", weights_only=True)
    for i in range(len(R.CHANNELS[net])):
        np.testing.assert_array_equal(lin[f"lin{i}"], sd[f"lin{i}.model.1.weight"].reshape(-1).numpy())


def test_squeeze_and_alex_layers_are_non_negative():
    for net in ("squeeze", "alex"):
        lin = golden(f"lpips_{net}_lin")
        assert all((lin[k] >= 0).all() for k in lin.files), net


def test_new_exports_are_declared_bound_and_built():
    header = open(os.path.join(REPO, "include", "evc_hip.h")).read()
    so = lib.hip_lib(require_device=False)
    assert "lpips.hip" in build.HIP_SOURCES
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, header) and name in lib.HIP_SYMBOLS
        assert getattr(so, name) is not None
    assert "nn.Upsample(size" in header and "scale_factor" in header          # the two up-sampling forms are discussed


def test_argument_checks_return_einval_before_any_launch():
    """No device is needed: every refusal comes back before a launch."""
    so = lib.hip_lib(require_device=False)
    d, odd = c_void_p(4096), c_void_p(4100)
    pool, lmap, mean, up = (getattr(so, n) for n in NEW_EXPORTS)
    EINVAL = -1
    for args in ((None, d, 1, 4, 4, 8, 2, 2, 0), (d, None, 1, 4, 4, 8, 2, 2, 0), (d, d, 0, 4, 4, 8, 2, 2, 0), (d, d, 1, 4, 4, 6, 2, 2, 0),
                 (d, d, 1, 4, 4, 8, 4, 2, 0), (d, d, 1, 4, 4, 8, 1, 1, 0), (d, d, 1, 4, 4, 8, 2, 0, 0), (d, d, 1, 4, 4, 8, 2, 2, 2),
                 (d, d, 1, 1, 4, 8, 2, 2, 0), (d, d, 1, 4, 2, 8, 3, 2, 0), (d, d, 1, 1, 4, 8, 3, 2, 1), (d, d, 1, 0, 4, 8, 2, 2, 1)):
        assert pool(*args, None) == EINVAL, args
    for args in ((None, d, d, d, 1, 1, 64), (d, None, d, d, 1, 1, 64), (d, d, None, d, 1, 1, 64), (d, d, d, None, 1, 1, 64),
                 (d, d, d, d, 0, 1, 64), (d, d, d, d, 1, 0, 64), (d, d, d, d, 1, 1, 0), (d, d, d, d, 1, 1, 48), (d, d, d, d, 1, 1, 96),
                 (d, d, d, d, 1, 1, 576), (odd, d, d, d, 1, 1, 64), (d, odd, d, d, 1, 1, 64), (d, d, odd, d, 1, 1, 64)):
        assert lmap(*args, None) == EINVAL, args
    for args in ((None, d, 1, 4, 0), (d, None, 1, 4, 0), (d, d, 0, 4, 0), (d, d, 1, 0, 0)):
        assert mean(*args, None) == EINVAL, args
    for args in ((None, d, 1, 2, 2, 4, 4, 0), (d, None, 1, 2, 2, 4, 4, 0), (d, d, 0, 2, 2, 4, 4, 0), (d, d, 1, 0, 2, 4, 4, 0),
                 (d, d, 1, 2, 0, 4, 4, 0), (d, d, 1, 2, 2, 0, 4, 0), (d, d, 1, 2, 2, 4, 0, 0)):
        assert up(*args, None) == EINVAL, args


def test_the_new_flags_parse_and_stay_out_of_args_yml_by_default():
    a = cli.build_parser().parse_args([])
    assert a.lpips is None and a.lpips_net == "alex"
    a = cli.build_parser().parse_args(["--policy", "psnr", "--lpips", "vgg:vgg16.pth,vgg.pth", "--lpips-net", "squeeze"])
    assert a.lpips == "vgg:vgg16.pth,vgg.pth" and a.lpips_net == "squeeze"
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--lpips-net", "resnet"])
    assert {"lpips", "lpips_net"} <= set(cli.OPT_IN_FLAGS)
    r = receiver.build_parser().parse_args(["--bitstream-dir", "x", "--lpips", "squeeze:one.pth"])
    assert r.lpips == "squeeze:one.pth" and receiver.build_parser().parse_args(["--bitstream-dir", "x"]).lpips is None


def test_spec_grammar_and_a_missing_file_is_named(tmp_path):
    from evc_amd import lpips as LP
    back, lin = tmp_path / "vgg16.pth", tmp_path / "vgg.pth"
    back.write_bytes(b"")
    lin.write_bytes(b"")
    assert LP.parse_spec(f"vgg:{back},{lin}") == ("vgg", [str(back), str(lin)])
    assert LP.parse_spec(f"squeeze:{back}") == ("squeeze", [str(back)])
    assert LP.parse_spec(f"{back},{lin}", "alex") == ("alex", [str(back), str(lin)])
    missing = tmp_path / "nowhere" / "squeeze.pth"
    for call in (lambda: LP.parse_spec(f"squeeze:{back},{missing}"),
                 lambda: cli.main(["--synthetic", "--policy", "psnr", "--lpips", f"squeeze:{back},{missing}"]),
                 lambda: receiver.main(["--bitstream-dir", str(tmp_path), "--lpips", f"squeeze:{missing}"])):
        with pytest.raises(FileNotFoundError, match=re.escape(str(missing))):
            call()
    with pytest.raises(ValueError, match="alex, vgg, squeeze"):
        LP.parse_spec(f"{back},{lin}")                     # --lpips needs its network named
    with pytest.raises(ValueError, match="resnet"):
        LP.parse_spec(f"{back}", "resnet")


def test_load_metric_keeps_its_old_spec_forms(tmp_path):
    assert isinstance(policy.load_metric("psnr"), policy.PsnrMetric)
    assert isinstance(policy.load_metric("psnr", None, "cuda", net="vgg"), policy.PsnrMetric)
    m = policy.load_metric("lpips", "torch.nn.functional:l1_loss")
    assert isinstance(m, policy.CallableMetric) and m.name == "torch.nn.functional:l1_loss"
    m = policy.load_metric("lpips", "torch.nn.functional:l1_loss", net="squeeze")          # a callable is no weight file
    assert m.name == "torch.nn.functional:l1_loss"
    with pytest.raises(RuntimeError, match="lpips"):
        policy.load_metric("lpips", None)
    with pytest.raises(ValueError, match="unknown policy metric"):
        policy.load_metric("ssim")
    with pytest.raises(FileNotFoundError, match="gone.pth"):
        policy.load_metric("lpips", f"file:{tmp_path / 'gone.pth'}", "cuda", net="vgg")
    import inspect
    assert list(inspect.signature(policy.load_metric).parameters) == ["policy", "spec", "device", "net"]
