"""Host-side pieces of FVD (evc_amd/fvd.py): the same-padding tables of every I3D layer, BatchNorm folding, the state-dict
loader and the Frechet distance against the reference's values (tests/golden/i3d_fvd.npz)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import i3d_recipe as R
from conftest import golden


def _fvd():
    import evc_amd  # noqa: F401
    from evc_amd import fvd
    return fvd


@pytest.mark.parametrize("T", [16, 30])
def test_same_padding_tables_of_every_layer(T):
    """Walk the layer sequence at T x 224 x 224: every pad pair follows compute_pad (pytorch_i3d.py) and the shapes follow the
    layer table (15 x 112^2 after the stem ... 4 x 7^2 before the head for 30 frames)."""
    fvd = _fvd()
    from evc_amd import lib as L
    shape = [T, 224, 224]
    seen = []

    def step(kernel, stride):
        out = []
        for n, k, s in zip(shape, kernel, stride):
            f, b = L.same_pad(n, k, s)
            p = R.compute_pad(n, k, s)
            assert (f, b) == (p // 2, p - p // 2) and b - f in (0, 1)
            assert (n + f + b - k) // s + 1 == math.ceil(n / s)
            out.append((n + f + b - k) // s + 1)
        return out

    for e in fvd.LAYERS:
        if e[0] == "unit":
            shape = step((e[4],) * 3, (2,) * 3 if e[4] == 7 else (1,) * 3)
        elif e[0] == "pool":
            shape = step(e[2], e[3])
        else:
            for k, s in (((1, 1, 1), (1, 1, 1)), ((3, 3, 3), (1, 1, 1))):   # branch units and the b3 pool keep the shape
                assert step(k, s) == shape
        seen.append((e[1], tuple(shape)))
    if T == 30:
        table = dict(seen)
        assert table["Conv3d_1a_7x7"] == (15, 112, 112) and table["MaxPool3d_2a_3x3"] == (15, 56, 56)
        assert table["MaxPool3d_3a_3x3"] == (15, 28, 28) and table["MaxPool3d_4a_3x3"] == (8, 14, 14)
        assert table["MaxPool3d_5a_2x2"] == (4, 7, 7) and table["Mixed_5c"] == (4, 7, 7)
    else:
        assert dict(seen)["Mixed_5c"] == (2, 7, 7)
    # the asymmetric case: 7 over 224 at stride 2 pads 2 in front, 3 behind
    assert L.same_pad(224, 7, 2) == (2, 3) and L.same_pad(15, 3, 2) == (1, 1) and L.same_pad(112, 3, 2) == (0, 1)


def test_bn_folding_equals_conv_then_bn_in_fp64():
    fvd = _fvd()
    sd = {k: v.double() for k, v in R.seeded_state_dict().items()}
    name = "Mixed_4c.b2b"                                          # a 3x3x3 unit with a 24-channel input
    w, b = fvd.fold_unit(sd, name)
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((1, 24, 4, 6, 6)))
    ref = F.batch_norm(F.conv3d(x, sd[f"{name}.conv3d.weight"]), sd[f"{name}.bn.running_mean"], sd[f"{name}.bn.running_var"],
                       sd[f"{name}.bn.weight"], sd[f"{name}.bn.bias"], False, 0.0, 1e-5)
    got = F.conv3d(x, w, b)
    assert w.dtype == torch.float64 and float((got - ref).abs().max()) < 1e-12 * float(ref.abs().max())
    wl, bl = fvd.fold_unit(sd, "logits")                          # bias, no BatchNorm
    assert torch.equal(wl, sd["logits.conv3d.weight"]) and torch.equal(bl, sd["logits.conv3d.bias"])


def test_loader_accepts_plain_and_dataparallel_keys(tmp_path):
    fvd = _fvd()
    sd = R.seeded_state_dict()
    plain, wrapped = tmp_path / "plain.pt", tmp_path / "wrapped.pt"
    torch.save(sd, plain)
    torch.save({"module." + k: v for k, v in sd.items()}, wrapped)
    a, b = fvd.normalise_keys(fvd.load_state_dict(str(plain))), fvd.normalise_keys(fvd.load_state_dict(str(wrapped)))
    assert set(a) == set(b) == set(sd)
    for name in fvd.unit_shapes():
        wa, ba = fvd.fold_unit(a, name)
        wb, bb = fvd.fold_unit(b, name)
        assert torch.equal(wa, wb) and torch.equal(ba, bb)


def test_loader_refuses_torchscript(tmp_path):
    fvd = _fvd()
    path = tmp_path / "i3d_torchscript.pt"
    torch.jit.script(torch.nn.Linear(2, 2)).save(str(path))
    with pytest.raises(ValueError, match="TorchScript"):
        fvd.load_state_dict(str(path))


def test_wrong_shape_is_refused_naming_the_key():
    fvd = _fvd()
    sd = R.seeded_state_dict()
    sd["Mixed_4b.b1b.conv3d.weight"] = torch.zeros(208, 96, 3, 3, 1)
    with pytest.raises(ValueError, match=r"Mixed_4b\.b1b\.conv3d\.weight"):
        fvd.fold_unit(sd, "Mixed_4b.b1b")
    del sd["Mixed_3b.b0.bn.running_var"]
    with pytest.raises(KeyError, match=r"Mixed_3b\.b0\.bn\.running_var"):
        fvd.fold_unit(sd, "Mixed_3b.b0")


def test_unit_table_matches_the_recipe():
    fvd = _fvd()
    mine = {n: (ci, co, k, bn) for n, ci, co, k, _, bn in R.units()}
    assert fvd.unit_shapes() == mine


def test_preprocess_geometry():
    fvd = _fvd()
    assert fvd.preprocess_geometry(128, 128) == (224, 224)
    assert fvd.preprocess_geometry(96, 128) == (224, math.ceil(128 * 224 / 96))
    assert fvd.preprocess_geometry(160, 120) == (math.ceil(160 * 224 / 120), 224)


def test_frechet_distance_against_the_reference():
    fvd = _fvd()
    g = golden("i3d_fvd")
    f = g["logits"]
    got = fvd.frechet_distance(f[g["set_a"]], f[g["set_b"]])
    assert abs(got - float(g["fvd_set"])) <= 1e-9 * abs(float(g["fvd_set"]))
    rep = fvd.frechet_distance(np.stack([f[0], f[0]]), np.stack([f[1], f[1]]))
    assert abs(rep - float(g["fvd_rep2"])) <= 1e-9 * float(g["fvd_rep2"])


def test_repeat2_fvd_is_the_squared_mean_difference():
    """Two identical samples have zero covariance: the reference's per-job number is ||mu_ge - mu_gt||^2."""
    fvd = _fvd()
    rng = np.random.default_rng(7)
    a, b = rng.standard_normal(400), rng.standard_normal(400)
    got = fvd.frechet_distance(np.stack([a, a]), np.stack([b, b]))
    assert abs(got - float(np.square(a - b).sum())) <= 1e-12 * got


def test_distance_of_a_set_to_itself_is_zero():
    fvd = _fvd()
    x = np.random.default_rng(8).standard_normal((5, 400))
    assert abs(fvd.frechet_distance(x, x)) < 1e-6 * float(np.trace(np.cov(x, rowvar=False)))


def test_cli_flag_and_weight_discovery(tmp_path, monkeypatch):
    import evc_amd  # noqa: F401
    from evc_amd import cli
    fvd = _fvd()
    monkeypatch.chdir(tmp_path)
    assert cli.build_parser().parse_args(["--fvd", "x.pt"]).fvd == "x.pt"
    assert fvd.find_i3d_weights() is None
    logs = []
    assert cli.resolve_fvd(cli.build_parser().parse_args([]), log=logs.append) is None
    assert len(logs) == 1 and logs[0].startswith("FVD: skipped")
    d = tmp_path / "fvd_utils" / "models" / "fvd"
    d.mkdir(parents=True)
    (d / "i3d_pretrained_400.pt").write_bytes(b"")
    assert fvd.find_i3d_weights() == "./fvd_utils/models/fvd/i3d_pretrained_400.pt"
