"""GPU tests of FVD (evc_amd/fvd.py, csrc/i3d.hip): the same-padded max-pool bit for bit, the fused stem and every end point
against the torch CPU restatement of tests/i3d_recipe.py, the logits and FVD values against the reference's
(tests/golden/i3d_fvd.npz), batching, and the CLI's fvd_<idx>.npy."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import i3d_recipe as R
from conftest import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sd():
    return R.seeded_state_dict()


@pytest.fixture(scope="module")
def net(sd):
    import evc_amd  # noqa: F401
    from evc_amd import fvd
    return fvd.I3d(sd, device="cuda:0")


def _clip(i):
    return R.clip(*golden("i3d_fvd")["clips"][i])


@pytest.mark.parametrize("kernel,stride,shape", [
    ((1, 3, 3), (1, 2, 2), (2, 15, 112, 112, 64)),
    ((1, 3, 3), (1, 2, 2), (1, 5, 57, 31, 8)),
    ((3, 3, 3), (2, 2, 2), (2, 15, 28, 28, 16)),
    ((3, 3, 3), (2, 2, 2), (1, 7, 13, 9, 4)),
    ((2, 2, 2), (2, 2, 2), (2, 8, 14, 14, 32)),
    ((2, 2, 2), (2, 2, 2), (1, 5, 7, 11, 4)),
    ((3, 3, 3), (1, 1, 1), (2, 9, 15, 13, 12)),
])
def test_maxpool3d_same_is_bit_exact(kernel, stride, shape):
    import evc_amd  # noqa: F401
    from evc_amd import lib as L
    B, T, H, W, C = shape
    x = torch.from_numpy(np.random.default_rng(5).standard_normal(shape, dtype=np.float32))   # negatives: the zero pad counts
    got = L.maxpool3d_same_nthwc(x.view(B * T, H, W, C).cuda(), T, kernel, stride).cpu()
    xc = x.permute(0, 4, 1, 2, 3)
    ref = F.max_pool3d(F.pad(xc, R.same_pad_args((T, H, W), kernel, stride)), kernel, stride).permute(0, 2, 3, 4, 1)
    assert torch.equal(got.view(ref.shape), ref.contiguous())


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_fused_stem_against_torch(sd):
    """Resize (non-square: crop), scale, same padding, 7x7x7 stride 2, BN, ReLU -- with a one-frame stem workspace so that the
    patch rows are produced in chunks."""
    import evc_amd  # noqa: F401
    from evc_amd import fvd
    small = fvd.I3d(sd, device="cuda:0", stem_workspace_bytes=112 * 112 * fvd.STEM_LD * 4)
    clips = torch.stack([R.clip(21, 9, 96, 128), R.clip(22, 9, 96, 128)])
    y, To = small._stem(clips.cuda())
    x = torch.stack([R.preprocess(v.permute(1, 0, 2, 3)) for v in clips])
    ref = R._unit({k: v.float() for k, v in sd.items()}, "Conv3d_1a_7x7", x, 7, (2, 2, 2))
    assert To == 5 and _rel(y.view(2, 5, 112, 112, 64).permute(0, 4, 1, 2, 3).cpu(), ref) < 3e-5


@pytest.mark.parametrize("i", [0, 5])
def test_every_end_point_against_torch(net, sd, i):
    clip = _clip(i)
    logits, eps = net.forward(clip[None].cuda(), endpoints=True)
    ref_logits, ref_eps = R.forward(sd, clip[None])
    for name in R.END_POINTS:
        got = eps[name].permute(0, 4, 1, 2, 3).cpu()
        assert got.shape == ref_eps[name].shape, name
        assert _rel(got, ref_eps[name]) <= 3e-5, (name, _rel(got, ref_eps[name]))
    assert _rel(logits.cpu(), ref_logits) <= 3e-5
    g = golden("i3d_fvd")
    sums = g["checksums_first"] if i == 0 else g["checksums_last"]
    for k, name in enumerate(R.END_POINTS):
        c = R.checksums(eps[name].permute(0, 4, 1, 2, 3).cpu())
        assert np.allclose(c, sums[k], rtol=1e-4), name


def test_logits_against_the_reference_golden(net):
    g = golden("i3d_fvd")
    for i in range(len(g["clips"])):
        got = net(_clip(i)[None]).double().cpu().numpy()[0]
        ref = g["logits"][i]
        assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max(), i


def test_batched_equals_one_clip_at_a_time(net):
    clips = torch.stack([_clip(i) for i in range(5)])
    batched = net(clips).cpu()
    single = torch.cat([net(c[None]) for c in clips]).cpu()
    assert _rel(batched, single) <= 1e-5


def test_calculate_fvd_against_the_reference_golden(net):
    import evc_amd  # noqa: F401
    from evc_amd import fvd
    g = golden("i3d_fvd")
    a = torch.stack([_clip(i) for i in (0, 1, 2)])
    b = torch.stack([_clip(i) for i in (3, 4)])
    # the 16-frame clip is the third member of set b: features do not depend on T, so it joins through `features`
    fa = fvd.features(a, net)
    fb = np.concatenate([fvd.features(b, net), fvd.features(_clip(5)[None], net)])
    assert abs(fvd.frechet_distance(fa, fb) - float(g["fvd_set"])) <= 1e-3 * float(g["fvd_set"])
    v1, v2 = _clip(0)[None].repeat(2, 1, 1, 1, 1), _clip(1)[None].repeat(2, 1, 1, 1, 1)   # city_sender.py:575-577
    calls = []
    counting = lambda x: (calls.append(x.shape[0]), net(x))[1]                       # noqa: E731
    got = fvd.calculate_fvd(v1, v2, counting)
    assert calls == [2]                              # one pass, the repeated clips run once each
    assert abs(got - float(g["fvd_rep2"])) <= 1e-3 * float(g["fvd_rep2"])


def test_cli_writes_fvd_next_to_unchanged_outputs(tmp_path, monkeypatch, sd, capsys):
    import evc_amd  # noqa: F401
    from evc_amd import cli
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.chdir(tmp_path)
    weights = tmp_path / "i3d_seeded.pt"
    torch.save(sd, weights)

    def run(out, extra):
        cli.main(["--config", os.path.join(repo, "configs", "mine.yml"), "--synthetic", "--exp", str(tmp_path / "exp"),
                  "--data_npy", "missing.npy", "--output_path", str(out), "--start_idx", "0", "--end_idx", "0",
                  "--subsample", "2", "--q", "3", "--config_mod", "model.ngf=32 model.n_head_channels=32", "--policy", "psnr",
                  "--thresholds", "200", "-100", "--bpp-limit", "1e9"] + extra)
        return capsys.readouterr().out

    log_with = run(tmp_path / "with", ["--fvd", str(weights)])
    log_without = run(tmp_path / "without", [])
    d, d0 = tmp_path / "with" / "output_0", tmp_path / "without" / "output_0"
    env, vals = np.load(d / "fvd_0.npy"), np.load(d / "fvd_values_0.npy")
    assert vals.shape == (2,) and np.isfinite(vals).all() and (vals >= 0).all()
    assert env.shape[0] == 2 and np.isfinite(env).all()
    assert sum(line.count("FVD: ") for line in log_with.splitlines()) == 2 + 1      # two jobs + the weights line
    assert "FVD: skipped" in log_without and not list(d0.glob("fvd*"))
    for f in sorted(p.name for p in d0.iterdir()):
        if f.endswith(".npy"):
            assert (d / f).read_bytes() == (d0 / f).read_bytes(), f
    assert sorted(p.name for p in d.iterdir()) == sorted([p.name for p in d0.iterdir()] + ["fvd_0.npy", "fvd_values_0.npy"])
