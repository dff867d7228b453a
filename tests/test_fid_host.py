"""Host tests of FID / precision-recall (evc_amd/fid.py): the command-line flags, state-dict checking, the Frechet distance
against the reference's sqrtm form and against an eigenvalue computation, and the exports of csrc/inception.hip."""
import os
import re

import numpy as np
import pytest
import torch

import fid_recipe as R
from conftest import REPO

import evc_amd  # noqa: F401
from evc_amd import cli, fid, receiver


# ---- the flags ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("parser,base", [(cli.build_parser, []), (receiver.build_parser, ["--bitstream-dir", "bits"])])
def test_fid_flags_defaults_and_choices(parser, base, capsys):
    a = parser().parse_args(base)
    assert a.fid is None and a.fid_dims == 2048
    a = parser().parse_args(base + ["--fid", "w.pth", "--fid-dims", "64"])
    assert a.fid == "w.pth" and a.fid_dims == 64
    for d in (192, 768, 2048):
        assert parser().parse_args(base + ["--fid-dims", str(d)]).fid_dims == d
    with pytest.raises(SystemExit):
        parser().parse_args(base + ["--fid-dims", "128"])
    capsys.readouterr()
    assert {"fid", "fid_dims"} <= set(cli.OPT_IN_FLAGS)       # args.yml of a run without the flags is what it was


@pytest.mark.parametrize("main,base", [(cli.main, []), (receiver.main, ["--bitstream-dir", "bits"])])
def test_missing_weight_file_exits_naming_it(main, base, tmp_path):
    missing = str(tmp_path / "no_such_inception.pth")
    with pytest.raises(SystemExit) as e:
        main(base + ["--fid", missing])
    assert "--fid" in str(e.value) and missing in str(e.value)


# ---- the state dict -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sd():
    return R.seeded_state_dict()


def test_network_definition_matches_the_restatement(sd):
    specs = fid.conv_specs()
    assert {n: (ci, co, (kh, kw)) for n, ci, co, kh, kw in R.units()} == {n: (s[0], s[1], s[2]) for n, s in specs.items()}
    assert len(specs) == 94 and all(s[0] % 16 == 0 and s[1] % 16 == 0 for n, s in specs.items() if n != "Conv2d_1a_3x3")
    folded = fid.fold_state_dict(sd)                          # fc.* and num_batches_tracked are in sd and ignored
    assert set(folded) == set(specs)
    name = "Mixed_6b.branch7x7_2"
    w, b = folded[name]
    g = lambda k: sd[f"{name}.{k}"].double()                  # noqa: E731
    scale = g("bn.weight") / torch.sqrt(g("bn.running_var") + 1e-3)
    assert w.dtype == torch.float64 and torch.equal(w, g("conv.weight") * scale.view(-1, 1, 1, 1))
    assert torch.equal(b, g("bn.bias") - g("bn.running_mean") * scale)
    assert fid.BLOCK_INDEX_BY_DIM == {64: 0, 192: 1, 768: 2, 2048: 3}
    # 2 FLOP per MAC at 299 x 299, the figure the literature quotes for Inception-v3 is 5.7 GMAC with the classifier
    assert 11.0e9 < fid.flops_per_image() < 11.8e9


def test_bad_state_dicts_raise_before_any_device_work(sd, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work before the state dict was checked")
    monkeypatch.setattr(fid.L, "hip_lib", no_device)
    monkeypatch.setattr(fid.L, "conv_pack_weights", no_device)
    missing = {k: v for k, v in sd.items() if k != "Mixed_7c.branch3x3dbl_3b.bn.running_var"}
    with pytest.raises(KeyError, match="Mixed_7c.branch3x3dbl_3b.bn.running_var"):
        fid.InceptionV3(missing)
    wrong = dict(sd)
    wrong["Mixed_6c.branch7x7dbl_2.conv.weight"] = torch.zeros((160, 160, 1, 7))      # the module's filter is 7 x 1
    with pytest.raises(ValueError, match="Mixed_6c.branch7x7dbl_2.conv.weight"):
        fid.InceptionV3(wrong)
    with pytest.raises(AssertionError, match="device work"):                           # a good one gets as far as the library
        fid.InceptionV3({k: v for k, v in sd.items() if not k.startswith("fc.")})


def test_from_file_loads_weights_only(sd, tmp_path, monkeypatch):
    path = tmp_path / "inception.pth"
    torch.save(sd, path)
    seen = {}
    real_load = torch.load

    def load(f, *a, **kw):
        seen.update(kw)
        return real_load(f, *a, **kw)
    monkeypatch.setattr(torch, "load", load)
    got = fid.load_state_dict(str(path))
    assert seen.get("weights_only") is True and set(got) == set(sd)


# ---- the Frechet distance ---------------------------------------------------------------------------------------------------

def _sets(seed, n, m, d):
    rng = np.random.default_rng(seed)
    mix = rng.standard_normal((d, d)) / np.sqrt(d)
    a = rng.standard_normal((n, d)) @ mix + 0.3
    b = 1.2 * rng.standard_normal((m, d)) @ mix.T
    return a.astype(np.float32), b.astype(np.float32)


def test_frechet_distance_against_the_sqrtm_form():
    a, b = _sets(3, 120, 100, 64)
    got, ref = fid.frechet_distance(a, b), R.frechet_distance_sqrtm(a, b)
    print("frechet d=64: nuclear-norm form", got, "sqrtm form", ref, "relative", abs(got - ref) / abs(ref))
    assert ref > 1 and abs(got - ref) <= 1e-9 * abs(ref)


def test_frechet_distance_rank_deficient_against_the_eigenvalues():
    a, b = _sets(4, 20, 25, 192)
    got, ref = fid.frechet_distance(a, b), R.frechet_distance_eig(a, b)
    print("frechet d=192, 20 + 25 samples: nuclear-norm form", got, "eigenvalue form", ref, "relative", abs(got - ref) / abs(ref))
    assert ref > 1 and abs(got - ref) <= 1e-9 * abs(ref)


def test_frechet_distance_of_identical_sets_is_zero():
    a, _ = _sets(5, 30, 30, 64)
    trace = float(np.trace(np.cov(a.astype(np.float64), rowvar=False)))
    assert abs(fid.frechet_distance(a, a.copy())) <= 1e-9 * trace
    with pytest.raises(ValueError):
        fid.frechet_distance(a, a[:, :32])
    with pytest.raises(ValueError):
        fid.features(None, None, dims=100)


def test_reference_precision_recall_golden_holds_the_gap_condition():
    g = np.load(os.path.join(REPO, "tests", "golden", "fid_pr.npz"))
    assert len(g["sets"]) == len(R.PR_SETS)
    for (seed, n, m, d, k), (shift, p, r, gap), ref in zip(g["sets"], g["values"], g["reference"]):
        real, gen = R.feature_sets(int(seed), int(n), int(m), int(d), float(shift))
        assert R.min_gap(real, gen, int(k)) == gap and gap > R.GAP_BAR
        assert R.precision_recall(real, gen, int(k)) == (p, r)
        assert np.abs(ref - np.array([p, r, p, r])).max() < 1e-7            # the reference's full and part forms, fp32 means


# ---- the exports ------------------------------------------------------------------------------------------------------------

NEW = ("evc_inception_stem_im2col_f32", "evc_im2col_nhwc_f32", "evc_pool3x3s1p1_nhwc_f32", "evc_spatial_mean_nhwc_f32",
       "evc_knn_radius_f32", "evc_manifold_hits_f32")


def test_inception_exports_are_declared_bound_and_built():
    """Declared in the header, bound in lib.py, compiled from csrc/inception.hip, exported by the library; argument checks return
    EVC_EINVAL before any launch (the test runs without a GPU: a launch would fail)."""
    from evc_amd import build, lib
    header = open(os.path.join(REPO, "include", "evc_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header) and name in lib.HIP_SYMBOLS
    assert "inception.hip" in build.HIP_SOURCES and os.path.isfile(os.path.join(build.CSRC, "inception.hip"))
    so = lib.hip_lib(require_device=False)
    p = 16      # any non-null pointer: nothing is dereferenced before the checks
    assert so.evc_inception_stem_im2col_f32(None, p, 1, 3, 8, 8, 0, 1, 32, None) == -1
    assert so.evc_inception_stem_im2col_f32(p, p, 1, 4, 8, 8, 0, 1, 32, None) == -1           # 3 channels only
    assert so.evc_inception_stem_im2col_f32(p, p, 2, 3, 8, 8, 1, 2, 32, None) == -1           # frames beyond N
    assert so.evc_inception_stem_im2col_f32(p, p, 1, 3, 8, 8, 0, 1, 24, None) == -1           # 27 columns do not fit
    assert so.evc_inception_stem_im2col_f32(p, p, 1, 3, 0, 8, 0, 1, 32, None) == -1
    assert so.evc_im2col_nhwc_f32(p, None, 1, 8, 8, 16, 3, 3, 2, 2, 0, 0, 144, None) == -1
    assert so.evc_im2col_nhwc_f32(p, p, 1, 8, 8, 6, 3, 3, 2, 2, 0, 0, 56, None) == -1         # C % 4
    assert so.evc_im2col_nhwc_f32(p, p, 1, 8, 8, 16, 3, 3, 2, 2, 0, 0, 128, None) == -1       # ld_out < KH*KW*C
    assert so.evc_im2col_nhwc_f32(p, p, 1, 2, 8, 16, 3, 3, 1, 1, 0, 0, 144, None) == -1       # no output row
    assert so.evc_im2col_nhwc_f32(p, p, 1, 8, 8, 16, 3, 3, 0, 1, 0, 0, 144, None) == -1
    assert so.evc_pool3x3s1p1_nhwc_f32(p, p, 1, 4, 4, 4, 2, None) == -1                       # unknown mode
    assert so.evc_pool3x3s1p1_nhwc_f32(p, p, 1, 4, 4, 6, 0, None) == -1
    assert so.evc_pool3x3s1p1_nhwc_f32(p, None, 1, 4, 4, 4, 0, None) == -1
    assert so.evc_spatial_mean_nhwc_f32(p, p, 1, 0, 64, None) == -1
    assert so.evc_spatial_mean_nhwc_f32(p, p, 1, 64, 6, None) == -1
    assert so.evc_spatial_mean_nhwc_f32(None, p, 1, 64, 64, None) == -1
    assert so.evc_knn_radius_f32(p, p, 3, 8, 3, None) == -1                                   # n <= k
    assert so.evc_knn_radius_f32(p, p, 10, 6, 3, None) == -1                                  # d % 4
    assert so.evc_knn_radius_f32(p, p, 10, 8, 0, None) == -1 and so.evc_knn_radius_f32(p, p, 10, 8, 9, None) == -1
    assert so.evc_knn_radius_f32(p, None, 10, 8, 3, None) == -1
    assert so.evc_manifold_hits_f32(p, p, p, p, 4, 4, 6, None) == -1
    assert so.evc_manifold_hits_f32(p, p, p, p, 0, 4, 8, None) == -1
    assert so.evc_manifold_hits_f32(p, p, None, p, 4, 4, 8, None) == -1
    # the filter shapes of the network go through the dispatch's own query (no launch): all are stride-1 "same" shapes
    for kh, kw in ((1, 7), (7, 1), (1, 3), (3, 1), (5, 5), (3, 3)):
        assert isinstance(lib.conv_accepts(2, 17, 17, 128, 128, kh, kw, lib.ARITH_BF16X6, invariant=True), bool)
    assert not lib.conv_accepts(1, 8, 8, 16, 16, 7, 7, lib.ARITH_BF16X6)                      # 49 taps: refused, so im2col + 1x1
