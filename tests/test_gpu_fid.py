"""GPU tests of FID / precision-recall (evc_amd/fid.py, csrc/inception.hip): the pools, the NHWC im2col and the fused stem against
torch, every end point of the Inception-v3 against the float64 CPU restatement of tests/fid_recipe.py, batching, the set kernels
against the reference's goldens (tests/golden/fid_pr.npz) and float64, and the command lines."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fid_recipe as R
from conftest import REPO, golden

pytestmark = pytest.mark.gpu
U = 2.0 ** -24            # relative error of one fp32 rounding


@pytest.fixture(scope="module")
def L():
    import evc_amd  # noqa: F401
    from evc_amd import lib
    return lib


@pytest.fixture(scope="module")
def fid():
    import evc_amd  # noqa: F401
    from evc_amd import fid
    return fid


@pytest.fixture(scope="module")
def sd():
    return R.seeded_state_dict()


@pytest.fixture(scope="module")
def net(fid, sd):
    return fid.InceptionV3(sd, device="cuda:0", max_images=2)


def _nhwc(seed, shape):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape, dtype=np.float32))


def _same_bits(a, b):
    """Equal bit for bit, a NaN in the same places."""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


# ---- the pools --------------------------------------------------------------------------------------------------------------

POOL_SHAPES = [(1, 1, 4, 4), (1, 5, 7, 8), (2, 17, 17, 32), (1, 8, 8, 2048)]


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_max_pool_is_bit_exact(L, shape):
    x = _nhwc(3, shape) - 0.5                                         # negatives: the padding must not take part
    for with_nan in (False, True):
        if with_nan:
            x[0, shape[1] // 2, shape[2] // 2, 1] = float("nan")
        got = L.pool3x3s1p1_nhwc(x.cuda(), L.POOL_MAX).cpu()
        ref = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1)
        assert _same_bits(got, ref) and bool(torch.isnan(got).any()) == with_nan


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_avg_pool_against_float64(L, shape):
    x = _nhwc(4, shape)
    for with_nan in (False, True):
        if with_nan:
            x[0, shape[1] // 2, shape[2] // 2, 1] = float("nan")
        got = L.pool3x3s1p1_nhwc(x.cuda(), L.POOL_AVG).cpu().double()
        xc = x.double().permute(0, 3, 1, 2)
        ref = F.avg_pool2d(xc, 3, 1, 1, count_include_pad=False).permute(0, 2, 3, 1)
        # eight additions and one division of 0.5 ulp each on sum|x| / count
        bound = 9 * U * F.avg_pool2d(xc.abs(), 3, 1, 1, count_include_pad=False).permute(0, 2, 3, 1)
        nan = torch.isnan(ref)
        assert torch.equal(torch.isnan(got), nan) and bool(nan.any()) == with_nan
        assert bool(((got - ref).abs() <= bound)[~nan].all())


# ---- im2col -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,k,stride,pad", [
    ((2, 35, 35, 16), (3, 3), (2, 2), (0, 0)), ((1, 7, 9, 16), (3, 3), (2, 2), (0, 0)), ((1, 5, 9, 16), (1, 7), (1, 1), (0, 3)),
    ((1, 5, 9, 16), (7, 1), (1, 1), (3, 0)), ((1, 6, 6, 16), (5, 5), (1, 1), (2, 2)), ((1, 9, 7, 4), (3, 3), (1, 1), (0, 0))])
def test_im2col_nhwc_is_bit_exact(L, shape, k, stride, pad):
    N, H, W, C = shape
    x = _nhwc(5, shape)
    K = k[0] * k[1] * C
    Ho, Wo = (H + 2 * pad[0] - k[0]) // stride[0] + 1, (W + 2 * pad[1] - k[1]) // stride[1] + 1
    out = torch.full((N, Ho, Wo, K + 16), float("nan"), device="cuda")
    got = L.im2col_nhwc(x.cuda(), k[0], k[1], stride, pad, ld_out=K + 16, out=out).cpu()
    ref = F.unfold(x.permute(0, 3, 1, 2), k, padding=pad, stride=stride)                  # (N, C * KH * KW, Ho * Wo), (c, ky, kx)
    ref = ref.view(N, C, k[0] * k[1], Ho, Wo).permute(0, 3, 4, 2, 1).reshape(N, Ho, Wo, K)     # -> (ky, kx, c)
    assert torch.equal(got[..., :K], ref) and bool((got[..., K:] == 0).all())
    assert torch.equal(L.im2col_nhwc(x.cuda(), k[0], k[1], stride, pad).cpu(), ref)       # dense rows


# ---- the stem ---------------------------------------------------------------------------------------------------------------

def _rows(pre):
    """(N, 3, 299, 299) -> the (N, 149, 149, 27) patch rows of a 3x3 stride-2 unpadded convolution, (c, ky, kx) order."""
    n = pre.shape[0]
    return F.unfold(pre, 3, stride=2).view(n, 27, 149, 149).permute(0, 2, 3, 1)


@pytest.mark.parametrize("shape", [(2, 3, 96, 128), (1, 3, 128, 128), (1, 3, 299, 299), (1, 3, 320, 300)])
def test_stem_rows_against_float64_interpolate(L, shape):
    """The kernel maps the four source pixels 2x - 1 (one rounding), interpolates along x (a correctly rounded weight, a multiply
    and an add: three roundings) and along y (three more): seven roundings, within the bound of eight on max|2x - 1|."""
    x = R.images(6, shape[0], shape[2], shape[3])
    out = torch.full((shape[0], 149, 149, 32), float("nan"), device="cuda")
    got = L.inception_stem_im2col(x.cuda(), 0, out).cpu()
    ref = _rows(R.preprocess(x.double()))
    err = float((got[..., :27].double() - ref).abs().max())
    print(f"stem {shape}: max error {err:.3e}, bound {8 * U * float(ref.abs().max()):.3e}")
    assert err <= 8 * U * float(ref.abs().max()) and bool((got[..., 27:] == 0).all())
    if shape[2:] == (299, 299):
        assert torch.equal(got[..., :27], _rows(2 * x - 1))
    # a frame range: the rows of image N - 1 alone
    last = L.inception_stem_im2col(x.cuda(), shape[0] - 1, torch.empty((1, 149, 149, 32), device="cuda")).cpu()
    assert torch.equal(last[0], got[-1])


@pytest.mark.parametrize("shape,at,has_nan", [((1, 3, 128, 128), (1, 1), True), ((2, 3, 96, 128), (1, 126), True),
                                              ((1, 3, 128, 128), (40, 0), False), ((1, 3, 320, 300), (1, 1), False)])
def test_stem_inf_pixel_gives_nan_where_torch_does(L, shape, at, has_nan):
    """A NaN arises where a zero weight meets the inf: output rows / columns whose source position is clamped at 0 (up-scaling)
    take weight 0 from source row / column 1.  Interior positions and down-scaling have no zero weight: the inf spreads as inf."""
    x = R.images(7, shape[0], shape[2], shape[3])
    x[0, 1, at[0], at[1]] = float("inf")
    got = L.inception_stem_im2col(x.cuda(), 0, torch.empty((shape[0], 149, 149, 32), device="cuda")).cpu()[..., :27]
    ref = _rows(R.preprocess(x))                                     # torch's float32 interpolate
    assert bool(torch.isnan(ref).any()) == has_nan and bool(torch.isinf(ref).any())
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(torch.isinf(got), torch.isinf(ref))


# ---- the network ------------------------------------------------------------------------------------------------------------

def _nchw(t):
    return t.permute(0, 3, 1, 2) if t.dim() == 4 else t


@pytest.fixture(scope="module")
def end_points(net, sd):
    """Every end point of two 128 x 128 images and one 96 x 128 image: HIP, and the CPU restatement in float64 and float32."""
    sets = [R.images(31, 2, 128, 128), R.images(32, 1, 96, 128)]
    hip, f64, f32 = {}, {}, {}
    for x in sets:
        blocks, eps = net.forward(x, endpoints=True)
        eps = dict(eps, **{f"block{i}": b for i, b in enumerate(blocks)})
        r64, r32 = R.forward(sd, x, torch.float64), R.forward(sd, x, torch.float32)
        for name in R.END_POINTS:
            hip.setdefault(name, []).append(_nchw(eps[name]).cpu().double())
            f64.setdefault(name, []).append(r64[name])
            f32.setdefault(name, []).append(r32[name].double())
    cat = lambda d: {k: torch.cat([t.flatten(1) for t in v]) for k, v in d.items()}       # noqa: E731
    shapes = {k: [tuple(t.shape) for t in v] for k, v in hip.items()}
    ref_shapes = {k: [tuple(t.shape) for t in v] for k, v in f64.items()}
    return cat(hip), cat(f64), cat(f32), shapes, ref_shapes


def _errors(end_points):
    hip, f64, f32, _, _ = end_points
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())                         # noqa: E731
    return {name: (rel(hip[name], f64[name]), rel(f32[name], f64[name])) for name in R.END_POINTS}


def test_every_end_point_against_the_float64_restatement(end_points):
    """e_hip = max|hip - f64| / max|f64| against e_t32, the same for torch's float32 CPU evaluation: both accumulate in fp32 in
    different orders, so a factor of 2 over the other fp32 implementation is the margin."""
    assert end_points[3] == end_points[4]
    assert end_points[3]["block0"][0] == (2, 64, 73, 73) and end_points[3]["block3"][1] == (1, 2048)
    errors = _errors(end_points)
    for name, (e_hip, e_t32) in errors.items():
        print(f"end point {name}: e_hip {e_hip:.3e} e_t32 {e_t32:.3e} ratio {e_hip / e_t32:.2f}")
    worst = {name: e for name, e in errors.items() if not e[0] <= 2 * e[1]}
    assert not worst, worst


def test_batched_equals_one_image_at_a_time(fid, net):
    x = R.images(33, 3, 128, 128)                                    # max_images = 2: a chunk of two and a chunk of one
    for dims in (2048, 64):
        batched = fid.features(x, net, dims)
        single = np.concatenate([fid.features(x[i:i + 1], net, dims) for i in range(3)])
        assert batched.shape == (3, dims) and batched.dtype == np.float32 and np.array_equal(batched, single)


def test_features_are_the_spatial_mean_of_the_block(fid, net, L):
    x = R.images(34, 2, 128, 128)
    blocks = net.forward(x)
    assert [tuple(b.shape) for b in blocks] == [(2, 73, 73, 64), (2, 35, 35, 192), (2, 17, 17, 768), (2, 2048)]
    for dims, i in fid.BLOCK_INDEX_BY_DIM.items():
        got = fid.features(x, net, dims)
        if i == 3:
            assert np.array_equal(got, blocks[3].cpu().numpy())
            continue
        b = blocks[i].cpu().double()
        hw = b.shape[1] * b.shape[2]
        assert np.array_equal(got, L.spatial_mean_nhwc(blocks[i]).cpu().numpy())
        # the kernel adds in fp64 and rounds the quotient once: half an ulp of the mean, and the fp64 sum's own error
        bound = U * b.mean((1, 2)).abs() + hw * 2.0 ** -52 * b.abs().mean((1, 2))
        assert bool(((torch.from_numpy(got).double() - b.mean((1, 2))).abs() <= bound).all()), dims


# ---- precision / recall -----------------------------------------------------------------------------------------------------

def test_precision_recall_equals_the_reference_goldens(fid):
    g = golden("fid_pr")
    for (seed, n, m, d, k), (shift, p, r, gap) in zip(g["sets"], g["values"]):
        real, gen = R.feature_sets(int(seed), int(n), int(m), int(d), float(shift))
        assert R.min_gap(real, gen, int(k)) > R.GAP_BAR                  # the condition under which exact equality is asked
        assert fid.precision_recall(real, gen, k=int(k)) == (p, r)


@pytest.mark.parametrize("k", [1, 3, 8])
def test_knn_radius_against_float64(L, k):
    real, _ = R.feature_sets(7, 40, 30, 64, 0.6)
    got = L.knn_radius(torch.from_numpy(real).cuda(), k).cpu().numpy()
    ref = R.knn_radius2(real, k)
    assert got.dtype == np.float64 and np.abs(got - ref).max() <= 1e-12 * ref.max() and (np.abs(got - ref) <= 1e-12 * ref).all()
    wide = np.random.default_rng(8).standard_normal((70, 2048)).astype(np.float32)        # the width of block 3
    got = L.knn_radius(torch.from_numpy(wide).cuda(), k).cpu().numpy()
    assert (np.abs(got - R.knn_radius2(wide, k)) <= 1e-12 * got).all()


def test_set_kernels_refuse_bad_sizes(L):
    x = torch.zeros((3, 8), device="cuda")
    with pytest.raises(L.EvcKernelError, match="code -1"):
        L.knn_radius(x, 3)                                           # n <= k
    with pytest.raises(L.EvcKernelError, match="code -1"):
        L.knn_radius(torch.zeros((10, 6), device="cuda"), 3)         # d % 4
    with pytest.raises(L.EvcKernelError, match="code -1"):
        L.manifold_hits(torch.zeros((4, 6), device="cuda"), torch.zeros((4, 6), device="cuda"), torch.zeros(4, device="cuda", dtype=torch.float64))


# ---- the distance through the network -----------------------------------------------------------------------------------------

def test_calculate_fid_against_the_restatement(fid, net, sd, end_points):
    """12 + 10 frames at dims = 64 against the float64 Frechet distance of the restatement's float64 features.  The sets have
    fewer samples than features, where the sqrtm form is itself only good to about 1e-7, so the yardstick is fid_ref's eigenvalue
    form.  The distance is a smooth function of the features: ten times the relative error of block 0 is the bar."""
    a, b = R.images(41, 12, 128, 128), 0.6 * R.images(42, 10, 128, 128)
    got = fid.calculate_fid(a, b, net, dims=64)
    ref = R.frechet_distance_eig(*[R.forward(sd, v, torch.float64, last="block0")["block0"].mean((2, 3)).numpy() for v in (a, b)])
    e_block0 = _errors(end_points)["block0"][0]
    print(f"calculate_fid dims=64: hip {got!r} float64 {ref!r} relative {abs(got - ref) / ref:.3e}, block 0 feature error {e_block0:.3e}")
    assert ref > 1 and abs(got - ref) <= 10 * e_block0 * ref


# ---- the command lines ----------------------------------------------------------------------------------------------------

MODEL = ["--synthetic", "--config_mod", "model.ngf=32 model.n_head_channels=32"]
LINE = re.compile(r"FID: (-?\d+\.\d+) precision: (\d\.\d{5}) recall: (\d\.\d{5})")


def test_cli_writes_fid_next_to_unchanged_outputs_and_the_receiver_prints_it(tmp_path, monkeypatch, sd, capsys):
    import evc_amd  # noqa: F401
    from evc_amd import cli, receiver
    monkeypatch.chdir(tmp_path)
    weights = tmp_path / "inception_seeded.pth"
    torch.save(sd, weights)
    common = ["--config", os.path.join(REPO, "configs", "mine.yml"), "--exp", str(tmp_path / "exp"), "--data_npy", "missing.npy"]

    def run(out, extra):
        cli.main(common + ["--output_path", str(out), "--start_idx", "0", "--end_idx", "0", "--subsample", "2", "--q", "3",
                           "--policy", "psnr", "--thresholds", "200", "-100", "--bpp-limit", "1e9"] + MODEL + extra)
        return capsys.readouterr().out

    fid_flags = ["--fid", str(weights), "--fid-dims", "64"]
    log_with = run(tmp_path / "with", fid_flags + ["--bitstream-dir", str(tmp_path / "bits")])
    log_without = run(tmp_path / "without", ["--bitstream-dir", str(tmp_path / "bits0")])
    d, d0 = tmp_path / "with" / "output_0", tmp_path / "without" / "output_0"
    sent = LINE.findall(log_with)
    assert len(sent) == 2 and sum(ln.count("FID:") for ln in log_with.splitlines()) == 2 and "FID" not in log_without
    env, vals, pr = np.load(d / "fid_0.npy"), np.load(d / "fid_values_0.npy"), np.load(d / "pr_values_0.npy")
    assert env.shape[0] == 2 and env.ndim == 2 and np.isfinite(env).all()
    assert vals.shape == (2,) and np.isfinite(vals).all()
    assert pr.shape == (2, 2) and np.isfinite(pr).all() and (pr >= 0).all() and (pr <= 1).all()
    assert [float(s[0]) for s in sent] == [float("%f" % v) for v in vals]
    for f in sorted(p.name for p in d0.iterdir()):
        if f.endswith(".npy"):
            assert (d / f).read_bytes() == (d0 / f).read_bytes(), f
    assert sorted(p.name for p in d.iterdir()) == sorted([p.name for p in d0.iterdir()] + ["fid_0.npy", "fid_values_0.npy", "pr_values_0.npy"])

    # the receiver: the same line per job, on the streams the sender wrote (the synthetic clips saved as its originals)
    from evc_amd import synthetic
    np.save(tmp_path / "clips.npy", synthetic.make_clips(1, seed=1234))
    receiver.main(["--config", os.path.join(REPO, "configs", "mine.yml"), "--exp", str(tmp_path / "exp"), "--data_npy",
                   str(tmp_path / "clips.npy"), "--bitstream-dir", str(tmp_path / "bits"), "--output_path", str(tmp_path / "rx")]
                  + MODEL + fid_flags)
    out = capsys.readouterr().out
    got = LINE.findall(out)
    assert len(got) == 2 and "frames: MISMATCH" not in out
    for a, b in zip(sorted(float(g[0]) for g in got), sorted(float(s[0]) for s in sent)):       # the sender's frames, decoded again
        assert abs(a - b) <= 1e-3 * abs(b) + 1e-6, (got, sent)
