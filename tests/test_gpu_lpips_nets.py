"""GPU tests of the LPIPS family (evc_amd/lpips.py ``Lpips``; csrc/lpips.hip evc_maxpool2d_nhwc_f32, evc_lpips_map_f32,
evc_lpips_map_mean_f32, evc_lpips_upsample_add_f32) against torch and the float64 restatement of tests/lpips_ref.py.

Bars of the networks (float32 torch CPU against float64 on the same inputs: worst tap 7.3e-7 of its max, worst distance 2.3e-6
relative, worst map 1.8e-6 of its max): taps <= 2e-5 max|ref|, distances rtol 2e-4, map elements <= 2e-4 max|ref|.
Bars of the single kernels are derived where they are used."""
import contextlib
import functools
import io
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R
from conftest import golden

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAP_BAR, DIST_RTOL, MAP_BAR = 2e-5, 2e-4, 2e-4
SIZES = {"vgg": [(32, 32), (40, 24), (16, 16)], "squeeze": [(34, 34), (35, 21), (17, 17)], "alex": [(64, 64), (67, 35), (35, 35)]}
NET_CASES = [(net, size) for net in R.NETS for size in SIZES[net]]
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def L():
    import evc_amd  # noqa: F401
    from evc_amd import lib
    lib.hip_lib()
    return lib


@functools.lru_cache(maxsize=None)
def state_dict(net):
    return R.seeded_state_dict(net, 21, golden(f"lpips_{net}_lin"))


@functools.lru_cache(maxsize=None)
def hip_net(net, max_pairs=None, saved=False):
    from evc_amd.lpips import Lpips
    sd = state_dict(net)
    return Lpips(net, R.as_saved_module(net, sd) if saved else sd, max_pairs=max_pairs)


@functools.lru_cache(maxsize=None)
def case(net, size, n=3):
    """Inputs and the float64 references of one (net, size), computed once and shared (never written to)."""
    a, b = R.pairs(100 + size[0] + size[1], n, *size)
    sd = state_dict(net)
    with torch.no_grad():
        taps = R.features(net, sd, torch.cat([a, b]).double())
        dist = R.distance(net, sd, a.double(), b.double())
        smap = R.spatial_map(net, sd, a.double(), b.double())
    assert (dist > 1e-5).all(), dist
    return types.SimpleNamespace(a=a, b=b, taps=taps, dist=dist, map=smap)


def check_against(c, got_d=None, got_m=None, rows=None, what=""):
    rows = range(len(c.dist)) if rows is None else rows
    if got_d is not None:
        rel = max(abs(float(got_d[i]) - float(c.dist[r])) / float(c.dist[r]) for i, r in enumerate(rows))
        print(f"{what}: worst distance error {rel:.3e} relative (bar {DIST_RTOL})")
        assert rel <= DIST_RTOL
    if got_m is not None:
        ref = c.map[list(rows)]
        worst = float((got_m.double().cpu() - ref).abs().max() / ref.abs().max())
        print(f"{what}: worst map error {worst:.3e} of max|ref| (bar {MAP_BAR})")
        assert worst <= MAP_BAR


# ---- the kernels against torch ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 5, 3, 8), (2, 8, 8, 64), (1, 17, 10, 128)])
@pytest.mark.parametrize("k,stride,ceil", [(2, 2, False), (3, 2, True)])
def test_maxpool2d_bit_exact_with_overhanging_windows_and_a_nan(L, shape, k, stride, ceil):
    """(3, 2, ceil) on sides 8, 10 and 17: 8 -> 4 and 10 -> 5 with a last window hanging over the edge by one; on side 3: one window."""
    x = torch.from_numpy(np.random.default_rng(sum(shape)).standard_normal(shape).astype(np.float32))
    x[0, shape[1] - 1, shape[2] - 1, 3] = float("nan")                   # in the last (overhanging) window
    x[-1, 1, 1, 0] = float("nan")
    ref = F.max_pool2d(x.permute(0, 3, 1, 2), k, stride, ceil_mode=ceil).permute(0, 2, 3, 1)
    got = L.maxpool2d_nhwc(x.cuda(), k, stride, ceil_mode=ceil).cpu()
    assert got.shape == ref.shape and int(torch.isnan(ref).sum()) >= 1
    np.testing.assert_array_equal(got.numpy(), ref.numpy())


@pytest.mark.parametrize("C", [64, 384, 512])
@pytest.mark.parametrize("HW", [1, 2, 1024])
def test_lpips_map_against_float64(L, C, HW):
    """Bar 2e-5 relative per pixel.  Both inputs are independent ReLU-ed normals, so no difference cancels.  The norm is a sum of
    C squares in C / 64 serial steps and a 4-step tree (<= 12 roundings), its reciprocal square root form adds 4, the
    normalised difference 3 per image, squaring and weighting 3, the weighted sum again <= 12: under 40 roundings in a chain
    where every term is non-negative, i.e. <= 40 * 2^-24 = 2.4e-6 relative if every rounding fell the same way; 2e-5 leaves 8x."""
    rng = np.random.default_rng(C + HW)
    f0, f1 = (torch.from_numpy(np.maximum(rng.standard_normal((3, HW, 1, C)), 0).astype(np.float32)) for _ in range(2))
    w = torch.from_numpy(np.abs(rng.standard_normal(C)).astype(np.float32) / C)
    ref = R.layer_map(f0.double().permute(0, 3, 1, 2), f1.double().permute(0, 3, 1, 2), w)[:, 0]
    got = L.lpips_map(f0.cuda(), f1.cuda(), w.cuda()).cpu().double()
    worst = float(((got - ref).abs() / ref).max())
    print(f"C {C} HW {HW}: worst pixel {worst:.3e} relative")
    assert got.shape == ref.shape and float(ref.min()) > 0 and worst <= 2e-5


@pytest.mark.parametrize("HW", [1, 2, 1000, 16384])
def test_lpips_map_mean_against_float64(L, HW):
    """Positive inputs: a thread adds ceil(HW / 256) values in order, then 6 tree steps, 3 wave sums and the division, each
    rounding <= 2^-24 of a partial sum that never exceeds the total: rtol (ceil(HW / 256) + 10) * 2^-24."""
    m = torch.from_numpy(np.random.default_rng(HW).random((3, HW)).astype(np.float32))
    ref = m.double().mean(1)
    bar = ((HW + 255) // 256 + 10) * EPS
    dist = torch.full((3,), 7.0, device="cuda")
    L.lpips_map_mean(m.cuda(), dist, accumulate=False)
    worst = float(((dist.cpu().double() - ref).abs() / ref).max())
    print(f"HW {HW}: worst mean {worst:.3e} relative (bar {bar:.3e})")
    assert worst <= bar
    first = dist.clone()
    L.lpips_map_mean(m.cuda(), dist, accumulate=True)
    assert torch.equal(dist, first + first)                                   # same order every time, then one float32 addition


@pytest.mark.parametrize("hw,HW", [((1, 1), (16, 16)), ((2, 1), (40, 24)), ((7, 7), (128, 128)), ((16, 16), (34, 34))])
def test_upsample_add_against_torch_float32(L, hw, HW):
    """1 ulp of the output's max (2^-23 max|ref|) against torch's own float32 kernel on the device, with and without accumulate."""
    rng = np.random.default_rng(hw[0] * 100 + HW[0])
    m = torch.from_numpy(rng.random((3,) + hw).astype(np.float32)).cuda()
    ref = F.interpolate(m[:, None], size=HW, mode="bilinear", align_corners=False)[:, 0]
    cpu = F.interpolate(m.cpu()[:, None], size=HW, mode="bilinear", align_corners=False)[:, 0]
    out = torch.full((3,) + HW, float("nan"), device="cuda")
    L.lpips_upsample_add(m, out, accumulate=False)
    ulp = float(ref.abs().max()) * 2.0 ** -23
    worst = float((out - ref).abs().max())
    print(f"{hw} -> {HW}: worst {worst / ulp:.3f} ulp of the max against torch on the device, "
          f"{float((out.cpu() - cpu).abs().max()) / ulp:.3f} against torch on the CPU")
    assert worst <= ulp
    base = torch.from_numpy(rng.random((3,) + HW).astype(np.float32)).cuda()
    acc = base.clone()
    L.lpips_upsample_add(m, acc, accumulate=True)
    want = base + ref
    assert float((acc - want).abs().max()) <= float(want.abs().max()) * 2.0 ** -23
    assert torch.equal(acc, base + out)                                        # accumulate adds exactly what it stores otherwise


def test_upsample_add_propagates_nan_and_inf_as_torch(L):
    m = torch.rand((2, 5, 4), generator=torch.Generator().manual_seed(1)).cuda()
    m[0, 2, 1], m[1, 0, 3] = float("nan"), float("inf")
    ref = F.interpolate(m[:, None], size=(20, 12), mode="bilinear", align_corners=False)[:, 0]
    out = torch.empty_like(ref)
    L.lpips_upsample_add(m, out, accumulate=False)
    assert torch.equal(torch.isnan(out), torch.isnan(ref)) and torch.equal(torch.isinf(out), torch.isinf(ref))
    assert bool(torch.isnan(ref).any()) and bool(torch.isinf(ref).any()) and bool(torch.isfinite(ref).any())


# ---- the networks -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("net,size", NET_CASES)
def test_taps_distances_and_maps_against_the_restatement(L, net, size):
    c, hip = case(net, size), hip_net(net)
    a, b = c.a.cuda(), c.b.cuda()
    taps = hip.features(torch.cat([a, b]))
    assert [tuple(t.shape) for t in taps] == [(6,) + tuple(r.shape[2:]) + (r.shape[1],) for r in c.taps]
    worst = max(float((t.permute(0, 3, 1, 2).cpu().double() - r).abs().max() / r.abs().max()) for t, r in zip(taps, c.taps))
    print(f"{net} {size}: worst tap error {worst:.3e} of max|ref| (bar {TAP_BAR})")
    assert worst <= TAP_BAR
    d, m = hip(a, b), hip.spatial_map(a, b)
    assert d.shape == (3,) and m.shape == (3,) + size and d.dtype == m.dtype == torch.float32
    check_against(c, d, m, what=f"{net} {size}")
    one_d, one_m = hip(a[1], b[1]), hip.spatial_map(a[1], b[1])                 # the (3, H, W) single-frame form
    assert one_d.shape == (1,) and one_m.shape == (1,) + size
    check_against(c, one_d, one_m, rows=[1], what=f"{net} {size} single frame")
    assert float(hip(a, a).abs().max()) == 0.0 and float(hip.spatial_map(b, b).abs().max()) == 0.0


@pytest.mark.parametrize("net", R.NETS)
def test_key_spellings_normalize_and_max_pairs(L, net):
    size = SIZES[net][1]
    c, hip = case(net, size), hip_net(net)
    a, b = c.a.cuda(), c.b.cuda()
    d, m = hip(a, b), hip.spatial_map(a, b)
    saved = hip_net(net, saved=True)                                           # net.slice<K>.<idx> / lins.<k>. spellings
    assert torch.equal(saved(a, b), d) and torch.equal(saved.spatial_map(a, b), m)
    assert torch.equal(hip(a, b, normalize=True), hip(a * 2 - 1, b * 2 - 1))
    assert torch.equal(hip.spatial_map(a, b, normalize=True), hip.spatial_map(a * 2 - 1, b * 2 - 1))
    assert not torch.equal(hip(a, b, normalize=True), d)
    single = hip_net(net, max_pairs=1)                                         # three backbone passes of one pair each
    check_against(c, single(a, b), single.spatial_map(a, b), what=f"{net} {size} max_pairs=1")
    two = hip_net(net, max_pairs=2)                                            # a pass of two and a pass of one
    check_against(c, two(a, b), two.spatial_map(a, b), what=f"{net} {size} max_pairs=2")
    check_against(c, d, m, what=f"{net} {size} one pass")
    sm = hip.spatial_mean(a, b, normalize=False)
    assert sm.shape == (3,) and float(((sm.cpu().double() - c.map.mean((1, 2))).abs() / c.map.mean((1, 2))).max()) <= DIST_RTOL


@pytest.mark.parametrize("net,size,n", [("vgg", (64, 64), 1), ("alex", (128, 128), 1)])
def test_one_full_size_pair(L, net, size, n):
    """VGG at 64x64; AlexNet's spatial map at 128x128, whose taps 31, 15, 7 up-sample by non-integer factors."""
    c, hip = case(net, size, n), hip_net(net)
    if net == "alex":
        assert [tuple(t.shape[2:]) for t in c.taps] == [(31, 31), (15, 15), (7, 7), (7, 7), (7, 7)]
    check_against(c, hip(c.a.cuda(), c.b.cuda()), hip.spatial_map(c.a.cuda(), c.b.cuda()), what=f"{net} {size}")


def test_wrong_shapes_and_missing_keys_are_refused(L):
    from evc_amd.lpips import Lpips
    sd = dict(state_dict("squeeze"))
    bad = dict(sd)
    del bad["features.7.expand3x3.bias"]
    with pytest.raises(KeyError, match="features.7.expand3x3.bias"):
        Lpips("squeeze", bad)
    bad = dict(sd)
    bad["features.3.squeeze.weight"] = torch.zeros(16, 64, 3, 3)
    with pytest.raises(ValueError, match="features.3.squeeze"):
        Lpips("squeeze", bad)
    bad = dict(sd)
    bad["lin3.model.1.weight"] = torch.zeros(1, 256, 1, 1)
    with pytest.raises(ValueError, match="lin3"):
        Lpips("squeeze", bad)
    with pytest.raises(ValueError, match="resnet"):
        Lpips("resnet", sd)


@pytest.mark.parametrize("net", R.NETS)
def test_a_nan_pixel_makes_its_pair_nan_and_no_other(L, net):
    size = SIZES[net][0]
    c, hip = case(net, size), hip_net(net)
    a = c.a.clone()
    a[1, 2, size[0] // 2, size[1] // 2] = float("nan")
    d, m = hip(a.cuda(), c.b.cuda()).cpu(), hip.spatial_map(a.cuda(), c.b.cuda()).cpu()
    assert bool(torch.isnan(d[1])) and bool(torch.isnan(m[1]).all()) and bool(torch.isfinite(d[[0, 2]]).all())
    assert bool(torch.isfinite(m[[0, 2]]).all())
    check_against(c, d[[0, 2]], m[[0, 2]], rows=[0, 2], what=f"{net} {size} beside a NaN pair")


# ---- the command lines ----------------------------------------------------------------------------------------------------

MODEL = ["--synthetic", "--config_mod", "model.ngf=32 model.n_head_channels=32"]


@pytest.fixture(scope="module")
def sender_runs(tmp_path_factory):
    """A two-job psnr sweep with and without --lpips vgg:..., each job written as a job stream, and a two-job lpips sweep on the
    squeeze backbone; the weight files are the seeded state dicts, saved as the packages would have them."""
    import evc_amd  # noqa: F401
    from evc_amd import cli, synthetic
    tmp = tmp_path_factory.mktemp("lpips_cli")
    np.save(tmp / "clips.npy", synthetic.make_clips(1, seed=1234))
    for net in ("vgg", "squeeze"):
        sd = state_dict(net)
        torch.save({k: v for k, v in sd.items() if k.startswith("features.")}, tmp / f"{net}_backbone.pth")
        torch.save({k: v for k, v in sd.items() if k.startswith("lin")}, tmp / f"{net}.pth")
    torch.save(R.as_saved_module("vgg", state_dict("vgg")), tmp / "vgg_saved.pth")
    mp, text = pytest.MonkeyPatch(), {}
    mp.chdir(tmp)

    def run(name, extra, policy="psnr", thresholds=("200", "-100")):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            cli.main(["--config", os.path.join(REPO, "configs", "mine.yml"), "--exp", str(tmp / "exp"), "--data_npy",
                      str(tmp / "clips.npy"), "--output_path", str(tmp / name), "--start_idx", "0", "--end_idx", "0", "--subsample",
                      "2", "--q", "3", "--policy", policy, "--thresholds", *thresholds, "--bpp-limit", "1e9"] + MODEL + extra)
        text[name] = buf.getvalue()

    try:
        run("with", ["--lpips", f"vgg:{tmp / 'vgg_backbone.pth'},{tmp / 'vgg.pth'}", "--bitstream-dir", str(tmp / "bits")])
        run("without", ["--bitstream-dir", str(tmp / "bits0")])
        run("rule", ["--lpips-net", "squeeze", "--metric", f"{tmp / 'squeeze_backbone.pth'},{tmp / 'squeeze.pth'}"], policy="lpips",
            thresholds=("100", "-1"))
    finally:
        mp.undo()
    return types.SimpleNamespace(tmp=tmp, log=text)


def _clip(half):
    return np.stack([half[:, f * 128:(f + 1) * 128].transpose(2, 0, 1) for f in range(30)])


def test_sender_writes_lpips_next_to_unchanged_outputs(L, sender_runs):
    tmp = sender_runs.tmp
    d, d0 = tmp / "with" / "output_0", tmp / "without" / "output_0"
    frames, env = np.load(d / "lpips_vgg_frames_0.npy"), np.load(d / "lpips_vgg_0.npy")
    assert frames.shape == (2, 30) and frames.dtype == np.float64 and np.isfinite(frames).all() and (frames >= 0).all()
    assert env.shape[0] == 2 and np.isfinite(env).all()
    printed = [float(m) for m in re.findall(r"LPIPS\(vgg\): (\d+\.\d{5})\b", sender_runs.log["with"])]
    assert printed == [float("%.5f" % v) for v in frames.mean(axis=1)]
    assert "LPIPS" not in sender_runs.log["without"] and not list(d0.glob("lpips*"))
    for f in sorted(p.name for p in d0.iterdir()):
        if f.endswith(".npy"):
            assert (d / f).read_bytes() == (d0 / f).read_bytes(), f
    assert sorted(p.name for p in d.iterdir()) == sorted([p.name for p in d0.iterdir()] + ["lpips_vgg_0.npy", "lpips_vgg_frames_0.npy"])
    drop = lambda text: [ln.replace(str(tmp / "without"), "OUT").replace(str(tmp / "with"), "OUT").replace("bits0", "bits")  # noqa: E731
                         for ln in text.splitlines() if "LPIPS" not in ln and not ln.startswith("done in")]
    assert drop(sender_runs.log["with"]) == drop(sender_runs.log["without"])
    # the values are a direct call's on the frames the run saved (upper half: originals, lower half: decoded frames); the one
    # saved state dict gives the same network
    from evc_amd.lpips import Lpips
    img = np.load(d / "city_output_npy_idx0_q3_thr-100.00.npy")
    job = ["thr -100.00" in ln for ln in sender_runs.log["with"].splitlines() if "LPIPS(vgg):" in ln].index(True)
    x, gt = torch.from_numpy(_clip(img[128:])), torch.from_numpy(_clip(img[:128]))
    net = Lpips.from_spec(f"vgg:{tmp / 'vgg_saved.pth'}")
    direct = net.spatial_mean(x, gt).double().cpu().numpy()
    np.testing.assert_array_equal(frames[job], direct)
    rel = np.abs(direct - net.spatial_map(x, gt, normalize=True).double().mean((1, 2)).cpu().numpy()) / direct
    assert rel.max() <= 1e-5                                                    # the mean of the map, in another summation order


def test_lpips_net_drives_the_accept_rule(L, sender_runs):
    tmp = sender_runs.tmp
    d = tmp / "rule" / "output_0"
    assert "decision rule: lpips (--policy)" in sender_runs.log["rule"]
    vals = np.load(d / "lpips_frames_0.npy")                                    # the file --policy lpips always wrote
    assert vals.shape == (2, 30) and not list(d.glob("lpips_squeeze*"))
    sent = {float(m.group(1)): sum(int(v) for v in m.group(2).split(","))
            for m in re.finditer(r"thr (-?\d+\.\d{2}): d=\[([0-9, ]+)\]", sender_runs.log["rule"])}
    assert sent[100.0] == 2 and sent[-1.0] > sent[100.0]                       # accepted everything / nothing
    from evc_amd.lpips import Lpips
    sq = Lpips.from_spec(f"{tmp / 'squeeze_backbone.pth'},{tmp / 'squeeze.pth'}", "squeeze")
    jobs = [float(m) for m in re.findall(r"thr (-?\d+\.\d{2}): d=", sender_runs.log["rule"])]
    img = np.load(d / "city_output_npy_idx0_q3_thr100.00.npy")
    x, gt = torch.from_numpy(_clip(img[128:])), torch.from_numpy(_clip(img[:128]))
    np.testing.assert_array_equal(vals[jobs.index(100.0)], sq(x, gt).double().cpu().numpy())      # frames as they are
    assert not np.array_equal(vals[jobs.index(100.0)], sq(x, gt, normalize=True).double().cpu().numpy())


def test_receiver_prints_the_line(L, sender_runs, capsys):
    from evc_amd import receiver
    tmp = sender_runs.tmp
    assert len(os.listdir(tmp / "bits")) == 2
    sent = {m.group(1): float(m.group(2)) for m in re.finditer(r"thr (-?\d+\.\d{2}): LPIPS\(vgg\): (\d+\.\d{5})", sender_runs.log["with"])}
    receiver.main(["--config", os.path.join(REPO, "configs", "mine.yml"), "--exp", str(tmp / "exp"), "--data_npy",
                   str(tmp / "clips.npy"), "--bitstream-dir", str(tmp / "bits"), "--output_path", str(tmp / "rx"),
                   "--lpips", f"vgg:{tmp / 'vgg_backbone.pth'},{tmp / 'vgg.pth'}"] + MODEL)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("job_")]
    assert len(lines) == 2 and len(sent) == 2
    for ln in lines:
        m = re.search(r"thr(-?\d+\.\d{2}).* PSNR \S+ LPIPS\(vgg\) (\d+\.\d{5})", ln)
        assert m, ln
        assert abs(float(m.group(2)) - sent[m.group(1)]) <= 2e-5 + DIST_RTOL * sent[m.group(1)], (ln, sent)
