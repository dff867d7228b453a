"""GPU tests of MS-SSIM (evc_amd/msssim.py, csrc/msssim.hip) against the float64 yardstick of tests/msssim_ref.py: parity of the
level means and of the values on five-level and shorter pyramids and four content kinds, level 0 against the SSIM kernel, exact
and closed-form values, batch independence bit for bit, NaN / inf, refusals, the frame helper, and --ms-ssim of the sender, the
receiver and the stitcher next to outputs that do not change."""
import contextlib
import io
import os
import re
import types

import numpy as np
import pytest
import torch

import msssim_ref as M

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(5, s, k) for s in M.SHAPES5 for k in M.KINDS] + [(n, s, k) for n, s in M.SMALL for k in M.KINDS]


@pytest.fixture(scope="module")
def S():
    import evc_amd  # noqa: F401
    from evc_amd import lib, msssim
    lib.hip_lib()
    return msssim


@pytest.mark.parametrize("levels,shape,kind", CASES)
def test_levels_and_values_against_the_float64_yardstick(S, levels, shape, kind):
    """Levels: 1e-10, some 300x the 3.4e-13 the yardstick's two forms differ by on these cases on the CPU
    (tests/test_msssim_host.py prints them) -- the margin of the SSIM test.  Values: 1e-10 where every factor is >= 0.99.  On
    noise a factor can be negative (relu: the value is exactly 0) or as small as 4e-4, where d/df f^w = w f^(w-1) <= 100: 1e-7,
    with ten-fold room.  The noise cases assert those preconditions on the yardstick itself."""
    a, b, ref = M.case(kind, shape, levels)
    w = M.WEIGHTS[:levels]
    got = S.ms_ssim_levels(a, b, levels)
    assert got.dtype == np.float64 and got.shape == (3, levels, 2)
    worst = float(np.abs(got - ref).max())
    print(f"{kind} {shape} L={levels}: |kernel - yardstick| levels = {worst:.3e}")
    assert worst <= 1e-10
    want, f = M.combine(ref, w), M.factors(ref)
    if kind != "noise":
        assert f.min() >= 0.99
        worst_v = float(np.abs(S.combine(got, w) - want).max())
        print(f"   values {want}, |kernel - yardstick| = {worst_v:.3e}")
        assert worst_v <= 1e-10
        return
    value = S.ms_ssim_planes(a, b, w)
    assert value.dtype == np.float64 and np.array_equal(value, S.combine(got, w))       # the value is combine of the levels, bit for bit
    negative = (f < 0).any(axis=-1)
    assert (f[f < 0] <= -0.006).all() and f[f >= 0].min() >= 4e-4                        # 1e-10 on a level cannot change a sign
    assert (value[negative] == 0.0).all() and (want[negative] == 0.0).all()
    worst_v = float(np.abs(value[~negative] - want[~negative]).max()) if (~negative).any() else 0.0
    print(f"   values {want}, negative factor in {negative.tolist()}, |kernel - yardstick| = {worst_v:.3e}")
    assert worst_v <= 1e-7


@pytest.mark.parametrize("levels,shape", [(5, s) for s in M.SHAPES5] + M.SMALL)
def test_level_0_against_the_ssim_kernel(S, levels, shape):
    """The same quantity in another operation order ((l * cs) against one quotient of products): 1e-12."""
    from evc_amd import ssim
    for kind in M.KINDS:
        a, b, _ = M.case(kind, shape, levels)
        worst = float(np.abs(S.ms_ssim_levels(a, b, levels)[:, 0, 0] - ssim.ssim_planes(a, b)).max())
        print(f"{kind} {shape}: |level 0 - ssim_planes| = {worst:.3e}")
        assert worst <= 1e-12


@pytest.mark.parametrize("shape", M.SHAPES5)
def test_identical_planes_give_exactly_one(S, shape):
    for kind in M.KINDS:
        a, _, _ = M.case(kind, shape)
        assert (S.ms_ssim_levels(a, a) == 1.0).all() and (S.ms_ssim_planes(a, a) == 1.0).all(), kind
    x = torch.from_numpy(M.case("noise", shape)[0]).cuda()             # device tensors are taken as they are
    assert (S.ms_ssim_levels(x, x.clone()) == 1.0).all() and (S.ms_ssim_planes(x, x.clone()) == 1.0).all()


@pytest.mark.parametrize("shape", [(176, 176), (192, 352)])
def test_constant_planes_on_even_pyramids_match_the_closed_form(S, shape):
    pairs = [(0.0, 1.0), (0.3, 0.6), (0.5, 0.5), (0.123, 0.987), (1.0, 1.0)]
    a = np.stack([np.full(shape, p, dtype=np.float32) for p, _ in pairs])
    b = np.stack([np.full(shape, q, dtype=np.float32) for _, q in pairs])
    x, y = a[:, 0, 0].astype(np.float64), b[:, 0, 0].astype(np.float64)
    lum = (2 * x * y + M.C1) / (x * x + y * y + M.C1)
    lv = S.ms_ssim_levels(a, b)
    print(f"constant planes {shape}: |cs - 1| = {np.abs(lv[..., 1] - 1).max():.3e}, |ssim - l| = {np.abs(lv[..., 0] - lum[:, None]).max():.3e}")
    assert np.abs(lv[..., 1] - 1).max() <= 1e-12 and np.abs(lv[..., 0] - lum[:, None]).max() <= 1e-12
    assert np.abs(S.ms_ssim_planes(a, b) - lum ** M.WEIGHTS[4]).max() <= 1e-12


def test_a_plane_does_not_depend_on_its_batch(S):
    """12 planes of 162x177: each alone (N = 1), inside the N = 12 launch and inside a slice of it, bit for bit."""
    rng = np.random.default_rng(3)
    a = rng.random((12, 162, 177), dtype=np.float32)
    b = np.clip(a + 0.05 * rng.standard_normal((12, 162, 177), dtype=np.float32), 0, 1)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    batch = S.ms_ssim_levels(ta, tb)
    assert batch.shape == (12, 5, 2) and np.array_equal(batch, S.ms_ssim_levels(ta, tb))
    alone = np.stack([S.ms_ssim_levels(ta[i:i + 1], tb[i:i + 1])[0] for i in range(12)])
    assert np.array_equal(alone, batch)
    assert np.array_equal(S.ms_ssim_levels(ta[4:9], tb[4:9]), batch[4:9])             # another N, another place in the batch
    assert np.isfinite(batch).all() and len(set(batch[:, 0, 0].tolist())) == 12


def test_non_finite_values_stay_in_their_plane(S):
    a, b = M.content("noisy_copy", (162, 177), planes=5)
    clean = S.ms_ssim_levels(a, b)
    a2, b2 = a.copy(), b.copy()
    a2[1, 80, 90] = np.nan
    b2[2, 0, 176] = np.inf
    got, ref = S.ms_ssim_levels(a2, b2), M.ms_ssim_levels(a2[:3], b2[:3])
    assert np.array_equal(np.isnan(got[:3]), np.isnan(ref))                           # every level sees the value: every level NaN
    assert np.isnan(got[1]).all() and np.isnan(got[2]).all()
    assert np.array_equal(got[[0, 3, 4]], clean[[0, 3, 4]]) and np.isfinite(clean).all()
    value = S.ms_ssim_planes(a2, b2)
    assert np.isnan(value).tolist() == [False, True, True, False, False]


def test_refusals(S):
    from evc_amd import lib as L
    so = L.hip_lib()
    x = torch.zeros((1, 41, 45), device="cuda")
    from evc_amd import ssim
    taps = torch.from_numpy(ssim.gaussian_taps()).cuda()
    out = torch.full((3, 2), 7.0, dtype=torch.float64, device="cuda")
    ws = torch.zeros(max(1, so.evc_msssim_workspace_bytes(1, 41, 45, 3) // 8), dtype=torch.float64, device="cuda")
    args = lambda n, h, w, lv: (L.fptr(x), L.fptr(x), n, h, w, lv, L.ptr(taps), S.C1, S.C2, L.ptr(out), L.ptr(ws), L.stream_ptr())  # noqa: E731
    f = so.evc_msssim_levels_f32
    assert f(*args(1, 40, 45, 3)) < 0 and f(*args(1, 45, 40, 3)) < 0 and f(*args(-1, 41, 45, 3)) < 0
    assert f(*args(1, 41, 45, 0)) < 0 and f(*args(1, 41, 45, 9)) < 0 and f(*args(1, 41, 45, 4)) < 0
    assert f(L.fptr(x), None, 1, 41, 45, 3, L.ptr(taps), S.C1, S.C2, L.ptr(out), L.ptr(ws), L.stream_ptr()) < 0
    assert f(None, None, 0, 41, 45, 3, None, S.C1, S.C2, None, None, L.stream_ptr()) == 0
    assert so.evc_msssim_workspace_bytes(1, 40, 45, 3) < 0 and so.evc_msssim_workspace_bytes(0, 41, 45, 3) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                # nothing was launched
    assert f(*args(1, 41, 45, 3)) == 0
    torch.cuda.synchronize()
    assert bool((out == 1.0).all())                                # zeros against zeros
    for shape in ((2, 160, 200), (2, 200, 160)):
        with pytest.raises(ValueError, match="larger than 160"):
            S.ms_ssim_planes(torch.zeros(shape, device="cuda"), torch.zeros(shape, device="cuda"))
    with pytest.raises(ValueError):
        S.ms_ssim_planes(torch.zeros((2, 161, 161), device="cuda"), torch.zeros((2, 161, 162), device="cuda"))
    empty = S.ms_ssim_planes(np.zeros((0, 3, 161, 161), dtype=np.float32), np.zeros((0, 3, 161, 161), dtype=np.float32))
    assert empty.shape == (0, 3) and empty.dtype == np.float64


def test_frames_are_the_channel_mean(S):
    rng = np.random.default_rng(8)
    v1 = rng.random((4, 3, 162, 177), dtype=np.float32)
    v2 = np.clip(v1 + 0.1 * rng.standard_normal(v1.shape, dtype=np.float32), 0, 1)
    planes = S.ms_ssim_planes(v1, v2)
    frames = S.ms_ssim_frames(v1, v2)
    assert planes.shape == (4, 3) and frames.shape == (4,) and np.array_equal(frames, planes.mean(axis=-1))
    assert np.array_equal(S.ms_ssim_frames(v1[:, :1], v2[:, :1]), planes[:, 0])        # grey: plane 0
    assert np.array_equal(S.ms_ssim_frames(torch.from_numpy(v1), torch.from_numpy(v2).cuda()), frames)
    assert ((frames > 0.5) & (frames < 1)).all()


# ---- the command lines ----------------------------------------------------------------------------------------------

H, W = 176, 192                                       # 2 x 2 tiles of 128x128; 176 -> 88 -> 44 -> 22 -> 11
MODEL = ["--synthetic", "--config_mod", "model.ngf=32 model.n_head_channels=32"]


def captured(main, argv):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        main(argv)
    return buf.getvalue()


def clip_of(half):
    """The sender's saved picture (H, 30 W, 3), frames side by side -> (30, 3, H, W)."""
    return np.ascontiguousarray(np.stack([half[:, f * W:(f + 1) * W].transpose(2, 0, 1) for f in range(30)]))


@pytest.fixture(scope="module")
def sender_runs(tmp_path_factory):
    """city_sender.py --data_yuv clip.y4m --yuv-fit joint on a 192x176 file of block-replicated noise, in process, with the
    reduced generator of tests/test_gpu_canvas.py: with --ssim --ms-ssim (and job streams), the same without --ms-ssim, and
    key frames only with --ms-ssim --yuv-metrics."""
    import evc_amd  # noqa: F401
    from evc_amd import cli, video_io as V
    tmp = tmp_path_factory.mktemp("msssim_cli")
    small = np.random.default_rng(11).random((30, 3, H // 16, W // 16), dtype=np.float32)
    V.write_clip(str(tmp / "clip.y4m"), np.repeat(np.repeat(small, 16, axis=2), 16, axis=3), 30)
    log = {}

    def run(name, extra, thresholds=("0.0", "200.0")):
        log[name] = captured(cli.main, ["--config", os.path.join(REPO, "configs", "mine.yml"), "--exp", str(tmp / f"exp_{name}"),
                                        "--data_yuv", str(tmp / "clip.y4m"), "--yuv-fit", "joint", "--output_path", str(tmp / name),
                                        "--start_idx", "0", "--end_idx", "0", "--subsample", "2", "--q", "3", "--policy", "psnr",
                                        "--thresholds", *thresholds, "--bpp-limit", "1e9", "--batch-invariant"] + MODEL + extra)

    with pytest.MonkeyPatch.context() as mp:
        mp.chdir(tmp)
        run("with", ["--ssim", "--ms-ssim", "--bitstream-dir", str(tmp / "bits_with")])
        run("without", ["--ssim", "--bitstream-dir", str(tmp / "bits_without")])
        run("yuv", ["--ms-ssim", "--yuv-metrics"], thresholds=("200.0",))
    return types.SimpleNamespace(tmp=tmp, log=log)


def test_sender_writes_ms_ssim_next_to_unchanged_outputs(S, sender_runs):
    tmp = sender_runs.tmp
    d, d0 = tmp / "with" / "output_0", tmp / "without" / "output_0"
    frames, env = np.load(d / "ms_ssim_frames_0.npy"), np.load(d / "ms_ssim_0.npy")
    assert frames.shape == (2, 30) and frames.dtype == np.float64 and env.dtype == np.float64
    assert np.isfinite(frames).all() and (frames >= 0).all() and (frames <= 1).all()
    assert env.shape[0] == 2 and np.isfinite(env).all()
    printed = re.findall(r"MS-SSIM: (-?\d+\.\d{5}) \((-?\d+\.\d\d|inf) dB\)", sender_runs.log["with"])
    assert [p[0] for p in printed] == ["%.5f" % v for v in frames.mean(axis=1)]
    assert [p[1] for p in printed] == ["%.2f" % S.to_db(v) for v in frames.mean(axis=1)]
    # without the flag: no line, no file; every other file and line is what it is with it
    assert "MS-SSIM" not in sender_runs.log["without"] and not list(d0.glob("ms_ssim*"))
    assert sorted(p.name for p in d.iterdir()) == sorted([p.name for p in d0.iterdir()] + ["ms_ssim_0.npy", "ms_ssim_frames_0.npy"])
    for f in sorted(p.name for p in d0.iterdir()):
        assert (d / f).read_bytes() == (d0 / f).read_bytes(), f
    for f in sorted(os.listdir(tmp / "bits_without")):
        assert (tmp / "bits_with" / f).read_bytes() == (tmp / "bits_without" / f).read_bytes(), f
    assert sorted(os.listdir(tmp / "bits_with")) == sorted(os.listdir(tmp / "bits_without"))
    drop = lambda text: [ln.replace("_without", "_X").replace("_with", "_X").replace(str(tmp / "without"), "OUT").replace(str(tmp / "with"), "OUT")  # noqa: E731
                         for ln in text.splitlines() if "MS-SSIM" not in ln and not ln.startswith("done in")]
    assert drop(sender_runs.log["with"]) == drop(sender_runs.log["without"])
    args_yml = lambda name: open(tmp / f"exp_{name}" / "video_samples" / "arg_config" / "args.yml").read()  # noqa: E731
    assert "ms_ssim: true" in args_yml("with") and "ms_ssim" not in args_yml("without")
    # the saved values are the API's for the frames the run saved, bit for bit (upper half: originals, lower half: decoded)
    order = [float(re.search(r"thr (-?\d+\.\d\d):", ln).group(1)) for ln in sender_runs.log["with"].splitlines() if "MS-SSIM:" in ln]
    assert sorted(order) == [0.0, 200.0]
    for job, thr in enumerate(order):
        img = np.load(d / ("city_output_npy_idx0_q3_thr%.2f.npy" % thr))
        assert img.shape == (2 * H, 30 * W, 3)
        gt, x = clip_of(img[:H]), clip_of(img[H:])
        assert np.array_equal(frames[job], S.ms_ssim_frames(x, gt)), thr
        if thr == 0.0:           # and the levels are the yardstick's (three frames: a key frame and two generated ones)
            pick = [0, 2, 29]
            worst = float(np.abs(S.ms_ssim_levels(x[pick], gt[pick]) - M.ms_ssim_levels(x[pick], gt[pick])).max())
            print(f"saved frames {pick}: |kernel - yardstick| levels = {worst:.3e}, MS-SSIM {frames[job][pick]}")
            assert worst <= 1e-10
            assert not np.array_equal(x[29], gt[29])


def test_yuv_metrics_gain_ms_ssim_on_the_clips_psnr_yuv_compares(S, sender_runs):
    from evc_amd import video_io as V
    d = sender_runs.tmp / "yuv" / "output_0"
    names = sorted(p.name for p in d.iterdir() if p.name.startswith(("ssim", "ms_ssim", "psnr_yuv")))
    assert names == sorted(["ms_ssim_0.npy", "ms_ssim_frames_0.npy", "ms_ssim_yuv_0.npy", "ms_ssim_yuv_frames_0.npy",
                            "psnr_yuv_0.npy", "psnr_yuv_frames_0.npy"])
    img = np.load(d / "city_output_npy_idx0_q3_thr200.00.npy")
    gt, x = clip_of(img[:H]), clip_of(img[H:])
    a, b = V.yuv_metric_clips(x, gt)
    got = np.load(d / "ms_ssim_yuv_frames_0.npy")
    assert got.shape == (1, 30) and got.dtype == np.float64 and np.load(d / "ms_ssim_yuv_0.npy").shape[0] == 2
    want = S.ms_ssim_frames(b.astype(np.float32) / np.float32(255), a.astype(np.float32) / np.float32(255))
    assert np.array_equal(got[0], want) and np.array_equal(got[0], V.ms_ssim_yuv(x, gt))
    assert np.array_equal(np.load(d / "ms_ssim_frames_0.npy")[0], S.ms_ssim_frames(x, gt))
    assert not np.array_equal(got, np.load(d / "ms_ssim_frames_0.npy"))          # the 8-bit 4:2:0 round trip is another pair of clips


def test_receiver_prints_ms_ssim_only_when_asked(S, sender_runs, capsys):
    from evc_amd import receiver
    tmp = sender_runs.tmp
    sent = {float(t): float(v) for t, v in re.findall(r"thr (-?\d+\.\d\d): MS-SSIM: (-?\d+\.\d{5})", sender_runs.log["with"])}

    def run(out, extra):
        receiver.main(["--config", os.path.join(REPO, "configs", "mine.yml"), "--exp", str(tmp / "exp_rx"), "--data_yuv",
                       str(tmp / "clip.y4m"), "--yuv-fit", "joint", "--bitstream-dir", str(tmp / "bits_with"), "--output_path",
                       str(tmp / out)] + MODEL + extra)
        return sorted(ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("job_"))

    with_flag, plain = run("rx_ms", ["--ssim", "--ms-ssim"]), run("rx", ["--ssim"])
    assert len(with_flag) == len(plain) == 2
    for a, b in zip(with_flag, plain):
        assert " SSIM " in b and "MS-SSIM" not in b and b.endswith(", frames: match")
        m = re.fullmatch(r"(.* SSIM -?\d+\.\d{5}) MS-SSIM (-?\d+\.\d{5})(, frames: match)", a)
        assert m and m.group(1) + m.group(3) == b, (a, b)
        thr = float(re.search(r"thr(-?\d+\.\d\d)\.evc", a).group(1))
        assert float(m.group(2)) == sent[thr]                   # frames: match -- the sender's frames, the sender's value
    assert sorted(os.listdir(tmp / "rx")) == sorted(os.listdir(tmp / "rx_ms")) and len(os.listdir(tmp / "rx")) == 2
    for name in os.listdir(tmp / "rx"):
        assert (tmp / "rx" / name).read_bytes() == (tmp / "rx_ms" / name).read_bytes()


def test_frames_of_the_models_size_end_the_run_before_generating(S, tmp_path, capsys):
    from evc_amd import cli
    with pytest.MonkeyPatch.context() as mp:
        mp.chdir(tmp_path)
        with pytest.raises(SystemExit) as e:
            cli.main(["--config", os.path.join(REPO, "configs", "mine.yml"), "--exp", str(tmp_path / "exp"), "--output_path",
                      str(tmp_path / "out"), "--start_idx", "0", "--end_idx", "0", "--subsample", "2", "--q", "3", "--policy", "psnr",
                      "--thresholds", "0.0", "--ms-ssim"] + MODEL)
    text = str(e.value.code)
    assert e.value.code not in (0, None) and "128x128" in text and "> 160" in text
    assert "--yuv-fit joint" in text and "city_stitch.py --ms-ssim" in text
    assert "BPP" not in capsys.readouterr().out and not os.path.exists(tmp_path / "out" / "output_0")       # no job was run


def test_stitcher_reports_ms_ssim_of_the_whole_frames(S, sender_runs, tmp_path):
    """Hand-written decoded tiles of a 2 x 2 grid over the 192x176 source (the source plus noise, cut at the manifest's
    origins); no generation."""
    from evc_amd import stitch, video_io as V
    src = V.read_clips(str(sender_runs.tmp / "clip.y4m"), frames=30)
    assert src.shape == (1, 30, 3, H, W) and src.dtype == np.uint8
    gt = src[0].astype(np.float32) / 255.0
    noisy = np.clip(gt + 0.03 * np.random.default_rng(4).standard_normal(gt.shape, dtype=np.float32), 0, 1).astype(np.float32)
    m = V.tile_manifest(W, H, 128, 16, 1, 30, 30, "clip.y4m")
    V.write_manifest(str(tmp_path), m)
    assert (m["ny"], m["nx"]) == (2, 2)
    os.makedirs(tmp_path / "rx")
    for t, (oy, ox) in enumerate((y, x) for y in m["oy"] for x in m["ox"]):
        np.save(tmp_path / "rx" / f"decoded_v{t}_q3_thr0.50.npy", noisy[:, :, oy:oy + 128, ox:ox + 128])
    base = ["--tiles", str(tmp_path / "tiles.json"), "--decoded", str(tmp_path / "rx"), "--data_yuv", str(sender_runs.tmp / "clip.y4m")]
    line = lambda text: [ln for ln in text.splitlines() if ln.startswith("stitched_c0_q3_thr0.50:")]  # noqa: E731
    (plain,) = line(captured(stitch.main, base + ["--output_path", str(tmp_path / "full"), "--ssim"]))
    (asked,) = line(captured(stitch.main, base + ["--output_path", str(tmp_path / "full_ms"), "--ssim", "--ms-ssim"]))
    m2 = re.fullmatch(re.escape(plain) + r" MS-SSIM (-?\d+\.\d{5})", asked)
    assert m2 and " SSIM " in plain and "MS-SSIM" not in plain, (plain, asked)
    full = np.load(tmp_path / "full_ms" / "stitched_c0_q3_thr0.50.npy")
    assert full.shape == (30, 3, H, W) and full.dtype == np.float32
    assert m2.group(1) == "%.5f" % S.ms_ssim_frames(full, gt).mean() and 0.5 < float(m2.group(1)) < 1
    assert (tmp_path / "full" / "stitched_c0_q3_thr0.50.npy").read_bytes() == (tmp_path / "full_ms" / "stitched_c0_q3_thr0.50.npy").read_bytes()
    # a grid of frames too small for five levels is refused before anything is stitched
    V.write_manifest(str(tmp_path / "small"), V.tile_manifest(160, 144, 128, 16, 1, 30, 30, "clip.y4m"))
    with pytest.raises(SystemExit) as e:
        stitch.main(["--tiles", str(tmp_path / "small" / "tiles.json"), "--decoded", str(tmp_path / "rx"), "--output_path",
                     str(tmp_path / "none"), "--ms-ssim"])
    assert "160x144" in str(e.value.code) and "> 160" in str(e.value.code) and not os.path.exists(tmp_path / "none")
