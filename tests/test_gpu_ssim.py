"""GPU tests of SSIM (evc_amd/ssim.py, csrc/ssim.hip) against the float64 yardstick of tests/ssim_ref.py: parity on four shapes
and four content kinds, exact and closed-form values, batch independence bit for bit, NaN / inf, refusals, the frame and video
helpers, and --ssim of the sender and the receiver next to outputs that do not change."""
import os
import re
import types

import numpy as np
import pytest
import torch

import ssim_ref as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(k, s) for s in R.SHAPES for k in R.KINDS]


@pytest.fixture(scope="module")
def S():
    import evc_amd  # noqa: F401
    from evc_amd import lib, ssim
    lib.hip_lib()
    return ssim


@pytest.mark.parametrize("kind,shape", CASES)
def test_parity_with_the_float64_yardstick(S, kind, shape):
    """1e-10: 270x the largest difference two float64 summation orders show on these cases on the CPU (3.7e-13, nearly flat
    11x11; tests/test_ssim_host.py prints them), six orders of magnitude below an fp32 evaluation's 1.6e-4."""
    a, b = R.content(kind, shape)
    got, ref = S.ssim_planes(a, b), R.ssim_planes(a, b)
    assert got.dtype == np.float64 and got.shape == (3,)
    worst = float(np.abs(got - ref).max())
    print(f"{kind} {shape}: |kernel - yardstick| = {worst:.3e}, values {ref}")
    assert worst <= 1e-10


@pytest.mark.parametrize("shape", R.SHAPES)
def test_identical_planes_give_exactly_one(S, shape):
    for kind in R.KINDS:
        a, _ = R.content(kind, shape)
        assert (S.ssim_planes(a, a) == 1.0).all(), kind
    x = torch.from_numpy(R.content("noise", shape)[0]).cuda()          # device tensors are taken as they are
    assert (S.ssim_planes(x, x.clone()) == 1.0).all()


def test_constant_planes_match_the_closed_form(S):
    pairs = [(0.0, 1.0), (0.3, 0.6), (0.5, 0.5), (0.123, 0.987), (1.0, 1.0)]
    for shape in ((12, 17), (34, 70)):
        a = np.stack([np.full(shape, p, dtype=np.float32) for p, _ in pairs])
        b = np.stack([np.full(shape, q, dtype=np.float32) for _, q in pairs])
        x, y = a[:, 0, 0].astype(np.float64), b[:, 0, 0].astype(np.float64)
        want = (2 * x * y + R.C1) / (x * x + y * y + R.C1)
        got = S.ssim_planes(a, b)
        print(f"constant planes {shape}: |kernel - closed form| = {np.abs(got - want).max():.3e}")
        assert np.abs(got - want).max() <= 1e-12


def test_a_plane_does_not_depend_on_its_batch(S):
    """90 planes (one 30-frame clip): each alone (N = 1) and inside the N = 90 launch, bit for bit; two launches likewise."""
    rng = np.random.default_rng(3)
    a = rng.random((90, 34, 70), dtype=np.float32)
    b = np.clip(a + 0.05 * rng.standard_normal((90, 34, 70), dtype=np.float32), 0, 1)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    batch = S.ssim_planes(ta, tb)
    assert np.array_equal(batch, S.ssim_planes(ta, tb))
    alone = np.array([S.ssim_planes(ta[i:i + 1], tb[i:i + 1])[0] for i in range(90)])
    assert np.array_equal(alone, batch)
    assert np.array_equal(S.ssim_planes(ta[40:47], tb[40:47]), batch[40:47])        # another N, another place in the batch
    assert len(set(batch.tolist())) == 90


def test_non_finite_values_stay_in_their_plane(S):
    a, b = R.content("noisy_copy", (34, 70), planes=5)
    clean = S.ssim_planes(a, b)
    a2, b2 = a.copy(), b.copy()
    a2[1, 20, 33] = np.nan
    b2[2, 0, 69] = np.inf
    got, ref = S.ssim_planes(a2, b2), R.ssim_planes(a2, b2)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(got).tolist() == [False, True, True, False, False]
    assert np.array_equal(got[[0, 3, 4]], clean[[0, 3, 4]]) and np.isfinite(clean).all()


def test_refusals(S):
    from evc_amd import lib as L
    so = L.hip_lib()
    x = torch.zeros((1, 16, 16), device="cuda")
    taps = torch.from_numpy(S.gaussian_taps()).cuda()
    out, ws = torch.zeros(1, dtype=torch.float64, device="cuda"), torch.zeros(8, dtype=torch.float64, device="cuda")
    args = lambda n, h, w: (L.fptr(x), L.fptr(x), n, h, w, L.ptr(taps), S.C1, S.C2, L.ptr(out), L.ptr(ws), L.stream_ptr())  # noqa: E731
    assert so.evc_ssim_planes_f32(*args(1, 10, 16)) < 0 and so.evc_ssim_planes_f32(*args(1, 16, 10)) < 0
    assert so.evc_ssim_planes_f32(*args(-1, 16, 16)) < 0
    assert so.evc_ssim_planes_f32(L.fptr(x), None, 1, 16, 16, L.ptr(taps), S.C1, S.C2, L.ptr(out), L.ptr(ws), L.stream_ptr()) < 0
    assert so.evc_ssim_planes_f32(None, None, 0, 16, 16, None, S.C1, S.C2, None, None, L.stream_ptr()) == 0
    assert so.evc_ssim_workspace_bytes(1, 10, 16) < 0 and so.evc_ssim_workspace_bytes(1, 16, 10) < 0
    assert so.evc_ssim_planes_f32(*args(1, 16, 16)) == 0
    torch.cuda.synchronize()
    assert float(out[0]) == 1.0                                    # zeros against zeros
    for shape in ((2, 10, 16), (2, 16, 10)):
        with pytest.raises(ValueError):
            S.ssim_planes(torch.zeros(shape, device="cuda"), torch.zeros(shape, device="cuda"))
    with pytest.raises(ValueError):
        S.ssim_planes(torch.zeros((2, 16, 16), device="cuda"), torch.zeros((2, 16, 17), device="cuda"))
    empty = S.ssim_planes(np.zeros((0, 3, 16, 16), dtype=np.float32), np.zeros((0, 3, 16, 16), dtype=np.float32))
    assert empty.shape == (0, 3) and empty.dtype == np.float64


def test_frames_and_videos(S):
    rng = np.random.default_rng(8)
    v1 = rng.random((2, 6, 3, 34, 70), dtype=np.float32)
    v2 = np.clip(v1 + 0.1 * rng.standard_normal(v1.shape, dtype=np.float32), 0, 1)
    planes = S.ssim_planes(v1[0, :4], v2[0, :4])
    assert planes.shape == (4, 3)
    frames = S.ssim_frames(v1[0, :4], v2[0, :4])
    assert frames.shape == (4,) and np.array_equal(frames, planes.mean(axis=-1))
    grey = S.ssim_frames(v1[0, :4, :1], v2[0, :4, :1])
    assert np.array_equal(grey, planes[:, 0])
    got = S.calculate_ssim(torch.from_numpy(v1), torch.from_numpy(v2), 2, True)
    ref = R.calculate_ssim(v1, v2, 2, True)
    assert list(got) == list(ref) and got["ssim_per_frame"] == 2 and tuple(got["ssim_video_setting"]) == (6, 3, 34, 70)
    assert got["ssim_video_setting_name"] == ref["ssim_video_setting_name"]
    for part in ("ssim", "ssim_std"):
        assert list(got[part]) == list(ref[part]) and len(got[part]) == 4
        for k in ref[part]:
            assert abs(got[part][k] - ref[part][k]) <= 1e-10, (part, k)


# ---- the command lines ----------------------------------------------------------------------------------------------

MODEL = ["--synthetic", "--config_mod", "model.ngf=32 model.n_head_channels=32"]


@pytest.fixture(scope="module")
def sender_runs(tmp_path_factory):
    """The sweep of tests/test_gpu_fvd.py::test_cli_writes_fvd_next_to_unchanged_outputs, in process: once with --ssim, once
    without; and one all-generated job written as a job stream for the receiver."""
    import evc_amd  # noqa: F401
    from evc_amd import cli, synthetic
    tmp = tmp_path_factory.mktemp("ssim_cli")
    np.save(tmp / "clips.npy", synthetic.make_clips(1, seed=1234))
    mp, capfd_text = pytest.MonkeyPatch(), {}
    mp.chdir(tmp)
    import contextlib
    import io

    def run(name, extra, thresholds=("200", "-100")):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            cli.main(["--config", os.path.join(REPO, "configs", "mine.yml"), "--exp", str(tmp / "exp"), "--data_npy",
                      str(tmp / "clips.npy"), "--output_path", str(tmp / name), "--start_idx", "0", "--end_idx", "0", "--subsample",
                      "2", "--q", "3", "--policy", "psnr", "--thresholds", *thresholds, "--bpp-limit", "1e9"] + MODEL + extra)
        capfd_text[name] = buf.getvalue()

    try:
        run("with", ["--ssim"])
        run("without", [])
        run("stream", ["--ssim", "--bitstream-dir", str(tmp / "bits")], thresholds=("-100",))
        run("yuv", ["--ssim", "--yuv-metrics"], thresholds=("-100",))
    finally:
        mp.undo()
    return types.SimpleNamespace(tmp=tmp, log=capfd_text)


def test_sender_writes_ssim_next_to_unchanged_outputs(sender_runs):
    d, d0 = sender_runs.tmp / "with" / "output_0", sender_runs.tmp / "without" / "output_0"
    frames, env = np.load(d / "ssim_frames_0.npy"), np.load(d / "ssim_0.npy")
    assert frames.shape == (2, 30) and frames.dtype == np.float64
    assert np.isfinite(frames).all() and (frames > -1).all() and (frames <= 1).all()
    assert env.shape[0] == 2 and np.isfinite(env).all()
    printed = [float(m) for m in re.findall(r"SSIM: (-?\d+\.\d{5})\b", sender_runs.log["with"])]
    assert printed == [float("%.5f" % v) for v in frames.mean(axis=1)]
    assert "SSIM" not in sender_runs.log["without"] and not list(d0.glob("ssim*"))
    for f in sorted(p.name for p in d0.iterdir()):
        if f.endswith(".npy"):
            assert (d / f).read_bytes() == (d0 / f).read_bytes(), f
    assert sorted(p.name for p in d.iterdir()) == sorted([p.name for p in d0.iterdir()] + ["ssim_0.npy", "ssim_frames_0.npy"])
    tmp = sender_runs.tmp
    drop = lambda text: [ln.replace(str(tmp / "without"), "OUT").replace(str(tmp / "with"), "OUT")  # noqa: E731
                         for ln in text.splitlines() if "SSIM" not in ln and not ln.startswith("done in")]
    assert drop(sender_runs.log["with"]) == drop(sender_runs.log["without"])
    # the values are the yardstick's for the frames the run saved (upper half: originals, lower half: decoded frames)
    img = np.load(d / "city_output_npy_idx0_q3_thr-100.00.npy")
    clip = lambda half: np.stack([half[:, f * 128:(f + 1) * 128].transpose(2, 0, 1) for f in range(30)])  # noqa: E731
    job = ["thr -100.00" in ln for ln in sender_runs.log["with"].splitlines() if "SSIM:" in ln].index(True)
    ref = R.ssim_planes(clip(img[128:]), clip(img[:128])).mean(axis=-1)
    assert np.abs(frames[job] - ref).max() <= 1e-10


def test_yuv_metrics_gain_ssim_on_the_clips_psnr_yuv_compares(sender_runs):
    from evc_amd import video_io as V
    d = sender_runs.tmp / "yuv" / "output_0"
    names = sorted(p.name for p in d.iterdir() if p.name.startswith(("ssim", "psnr_yuv")))
    assert names == sorted(["ssim_0.npy", "ssim_frames_0.npy", "ssim_yuv_0.npy", "ssim_yuv_frames_0.npy", "psnr_yuv_0.npy",
                            "psnr_yuv_frames_0.npy"])
    img = np.load(d / "city_output_npy_idx0_q3_thr-100.00.npy")
    clip = lambda half: np.stack([half[:, f * 128:(f + 1) * 128].transpose(2, 0, 1) for f in range(30)])  # noqa: E731
    gt, x = clip(img[:128]), clip(img[128:])
    a, b = V.yuv_metric_clips(x, gt)
    assert a.dtype == b.dtype == np.uint8 and a.shape == b.shape == (30, 3, 128, 128)
    assert np.array_equal(a, V.yuv_round_trip_u8(gt)) and np.array_equal(b, V.yuv_round_trip_u8(x))
    psnr = np.load(d / "psnr_yuv_frames_0.npy")
    assert np.array_equal(psnr[0], V.psnr_u8(a, b)) and np.array_equal(psnr[0], V.psnr_yuv(x, gt))
    got = np.load(d / "ssim_yuv_frames_0.npy")
    assert got.shape == (1, 30) and np.load(d / "ssim_yuv_0.npy").shape[0] == 2
    ref = R.ssim_planes(b.astype(np.float32) / np.float32(255), a.astype(np.float32) / np.float32(255)).mean(axis=-1)
    assert np.abs(got[0] - ref).max() <= 1e-10
    assert not np.array_equal(got, np.load(d / "ssim_frames_0.npy"))          # the 8-bit 4:2:0 round trip is another pair of clips


def test_receiver_prints_ssim_only_when_asked(sender_runs, capsys):
    from evc_amd import receiver
    tmp = sender_runs.tmp
    assert len(os.listdir(tmp / "bits")) == 1
    sent = float(re.search(r"SSIM: (-?\d+\.\d{5})", sender_runs.log["stream"]).group(1))

    def run(out, extra):
        receiver.main(["--config", os.path.join(REPO, "configs", "mine.yml"), "--exp", str(tmp / "exp"), "--data_npy",
                       str(tmp / "clips.npy"), "--bitstream-dir", str(tmp / "bits"), "--output_path", str(tmp / out)] + MODEL + extra)
        return [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("job_")]

    with_flag, plain = run("rx_ssim", ["--ssim"]), run("rx", [])
    assert len(with_flag) == len(plain) == 1 and " PSNR " in plain[0] and "SSIM" not in plain[0]
    m = re.fullmatch(re.escape(plain[0]) + r" SSIM (-?\d+\.\d{5})", with_flag[0])
    assert m, (plain[0], with_flag[0])
    assert abs(float(m.group(1)) - sent) <= 2e-5           # same launch shapes as the sender: the same frames, the same value
    name = "decoded_v0_q3_thr-100.00.npy"
    assert os.listdir(tmp / "rx") == os.listdir(tmp / "rx_ssim") == [name]
    assert (tmp / "rx" / name).read_bytes() == (tmp / "rx_ssim" / name).read_bytes()
