"""GPU tests of csrc/yuv.hip (evc_yuv420_to_rgb, evc_rgb_to_yuv420) against the float64 fixture the reference's own transforms
produced (tests/golden/yuv_transform.npz) and the float64 restatement tests/yuv_ref.py, and of the command lines that read and
write video files.

The two bars, used by every test here:

  float form    max |out - float64 golden| <= 2e-6.  Derivation: the kernel does about 16 fp32 roundings (two 4-tap filters,
                three divisions by maxv, the three lines of ycbcr2rgb with their products) of values up to 1.5, whose ulp is
                1.2e-7 / 2 per rounding at most: 16 * 6e-8 * 1.5 = 1.4e-6.  torch's own fp32 evaluation of the reference lies
                1.5e-7 .. 2.9e-7 from float64.  The fixture stores the golden on a grid of 2^-22 (tests/golden/make_yuv_golden.py),
                so GRID / 2 = 1.2e-7 is taken OFF the bar where the fixture is the reference: 1.88e-6.
  integer form  the code equals the float64 golden's code wherever the golden's pre-rounding value is farther than
                delta = maxv * 1e-6 from a rounding tie (7x the fp32-against-fp64 difference of the pre-rounding values measured on
                the reference: 3.4e-5 code units at 8 bits, 1.4e-4 at 10); inside that band it may differ by 1; the band may hold
                at most 1 % of a case's samples.  Where the pre-rounding value comes from the stored grid, its rounding
                (255 * GRID / 2 = 3.1e-5 code units) is taken off delta, which only narrows the band.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import yuv_ref as YR
from conftest import golden

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 2), (12, 16), (18, 34), (32, 48)]
MODES = ("nearest", "bilinear", "bicubic")
GRID, OFFSET = 2.0 ** -22, 1.5
FLOAT_BAR = 2e-6
Y4M_LEAD = b"YUV4MPEG2 W34 H18 F120:4 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n"    # 59 bytes: with the marker every frame at an odd address
assert len(Y4M_LEAD) == 59


@pytest.fixture(scope="module")
def L():
    import evc_amd  # noqa: F401
    from evc_amd import lib
    lib.hip_lib()
    return lib


@pytest.fixture(scope="module")
def G():
    return golden("yuv_transform")


def golden_rgb(G, mode, H, W, bits):
    b = G[f"rgb_{mode}_{H}x{W}_{bits}"].astype(np.int64)
    return (b[0] + 256 * b[1] + 65536 * b[2]) * GRID - OFFSET


def upload(blob):
    return torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()


def check_codes(got, want, band, what):
    """The integer bar.  -> (samples in the band, samples)."""
    got, want = np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)
    assert got.shape == want.shape, what
    diff = np.abs(got - want)
    print(f"{what}: {int((diff != 0).sum())} of {diff.size} codes differ, {int(band.sum())} in the tie band")
    assert not diff[~band].any(), (what, "a code differs away from a rounding tie")
    assert diff.max(initial=0) <= 1, what
    return int(band.sum()), band.size


def layouts(y, u, v, bits):
    """The same frames as a packed raw buffer and as a Y4M file (header, FRAME markers): (name, bytes, first, stride)."""
    raw, first, stride = YR.frame_buffer(y, u, v, bits)
    yield "raw", raw, first, stride
    y4m, first, stride = YR.frame_buffer(y, u, v, bits, lead=Y4M_LEAD, marker=YR.FRAME_MARK)
    assert first == len(Y4M_LEAD) + 6 and first % 2 == 1
    yield "y4m", y4m, first, stride


# ---- evc_yuv420_to_rgb ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", SHAPES)
def test_yuv420_to_rgb_float_within_2e_6_of_the_float64_golden(L, G, H, W):
    """Every fixture case (8 / 10 bits x nearest / bilinear / bicubic), from a packed buffer and from a Y4M-style buffer with a
    non-zero, odd first-frame offset and markers between the frames.  Bar: module docstring, float form."""
    worst = 0.0
    for bits in (8, 10):
        y, u, v = (G[f"yuv_{p}_{H}x{W}_{bits}"] for p in "yuv")
        for name, blob, first, stride in layouts(y, u, v, bits):
            buf = upload(blob)
            for mode in MODES:
                out = L.yuv420_to_rgb(buf, 2, H, W, bits, mode, first=first, stride=stride)
                assert out.shape == (2, 3, H, W) and out.dtype == torch.float32
                err = float(np.abs(out.cpu().numpy().astype(np.float64) - golden_rgb(G, mode, H, W, bits)).max())
                print(f"{H}x{W} {bits}-bit {mode} {name}: max |out - golden| = {err:.3e}")
                worst = max(worst, err)
    assert worst <= FLOAT_BAR - GRID / 2, worst
    assert L.range_events() == 0


@pytest.mark.parametrize("H,W", SHAPES)
def test_yuv420_to_rgb_uint8_codes(L, G, H, W):
    """The uint8 form, rint(clamp(rgb * 255, 0, 255)).  Bar: module docstring, integer form."""
    delta = 255e-6 - 255 * GRID / 2
    for bits in (8, 10):
        y, u, v = (G[f"yuv_{p}_{H}x{W}_{bits}"] for p in "yuv")
        for name, blob, first, stride in layouts(y, u, v, bits):
            buf = upload(blob)
            for mode in MODES:
                out = L.yuv420_to_rgb(buf, 2, H, W, bits, mode, first=first, stride=stride, dtype=torch.uint8)
                assert out.dtype == torch.uint8
                want, pre = YR.rgb_u8(golden_rgb(G, mode, H, W, bits))
                k, n = check_codes(out.cpu().numpy(), want, YR.tie_band(pre, delta), f"{H}x{W} {bits}-bit {mode} {name} uint8")
                assert k <= 0.01 * n


def test_unaligned_output_takes_the_scalar_path_with_the_same_bits(L, G):
    """W % 8 == 0 but an output pointer off the 16-byte grid: the vector stores are not used, the numbers are the same."""
    H, W, bits = 32, 48, 8
    buf = upload(YR.frame_buffer(*(G[f"yuv_{p}_{H}x{W}_{bits}"] for p in "yuv"), bits)[0])
    for dtype in (torch.float32, torch.uint8):
        ref = L.yuv420_to_rgb(buf, 2, H, W, bits, "bicubic", dtype=dtype)
        flat = torch.zeros(2 * 3 * H * W + 2, dtype=dtype, device="cuda")
        out = L.yuv420_to_rgb(buf, 2, H, W, bits, "bicubic", dtype=dtype, out=flat[1:-1].view(2, 3, H, W))
        assert out.data_ptr() % 8 != 0 and torch.equal(out, ref)
        assert flat[0] == 0 and flat[-1] == 0


# ---- evc_rgb_to_yuv420 ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", SHAPES)
def test_rgb_to_yuv420_codes(L, G, H, W):
    """Seeded random and smooth clips, 8 and 10 bits, into a packed buffer and into a Y4M-style one whose markers and header
    must come through untouched.  Bar: module docstring, integer form; the range-event word stays 0."""
    for clip in ("random", "smooth"):
        x = torch.from_numpy(G[f"rgbk_{clip}_{H}x{W}"].astype(np.float32) / np.float32(255)).cuda()
        for bits in (8, 10):
            fb = H * W * (2 if bits > 8 else 1) * 3 // 2
            for lead, marker in ((b"", b""), (Y4M_LEAD, YR.FRAME_MARK)):
                events = torch.zeros(1, dtype=torch.int32, device="cuda")
                stride, first = len(marker) + fb, len(lead) + len(marker)
                canvas = bytearray(b"\xAA" * (len(lead) + 2 * stride + 3))
                canvas[:len(lead)] = lead
                for n in range(2):
                    at = len(lead) + n * stride
                    canvas[at:at + len(marker)] = marker
                buf = L.rgb_to_yuv420(x, events, bits, buf=upload(bytes(canvas)), first=first, stride=stride)
                got = buf.cpu().numpy().tobytes()
                assert int(events.item()) == 0
                k = n_all = 0
                planes = YR.split_buffer(got, 2, H, W, bits, first, stride)
                for name, p in zip("yuv", planes):
                    a, b = check_codes(p, G[f"code_{name}_{clip}_{H}x{W}_{bits}"], G[f"band_{name}_{clip}_{H}x{W}_{bits}"],
                                       f"{H}x{W} {clip} {bits}-bit {'y4m' if lead else 'raw'} {name}")
                    k, n_all = k + a, n_all + b
                assert k <= 0.01 * n_all
                # everything that is not a sample is as it was
                keep = bytearray(got)
                for n in range(2):
                    keep[first + n * stride:first + n * stride + fb] = b"\xAA" * fb
                blank = bytearray(canvas)
                for n in range(2):
                    blank[first + n * stride:first + n * stride + fb] = b"\xAA" * fb
                assert keep == blank


def test_frames_do_not_depend_on_the_launch_they_ride_in(L):
    """Frame n of an N-frame launch equals the one-frame launch bit for bit, both directions, vector and scalar shapes."""
    rng = np.random.default_rng(8)
    for H, W in ((18, 34), (32, 48)):
        N = 5
        x = torch.from_numpy(rng.random((N, 3, H, W), dtype=np.float32)).cuda()
        for bits in (8, 10):
            fb = H * W * (2 if bits > 8 else 1) * 3 // 2
            events = torch.zeros(1, dtype=torch.int32, device="cuda")
            all_ = L.rgb_to_yuv420(x, events, bits)
            for n in range(N):
                one = L.rgb_to_yuv420(x[n:n + 1], events, bits)
                assert torch.equal(one, all_[n * fb:(n + 1) * fb]), (H, W, bits, n)
            for mode in MODES:
                for dtype in (torch.float32, torch.uint8):
                    rgb = L.yuv420_to_rgb(all_, N, H, W, bits, mode, dtype=dtype)
                    for n in range(N):
                        one = L.yuv420_to_rgb(all_, 1, H, W, bits, mode, first=n * fb, dtype=dtype)
                        assert torch.equal(one[0], rgb[n]), (H, W, bits, mode, n)
            assert int(events.item()) == 0


def test_non_finite_pixels_write_zero_and_raise_the_word(L):
    H, W = 12, 16
    x0 = torch.from_numpy(YR.smooth_clip(2, H, W, seed=4)).cuda() * 0.5 + 0.25        # no sample is 0
    events = torch.zeros(1, dtype=torch.int32, device="cuda")
    clean = L.rgb_to_yuv420(x0, events, 8)
    assert int(events.item()) == 0 and int(clean.min()) > 0
    cy, cu, cv = YR.split_buffer(clean.cpu().numpy().tobytes(), 2, H, W)
    for value in (float("nan"), float("inf"), float("-inf")):
        for c in range(3):
            x = x0.clone()
            x[1, c, 5, 7] = value
            events.zero_()
            y, u, v = YR.split_buffer(L.rgb_to_yuv420(x, events, 8).cpu().numpy().tobytes(), 2, H, W)
            assert int(events.item()) == L.RANGE_NONFINITE, (value, c)
            assert y[1, 5, 7] == 0 and u[1, 2, 3] == 0 and v[1, 2, 3] == 0
            y[1, 5, 7], u[1, 2, 3], v[1, 2, 3] = cy[1, 5, 7], cu[1, 2, 3], cv[1, 2, 3]
            assert np.array_equal(y, cy) and np.array_equal(u, cu) and np.array_equal(v, cv)      # nothing else moved
    # the Python layer writes no file for such frames
    import evc_amd  # noqa: F401
    from evc_amd import video_io as V
    from evc_amd.recovery import NumericsError
    x = x0.clone()
    x[0, 1, 0, 0] = float("nan")
    target = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"evc_yuv_nonfinite_{os.getpid()}.y4m")
    with pytest.raises(NumericsError):
        V.write_clip(target, x, 30)
    assert not os.path.exists(target)


def test_round_trip_of_a_smooth_128x128_clip(L):
    """RGB -> 8-bit 4:2:0 -> RGB (bicubic) on a 30-frame 128x128 clip, against the float64 restatement at the same bars: the
    codes by the integer bar, the float RGB of the kernel's own codes by the float bar (no storage grid here: the full
    2e-6), the uint8 RGB by the integer bar."""
    T, H, W = 30, 128, 128
    x = YR.smooth_clip(T, H, W, seed=12)
    events = torch.zeros(1, dtype=torch.int32, device="cuda")
    buf = L.rgb_to_yuv420(torch.from_numpy(x).cuda(), events, 8)
    assert int(events.item()) == 0
    planes = YR.split_buffer(buf.cpu().numpy().tobytes(), T, H, W)
    codes, pre = YR.rgb_to_yuv420(x, 8)
    k = n = 0
    for name, p, c, q in zip("yuv", planes, codes, pre):
        a, b = check_codes(p, c, YR.tie_band(q, 255e-6), f"round trip {name}")
        k, n = k + a, n + b
    assert k <= 0.01 * n
    ref = YR.yuv420_to_rgb(*planes, 8, "bicubic")
    out = L.yuv420_to_rgb(buf, T, H, W, 8, "bicubic")
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
    print(f"round trip: max |rgb - float64 restatement| = {err:.3e}; against the input: {float(np.abs(ref - x).max()):.4f}")
    assert err <= FLOAT_BAR
    want, pre8 = YR.rgb_u8(ref)
    band = YR.tie_band(pre8, 255e-6)
    a, b = check_codes(L.yuv420_to_rgb(buf, T, H, W, 8, "bicubic", dtype=torch.uint8).cpu().numpy(), want, band, "round trip uint8")
    assert a <= 0.01 * b
    assert float(np.abs(ref - x).max()) < 0.05          # a smooth clip survives 4:2:0


def test_video_io_through_the_gpu(L, tmp_path):
    """write_clip -> file -> read_clips, Y4M and raw, 8 and 10 bits: the file's planes are the kernel's codes, the clips are
    the uint8 form of the conversion, a trailing partial clip is dropped."""
    import evc_amd  # noqa: F401
    from evc_amd import video_io as V
    x = YR.smooth_clip(7, 18, 34, seed=2)
    for bits in (8, 10):
        for name in ("a.y4m", f"a_34x18_25Hz_{bits}bit_.yuv"):
            path = str(tmp_path / f"{bits}_{name}")
            V.write_clip(path, x, 25, bits)
            f = V.open_video(path)
            assert (f.width, f.height, f.bits, f.fps, f.n_frames) == (34, 18, bits, 25, 7)
            events = torch.zeros(1, dtype=torch.int32, device="cuda")
            want = YR.split_buffer(L.rgb_to_yuv420(torch.from_numpy(x).cuda(), events, bits).cpu().numpy().tobytes(), 7, 18, 34, bits)
            for n in range(7):
                for p, w in zip(f.planes(n), want):
                    assert np.array_equal(p, w[n])
            said = []
            clips = V.read_clips(path, frames=3, log=said.append)
            assert clips.shape == (2, 3, 3, 18, 34) and clips.dtype == np.uint8 and len(said) == 1
            blob, first, stride = YR.frame_buffer(*want, bits)
            ref = L.yuv420_to_rgb(upload(blob), 6, 18, 34, bits, "bicubic", dtype=torch.uint8).cpu().numpy()
            assert np.array_equal(clips.reshape(6, 3, 18, 34), ref)
    a, b = V.yuv_round_trip_u8(x), V.yuv_round_trip_u8(x * 0.9)
    ps = V.psnr_u8(a, b)
    assert ps.shape == (7,) and np.isfinite(ps).all() and (V.psnr_u8(a, a) == np.inf).all()


# ---- the command lines ------------------------------------------------------------------------------------------------

def test_sender_reads_y4m_and_receiver_writes_the_same_y4m(L, tmp_path):
    """city_sender.py --data_yuv clip.y4m ... --yuv-out --yuv-metrics, then city_receiver.py --yuv, in fresh processes, with the
    reduced random-weight generator and step count of tests/test_gpu_job_stream.py: every job prints `frames: match`, the
    receiver's .y4m files equal the sender's byte for byte, and every .npy the sender writes equals that of the same run fed
    the equivalent --data_npy (read_clips of the same file)."""
    import evc_amd  # noqa: F401
    from evc_amd import synthetic, video_io as V
    clip = synthetic.make_clips(1, seed=11)[0].astype(np.float32) / 255
    y4m = tmp_path / "clip.y4m"
    V.write_clip(str(y4m), np.concatenate([clip, clip[:4]]), 30)           # 34 frames: one clip and a dropped tail
    np.save(tmp_path / "clip.npy", V.read_clips(str(y4m), log=lambda m: None))
    model = ["--config", os.path.join(REPO, "configs", "mine.yml"), "--synthetic", "--exp", str(tmp_path / "exp"),
             "--config_mod", "model.ngf=32 model.n_head_channels=32"]
    thresholds = [200.0, -100.0]            # all key frames; everything accepted
    common = ["--start_idx", "0", "--end_idx", "0", "--subsample", "2", "--q", "3", "--policy", "psnr", "--thresholds"] + \
        [str(t) for t in thresholds] + ["--bpp-limit", "1e9", "--batch-invariant"]
    send = [sys.executable, os.path.join(REPO, "city_sender.py")] + model + common
    out, bits, rx = tmp_path / "out", tmp_path / "bits", tmp_path / "rx"
    s = subprocess.run(send + ["--data_yuv", str(y4m), "--output_path", str(out), "--bitstream-dir", str(bits), "--yuv-out",
                               "--yuv-metrics"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert s.returncode == 0, s.stdout + s.stderr
    assert "the last 4 frame(s) are dropped" in s.stdout
    r = subprocess.run([sys.executable, os.path.join(REPO, "city_receiver.py")] + model +
                       ["--bitstream-dir", str(bits), "--output_path", str(rx), "--yuv", "--data_yuv", str(y4m)], cwd=tmp_path,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("frames: match") == len(thresholds) and "MISMATCH" not in r.stdout and "PSNR" in r.stdout, r.stdout
    for t in thresholds:
        sent = (out / "output_0" / ("city_idx0_q3_thr%.2f.y4m" % t)).read_bytes()
        assert sent == (rx / ("decoded_v0_q3_thr%.2f.y4m" % t)).read_bytes()
        f = V.open_video(str(rx / ("decoded_v0_q3_thr%.2f.y4m" % t)))
        assert (f.width, f.height, f.bits, f.fps, f.n_frames) == (128, 128, 8, 30, 30)
    ps = np.load(out / "output_0" / "psnr_yuv_frames_0.npy")
    assert ps.shape == (2, 30) and not np.isnan(ps).any() and np.load(out / "output_0" / "psnr_yuv_0.npy").shape[0] == 2
    # the same run from the equivalent .npy: every .npy output is the same, and nothing but the new files is added
    out2 = tmp_path / "out2"
    s2 = subprocess.run(send + ["--data_npy", str(tmp_path / "clip.npy"), "--output_path", str(out2), "--bitstream-dir",
                                str(tmp_path / "bits2")], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert s2.returncode == 0, s2.stdout + s2.stderr
    names2 = sorted(os.listdir(out2 / "output_0"))
    extra = sorted(set(os.listdir(out / "output_0")) - set(names2))
    assert extra == sorted(["psnr_yuv_0.npy", "psnr_yuv_frames_0.npy"] + ["city_idx0_q3_thr%.2f.y4m" % t for t in thresholds])
    for n in names2:
        assert (out / "output_0" / n).read_bytes() == (out2 / "output_0" / n).read_bytes(), n
    for n in sorted(os.listdir(bits)):
        assert (bits / n).read_bytes() == (tmp_path / "bits2" / n).read_bytes(), n
