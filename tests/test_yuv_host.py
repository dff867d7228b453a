"""Host tests of the video file boundary (no GPU): the numpy restatement tests/yuv_ref.py against the fixture the reference's
own transforms produced (tests/golden/yuv_transform.npz), Y4M / raw parsing, round trips and refusals of video_io.py, the two
exports of csrc/yuv.hip (declared, bound, built, argument checks before any launch), and the new command-line flags."""
import os
from fractions import Fraction

import numpy as np
import pytest

import yuv_ref as YR
from conftest import golden

import evc_amd  # noqa: F401
from evc_amd import video_io as V

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 2), (12, 16), (18, 34), (32, 48)]
GRID, OFFSET = 2.0 ** -22, 1.5          # how the fixture stores the float64 results (tests/golden/make_yuv_golden.py)


def golden_rgb(G, mode, H, W, bits):
    b = G[f"rgb_{mode}_{H}x{W}_{bits}"].astype(np.int64)
    return (b[0] + 256 * b[1] + 65536 * b[2]) * GRID - OFFSET


@pytest.fixture(scope="module")
def G():
    return golden("yuv_transform")


# ---- the restatement against the fixture ----------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", SHAPES)
def test_restatement_of_yuv420_to_rgb_equals_the_fixture(G, H, W):
    """Both are float64; the fixture's storage grid rounds by at most GRID / 2."""
    for bits in (8, 10):
        y, u, v = (G[f"yuv_{p}_{H}x{W}_{bits}"] for p in "yuv")
        assert y.shape == (2, H, W) and u.shape == v.shape == (2, H // 2, W // 2) and int(y.max()) <= 2 ** bits - 1
        for mode in ("nearest", "bilinear", "bicubic"):
            err = np.abs(YR.yuv420_to_rgb(y, u, v, bits, mode) - golden_rgb(G, mode, H, W, bits)).max()
            assert err <= GRID / 2 + 1e-12, (bits, mode, err)


@pytest.mark.parametrize("H,W", SHAPES)
def test_restatement_of_rgb_to_yuv420_equals_the_fixture(G, H, W):
    for clip in ("random", "smooth"):
        x = G[f"rgbk_{clip}_{H}x{W}"].astype(np.float32) / np.float32(255)
        for bits in (8, 10):
            codes, pre = YR.rgb_to_yuv420(x, bits)
            n_band = n = 0
            for name, c, p in zip("yuv", codes, pre):
                want, band = G[f"code_{name}_{clip}_{H}x{W}_{bits}"].astype(np.int64), G[f"band_{name}_{clip}_{H}x{W}_{bits}"]
                assert c.shape == want.shape
                assert np.array_equal(c[~band], want[~band]) and np.abs(c - want).max() <= 1
                assert np.array_equal(YR.tie_band(p, (2 ** bits - 1) * 1e-6), band)
                n_band, n = n_band + int(band.sum()), n + band.size
            assert n_band <= 0.01 * n


def test_bicubic_taps_are_the_issue_s_numbers():
    assert YR.TAPS["bicubic"] == (-0.03515625, 0.26171875, 0.87890625, -0.10546875)


def test_upsampling_matches_torch_interpolate_in_float64():
    """The restatement is written from the definition; torch's own F.interpolate is a second witness on a shape the fixture
    does not hold."""
    import torch
    p = np.random.default_rng(3).integers(0, 1024, (2, 1, 7, 5)).astype(np.float64)
    for mode in ("nearest", "bilinear", "bicubic"):
        kw = {} if mode == "nearest" else {"align_corners": False}
        ref = torch.nn.functional.interpolate(torch.from_numpy(p), scale_factor=2, mode=mode, **kw).numpy()
        assert np.abs(YR.upsample2(p, mode) - ref).max() < 1e-9, mode


# ---- files ------------------------------------------------------------------------------------------------------------

def planes_of(G, H, W, bits):
    return tuple(G[f"yuv_{p}_{H}x{W}_{bits}"] for p in "yuv")


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("ext", ["y4m", "yuv"])
def test_round_trip_bytes_planes_bytes(G, tmp_path, bits, ext):
    H, W = 18, 34
    y, u, v = planes_of(G, H, W, bits)
    lead = V.y4m_header(W, H, 25, bits) if ext == "y4m" else b""
    blob, first, stride = YR.frame_buffer(y, u, v, bits, lead=lead, marker=V.FRAME_MARK if ext == "y4m" else b"")
    src = tmp_path / f"clip_{W}x{H}_25Hz_{bits}bit_yuv420.{ext}"
    src.write_bytes(blob)
    f = V.open_video(str(src))
    assert (f.width, f.height, f.bits, f.fps, f.n_frames) == (W, H, bits, Fraction(25), 2)
    assert (f.first, f.stride) == (first, stride)
    for n in range(2):
        py, pu, pv = f.planes(n)
        assert py.dtype == (np.uint8 if bits == 8 else np.dtype("<u2"))
        assert np.array_equal(py, y[n]) and np.array_equal(pu, u[n]) and np.array_equal(pv, v[n])
    dst = tmp_path / f"copy_{W}x{H}_25Hz_{bits}bit_.{ext}"
    assert V.write_frames(str(dst), [f.planes(n) for n in range(2)], W, H, 25, bits) == 2
    assert dst.read_bytes() == blob
    piece, c_first, c_stride = f.chunk(1, 1)
    assert bytes(piece) == blob[first + stride:first + stride + f.frame_bytes] and (c_first, c_stride) == (0, stride)


def test_y4m_header_written_and_parsed():
    assert V.y4m_header(128, 128, 30) == b"YUV4MPEG2 W128 H128 F30:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n"
    assert V.y4m_header(34, 18, "30000/1001", 10) == b"YUV4MPEG2 W34 H18 F30000:1001 Ip A1:1 C420p10 XCOLORRANGE=FULL\n"
    g = V.parse_y4m_header(V.y4m_header(34, 18, "30000/1001", 10))
    assert g == dict(width=34, height=18, fps=Fraction(30000, 1001), bits=10)
    for tag, bits in (("420", 8), ("420jpeg", 8), ("420mpeg2", 8), ("420paldv", 8), ("420p10", 10)):
        assert V.parse_y4m_header(f"YUV4MPEG2 W16 H12 F25:1 Ip C{tag}".encode())["bits"] == bits
    assert V.parse_y4m_header(b"YUV4MPEG2 W16 H12 F25:1")["bits"] == 8          # no C tag: 4:2:0


@pytest.mark.parametrize("header,message", [
    (b"YUV4MPEG2 W16 H12 F25:1 Ip C422", "C422 is not supported"),
    (b"YUV4MPEG2 W16 H12 F25:1 Ip C444", "C444 is not supported"),
    (b"YUV4MPEG2 W16 H12 F25:1 Ip C444p10", "C444p10 is not supported"),
    (b"YUV4MPEG2 W16 H12 F25:1 Ip C420p12", "C420p12 is not supported"),
    (b"YUV4MPEG2 W16 H12 F25:1 It C420jpeg", "interlaced"),
    (b"YUV4MPEG2 W16 H12 F25:1 Im C420jpeg", "interlaced"),
    (b"YUV4MPEG2 W15 H12 F25:1 Ip C420jpeg", "even width and height"),
    (b"YUV4MPEG2 H12 F25:1", "without W or H"),
    (b"RIFF W16 H12", "does not begin with YUV4MPEG2"),
])
def test_refused_y4m_variants_say_why(header, message):
    with pytest.raises(V.VideoFormatError, match=message):
        V.parse_y4m_header(header)


def test_geometry_from_flag_and_file_name():
    assert V.parse_geometry("128x128") == dict(width=128, height=128, fps=Fraction(30), bits=8)
    assert V.parse_geometry("34x18@25:10") == dict(width=34, height=18, fps=Fraction(25), bits=10)
    assert V.parse_geometry("1920x1080@30000/1001") == dict(width=1920, height=1080, fps=Fraction(30000, 1001), bits=8)
    assert V.parse_geometry("64x32:10")["bits"] == 10
    for bad in ("128", "128x", "x128", "128x128@", "128x128:12", "127x128", "0x0"):
        with pytest.raises(V.VideoFormatError):
            V.parse_geometry(bad)
    assert V.geometry_from_name("/data/city_128x128_30Hz_8bit_yuv420p8.yuv") == dict(width=128, height=128, fps=Fraction(30), bits=8)
    assert V.geometry_from_name("Beauty_1920x1080_120Hz_10bit_yuv.yuv")["bits"] == 10
    assert V.geometry_from_name("clip.yuv") is None


def test_raw_file_needs_a_geometry_and_a_whole_number_of_frames(tmp_path):
    fb = V.frame_bytes(16, 12)
    assert fb == 16 * 12 * 3 // 2 and V.frame_bytes(16, 12, 10) == 2 * fb
    p = tmp_path / "clip.yuv"
    p.write_bytes(bytes(3 * fb))
    with pytest.raises(V.VideoFormatError, match="carries no geometry"):
        V.open_video(str(p))
    assert V.open_video(str(p), "16x12").n_frames == 3
    p.write_bytes(bytes(3 * fb - 5))
    with pytest.raises(V.VideoFormatError, match="not a whole number"):
        V.open_video(str(p), "16x12")
    named = tmp_path / "clip_16x12_30Hz_8bit_.yuv"
    named.write_bytes(bytes(2 * fb + 1))
    with pytest.raises(V.VideoFormatError, match="truncated file or wrong geometry"):
        V.open_video(str(named))
    with pytest.raises(V.VideoFormatError, match="no such file"):
        V.open_video(str(tmp_path / "absent.y4m"))


def test_truncated_or_marker_less_y4m_is_an_error(tmp_path):
    fb = V.frame_bytes(16, 12)
    good = V.y4m_header(16, 12, 30) + (V.FRAME_MARK + bytes(fb)) * 2
    p = tmp_path / "a.y4m"
    p.write_bytes(good)
    assert V.open_video(str(p)).n_frames == 2
    p.write_bytes(good[:-7])
    with pytest.raises(V.VideoFormatError, match="not a whole number"):
        V.open_video(str(p))
    p.write_bytes(good.replace(V.FRAME_MARK, b"FRAMe\n"))
    with pytest.raises(V.VideoFormatError, match="no plain FRAME marker"):
        V.open_video(str(p))


def test_clip_slicing_drops_the_tail():
    assert V.clip_slices(60) == ([(0, 30), (30, 30)], 0)
    assert V.clip_slices(71) == ([(0, 30), (30, 30)], 11)
    assert V.clip_slices(29) == ([], 29)
    assert V.clip_slices(7, frames=3) == ([(0, 3), (3, 3)], 1)


def test_read_clips_reports_a_dropped_tail_before_touching_the_gpu(tmp_path, monkeypatch):
    """Slicing is host work: with the kernel call replaced by a recorder, a 7-frame file read 3 frames at a time gives two
    launches over the right pieces of the file and one printed line about the dropped frame."""
    import torch
    from evc_amd import lib
    H, W = 12, 16
    rng = np.random.default_rng(0)
    y, u, v = rng.integers(0, 256, (7, H, W)), rng.integers(0, 256, (7, H // 2, W // 2)), rng.integers(0, 256, (7, H // 2, W // 2))
    blob, first, stride = YR.frame_buffer(y, u, v, 8, lead=V.y4m_header(W, H, 30), marker=V.FRAME_MARK)
    p = tmp_path / "seven.y4m"
    p.write_bytes(blob)
    calls, said = [], []

    def recorder(buf, N, H_, W_, bits, mode, first=0, stride=None, offsets=None, dtype=None, out=None):
        calls.append((bytes(buf.numpy()), N, first, stride, mode, dtype))
        return torch.zeros((N, 3, H_, W_), dtype=torch.uint8)
    monkeypatch.setattr(lib, "yuv420_to_rgb", recorder)
    out = V.read_clips(str(p), frames=3, device="cpu", log=said.append)
    assert out.shape == (2, 3, 3, H, W) and out.dtype == np.uint8
    assert len(said) == 1 and "7 frames = 2 clip(s) of 3" in said[0] and "last 1 frame" in said[0]
    assert [(c[1], c[2], c[3], c[4], c[5]) for c in calls] == [(3, 0, stride, "bicubic", torch.uint8)] * 2
    for b, c in enumerate(calls):
        at = first + 3 * b * stride
        assert c[0] == blob[at:at + 2 * stride + V.frame_bytes(W, H)]
    with pytest.raises(V.VideoFormatError, match="fewer than one clip"):
        V.read_clips(str(p), frames=30, device="cpu", log=said.append)


# ---- the exports ----------------------------------------------------------------------------------------------------

def test_yuv_exports_are_declared_bound_and_built():
    """Declared in the header, bound in lib.py, compiled from csrc/yuv.hip, exported by the library; argument checks return
    EVC_EINVAL before any launch (this machine has no GPU: a launch would fail otherwise)."""
    from evc_amd import build, lib
    header = open(os.path.join(REPO, "include", "evc_hip.h")).read()
    for name in ("evc_yuv420_to_rgb", "evc_rgb_to_yuv420"):
        assert name in header and name in lib.HIP_SYMBOLS
    assert "yuv.hip" in build.HIP_SOURCES
    so = lib.hip_lib(require_device=False)
    fb = 12 * 16 * 3 // 2
    offs = (0, 192, 240)
    ok = dict(bytes=2 * fb, first=0, stride=fb, N=2, H=12, W=16, bits=8, mode=2)

    def y2r(src=1, out=1, **kw):
        a = dict(ok, **kw)
        return so.evc_yuv420_to_rgb(src, a["bytes"], a["first"], a["stride"], *a.get("offs", offs), a["N"], a["H"], a["W"], a["bits"],
                                    a["mode"], out, 0, None)

    def r2y(rgb=1, dst=1, events=1, **kw):
        a = dict(ok, **kw)
        return so.evc_rgb_to_yuv420(rgb, dst, a["bytes"], a["first"], a["stride"], *a.get("offs", offs), a["N"], a["H"], a["W"],
                                    a["bits"], events, None)
    bad = [dict(H=13), dict(W=15), dict(H=0), dict(W=0), dict(N=0), dict(N=70000), dict(bits=12), dict(bits=9), dict(first=-1),
           dict(stride=-1), dict(bytes=2 * fb - 1), dict(first=1), dict(stride=fb + 1), dict(offs=(0, 192, 241)), dict(offs=(-1, 192, 240)),
           dict(bits=10), dict(bytes=0)]
    for kw in bad:
        assert y2r(**kw) == -1, kw
        assert r2y(**kw) == -1, kw
    assert y2r(mode=3) == -1 and y2r(mode=-1) == -1
    assert y2r(src=None) == -1 and y2r(out=None) == -1
    assert r2y(rgb=None) == -1 and r2y(dst=None) == -1 and r2y(events=None) == -1


# ---- the command lines ------------------------------------------------------------------------------------------------

def test_sender_flags():
    from evc_amd import cli
    a = cli.parse_args(["--data_yuv", "clip.y4m", "--yuv-out", "--yuv-metrics"])
    assert a.data_yuv == "clip.y4m" and a.yuv_out and a.yuv_metrics and a.yuv_upsample == "bicubic" and a.yuv_geometry is None
    a = cli.parse_args(["--data_yuv", "clip.yuv", "--yuv-geometry", "128x128@30:8", "--yuv-upsample", "nearest"])
    assert a.yuv_geometry == "128x128@30:8" and a.yuv_upsample == "nearest"
    a = cli.parse_args(["--data_npy", "x.npy"])              # nothing changes for the existing flags
    assert a.data_npy == "x.npy" and a.data_yuv is None and not a.yuv_out and not a.yuv_metrics
    assert cli.parse_args([]).data_npy == "city_bonn.npy"


@pytest.mark.parametrize("argv", [["--data_yuv", "clip.y4m", "--data_npy", "x.npy"], ["--data_npy=x.npy", "--data_yuv", "clip.y4m"],
                                  ["--yuv-geometry", "128x128"], ["--data_yuv", "c.yuv", "--yuv-upsample", "lanczos"]])
def test_sender_refuses_contradicting_inputs(argv, capsys):
    from evc_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.parse_args(argv)
    assert e.value.code == 2
    if "--data_npy" in " ".join(argv):
        assert "--data_yuv replaces --data_npy" in capsys.readouterr().err


def test_receiver_flags(capsys):
    from evc_amd import cli, receiver
    p = receiver.build_parser()
    a = cli.parse_args(["--bitstream-dir", "d", "--yuv", "--fps", "25", "--data_yuv", "clip.y4m"], p)
    assert a.yuv and a.fps == "25" and a.data_yuv == "clip.y4m"
    a = cli.parse_args(["--bitstream-dir", "d"], p)
    assert not a.yuv and a.fps == "30" and a.data_yuv is None and a.data_npy == "city_bonn.npy"
    with pytest.raises(SystemExit):
        cli.parse_args(["--bitstream-dir", "d", "--data_yuv", "clip.y4m", "--data_npy", "x.npy"], p)
    assert "--data_yuv replaces --data_npy" in capsys.readouterr().err


def test_a_file_of_another_size_is_refused_with_the_resizing_note(tmp_path):
    from evc_amd import cli
    p = tmp_path / "small.y4m"
    p.write_bytes(V.y4m_header(16, 12, 30) + V.FRAME_MARK + bytes(V.frame_bytes(16, 12)))
    a = cli.parse_args(["--data_yuv", str(p)])
    with pytest.raises(SystemExit, match="resizing is not built"):
        cli.load_yuv_clips(a, 128)
    a = cli.parse_args(["--data_yuv", str(tmp_path / "absent.y4m")])
    with pytest.raises(SystemExit, match="no such file"):
        cli.load_yuv_clips(a, 128)
