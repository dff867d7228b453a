"""Host tests of the frame-fitting path: the numpy restatement tests/resize_ref.py against Pillow's own
outputs (tests/golden/resize_pillow.npz, and live Pillow where it is installed), lib.resample_tables against the restatement,
the crop rule, the int32 guard, and the command-line flags.  Everything here is exact: Pillow's 8-bit resize is integer
arithmetic, so no test has a tolerance."""
import os
import random

import numpy as np
import pytest

import evc_amd  # noqa: F401
import resize_ref as R
from conftest import golden
from evc_amd import video_io as V

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL, CASES, KINDS, FIXTURES = R.ALL, R.CASES, R.KINDS, R.FIXTURES


@pytest.fixture(scope="module")
def G():
    return golden("resize_pillow")


def test_the_fixture_holds_every_case(G):
    assert str(G["pillow_version"])
    for case, (n, H, W, oh, ow, filters) in CASES.items():
        assert tuple(G[f"size_{case}"]) == (oh, ow)
        for kind in KINDS:
            x = G[f"in_{case}_{kind}"]
            assert x.shape == (n, 3, H, W) and x.dtype == np.uint8
            if kind == "binary":
                assert set(np.unique(x)) == {0, 255}
            for f in filters:
                assert G[f"out_{case}_{kind}_{f}"].shape == (n, 3, oh, ow)
    outs = np.concatenate([G[f"out_{c}_binary_{f}"].ravel() for c, k, f in FIXTURES if k == "binary"])
    assert (outs == 0).mean() > 0.1 and (outs == 255).mean() > 0.1          # both clip ends occur


@pytest.mark.parametrize("case,kind,filter", FIXTURES)
def test_the_restatement_equals_pillows_output(G, case, kind, filter):
    oh, ow = CASES[case][3:5]
    assert np.array_equal(R.fit_box(G[f"in_{case}_{kind}"], oh, ow, filter), G[f"out_{case}_{kind}_{filter}"])


def test_the_restatement_equals_live_pillow():
    """About 40 seeded geometries, up- and down-scaling, every filter, both image kinds."""
    Image = pytest.importorskip("PIL.Image")
    filters = {"lanczos": Image.LANCZOS, "bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR, "hamming": Image.HAMMING, "box": Image.BOX}
    rnd = random.Random(5)
    rng = np.random.default_rng(5)
    for i in range(40):
        H, W, oh, ow = (rnd.randint(1, 90) for _ in range(4))
        name = ALL[i % 5]
        x = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        if i % 2:
            x = np.where(x < 128, 0, 255).astype(np.uint8)
        want = np.array(Image.fromarray(x).resize((ow, oh), filters[name]))
        got = R.resize(np.ascontiguousarray(x.transpose(2, 0, 1)), oh, ow, name).transpose(1, 2, 0)
        assert np.array_equal(got, want), (H, W, oh, ow, name)


@pytest.mark.parametrize("n_in,n_out", [(32, 16), (24, 32), (136, 128), (270, 16), (1080, 128), (40, 12), (7, 7), (1, 5), (5, 1), (13000, 16)])
def test_resample_tables_equal_the_restatement(n_in, n_out):
    from evc_amd import lib
    for name in ALL:
        b, k, ksize = lib.resample_tables(n_in, n_out, name)
        rb, rk, rksize = R.tables(n_in, n_out, name)
        assert ksize == rksize and b.dtype == np.int32 and k.dtype == np.int32 and k.shape == (n_out, ksize)
        assert np.array_equal(b, rb) and np.array_equal(k, rk)
        assert (b[:, 0] >= 0).all() and (b[:, 1] <= ksize).all() and (b.sum(1) <= n_in).all()


def test_the_int32_guard_refuses_a_filter_that_could_wrap():
    """Lanczos stays near 1.3 * 2^30.  A made-up filter whose taps alternate +-1 around a small positive sum normalises to
    taps of size 1 / sum each: the absolute sum times 255 leaves int32 and the table is refused."""
    from evc_amd import lib
    _, k, _ = lib.resample_tables(1080, 128, "lanczos")
    assert 255 * int(np.abs(k.astype(np.int64)).sum(1).max()) + 2 ** 21 < 2 ** 31

    def wild(x):
        return (1.05 if int(np.floor(x * 4)) % 2 else -1.0) if -2.0 <= x < 2.0 else 0.0
    with pytest.raises(ValueError, match="int32"):
        lib.resample_tables(64, 8, (wild, 2.0))


@pytest.mark.parametrize("H,W,box", [(128, 128, (0, 0, 128, 128)), (1080, 1920, (0, 420, 1080, 1080)), (1920, 1080, (420, 0, 1080, 1080)),
                                     (33, 47, (0, 7, 32, 32)), (47, 33, (7, 0, 32, 32)), (288, 352, (0, 32, 288, 288)),
                                     (144, 160, (0, 8, 144, 144)), (2, 2, (0, 0, 2, 2)), (3, 8, (0, 3, 2, 2))])
def test_center_box(H, W, box):
    assert V.center_box(H, W) == box == R.center_box(H, W)
    # the reference's slices
    m = min(H, W)
    img = np.arange(H * W).reshape(H, W)
    want = img[H // 2 - m // 2:H // 2 + m // 2, W // 2 - m // 2:W // 2 + m // 2]
    assert np.array_equal(R.crop(img, box), want)


def test_exports_are_declared_bound_and_built():
    from evc_amd import build, lib
    header = open(os.path.join(REPO, "include", "evc_hip.h")).read()
    for name in ("evc_resample_h_u8", "evc_resample_v_u8"):
        assert name in header and name in lib.HIP_SYMBOLS
    assert build.HIP_SOURCES.index("resample.hip") < build.HIP_SOURCES.index("api.hip")
    so = lib.hip_lib(require_device=False)
    ok = dict(src=1, planes=3, rows=8, cols=8, plane_stride=64, row_stride=8, bounds=1, coeffs=1, ksize=7, n_out=4, dst=1)
    bad = [dict(src=None), dict(dst=None), dict(bounds=None), dict(coeffs=None), dict(planes=0), dict(rows=0), dict(cols=0), dict(ksize=0),
           dict(n_out=0), dict(row_stride=7), dict(plane_stride=63), dict(plane_stride=-1), dict(rows=-3), dict(cols=(1 << 24) + 1, row_stride=1 << 25)]
    for fn in (so.evc_resample_h_u8, so.evc_resample_v_u8):
        for kw in bad:
            a = dict(ok, **kw)
            assert fn(a["src"], a["planes"], a["rows"], a["cols"], a["plane_stride"], a["row_stride"], a["bounds"], a["coeffs"], a["ksize"],
                      a["n_out"], a["dst"], None) < 0, kw


# ---- the command lines ------------------------------------------------------------------------------------------------

def test_flags_and_their_defaults():
    from evc_amd import cli, receiver
    for parser, lead in ((None, []), (receiver.build_parser(), ["--bitstream-dir", "d"])):
        a = cli.parse_args(lead, parser)
        assert a.yuv_fit == "refuse" and a.yuv_resize == "lanczos" and a.data_frames is None
        a = cli.parse_args(lead + ["--data_yuv", "c.y4m", "--yuv-fit", "crop"], parser)
        assert a.yuv_fit == "crop" and a.yuv_resize == "lanczos"
        a = cli.parse_args(lead + ["--data_yuv", "c.y4m", "--yuv-fit", "crop", "--yuv-resize", "box"], parser)
        assert a.yuv_resize == "box"
        a = cli.parse_args(lead + ["--data_frames", "d/output_%04d.png", "--yuv-fit=crop", "--yuv-resize=hamming"], parser)
        assert a.data_frames == "d/output_%04d.png" and a.yuv_fit == "crop" and a.yuv_resize == "hamming" and a.data_yuv is None
    assert {"yuv_fit", "yuv_resize", "data_frames"} <= set(cli.YUV_FLAGS) <= set(cli.OPT_IN_FLAGS)     # args.yml without them is what it was


@pytest.mark.parametrize("argv,said", [
    (["--data_yuv", "c.y4m", "--yuv-resize", "box"], "--yuv-resize names the filter of --yuv-fit crop"),
    (["--data_yuv", "c.y4m", "--yuv-resize=lanczos"], "--yuv-resize names the filter of --yuv-fit crop"),
    (["--data_yuv", "c.y4m", "--yuv-fit", "refuse", "--yuv-resize", "box"], "--yuv-resize names the filter"),
    (["--yuv-fit", "crop"], "--yuv-fit fits the frames"),
    (["--data_yuv", "c.y4m", "--yuv-fit", "stretch"], "invalid choice"),
    (["--data_yuv", "c.y4m", "--yuv-fit", "crop", "--yuv-resize", "nearest"], "invalid choice"),
    (["--data_frames", "d/%04d.png", "--data_yuv", "c.y4m"], "--data_frames replaces"),
    (["--data_frames", "d/%04d.png", "--data_npy", "x.npy"], "--data_frames replaces"),
    (["--data_npy=x.npy", "--data_frames", "d/%04d.png"], "--data_frames replaces"),
])
def test_usage_errors(argv, said, capsys):
    from evc_amd import cli, receiver
    for parser, lead in ((None, []), (receiver.build_parser(), ["--bitstream-dir", "d"])):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(lead + argv, parser)
        assert e.value.code == 2 and said in capsys.readouterr().err


def test_the_refusal_names_the_flag(tmp_path):
    from evc_amd import cli
    p = tmp_path / "small.y4m"
    p.write_bytes(V.y4m_header(16, 12, 30) + V.FRAME_MARK + bytes(V.frame_bytes(16, 12)))
    for argv in (["--data_yuv", str(p)], ["--data_yuv", str(p), "--yuv-fit", "refuse"]):
        with pytest.raises(SystemExit) as e:
            cli.load_yuv_clips(cli.parse_args(argv), 128)
        assert "resizing is not built" in str(e.value) and "--yuv-fit crop" in str(e.value)


def write_pngs(tmp_path, n, size=(8, 6), mode="RGB"):
    Image = pytest.importorskip("PIL.Image")
    d = tmp_path / mode
    d.mkdir()
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (n, size[1], size[0], 3), dtype=np.uint8)
    for i, f in enumerate(frames):
        im = Image.fromarray(f)
        (im if mode == "RGB" else im.convert(mode)).save(d / ("output_%04d.png" % i))
    return str(d / "output_%04d.png"), frames


def test_data_frames_reads_rgb_files_until_one_is_missing(tmp_path):
    """Frames of the model's size never touch the GPU: 7 files = 2 clips of 3 and a dropped tail."""
    pattern, frames = write_pngs(tmp_path, 7)
    said = []
    clips = V.read_frame_clips(pattern, frames=3, log=said.append)
    assert clips.shape == (2, 3, 3, 6, 8) and clips.dtype == np.uint8
    assert np.array_equal(clips.reshape(6, 3, 6, 8), frames[:6].transpose(0, 3, 1, 2))
    assert len(said) == 1 and "the last 1 frame(s) are dropped" in said[0]
    with pytest.raises(V.VideoFormatError, match="fewer than one clip"):
        V.read_frame_clips(pattern, frames=30, log=said.append)
    with pytest.raises(V.VideoFormatError, match="no such file"):
        V.read_frame_clips(str(tmp_path / "absent_%04d.png"), log=said.append)
    with pytest.raises(V.VideoFormatError, match="not a frame pattern"):
        V.read_frame_clips(str(tmp_path / "no_field.png"), log=said.append)


def test_data_frames_refuses_a_palette_png(tmp_path):
    from evc_amd import cli
    pattern, _ = write_pngs(tmp_path, 30, mode="P")
    with pytest.raises(V.VideoFormatError, match=r"output_0000\.png: image mode P, only RGB is read"):
        V.read_frame_clips(pattern, frames=3, log=lambda m: None)
    with pytest.raises(SystemExit, match=r"--data_frames: .*output_0000\.png: image mode P"):
        cli.load_yuv_clips(cli.parse_args(["--data_frames", pattern]), 128)


def test_data_frames_of_another_size_are_refused_without_the_flag(tmp_path):
    from evc_amd import cli
    pattern, _ = write_pngs(tmp_path, 30)
    with pytest.raises(SystemExit, match="--yuv-fit crop"):
        cli.load_yuv_clips(cli.parse_args(["--data_frames", pattern]), 128, log=lambda m: None)
