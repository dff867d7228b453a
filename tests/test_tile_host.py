"""Host tests of the whole-frame tiling (DESIGN.md section 8c "Whole frames"): the grid of video_io.tile_axis / tile_grid, the
identities of the numpy restatement tests/tile_ref.py, the manifest, the parser's checks and the device-free logic of
stitch.py.  Nothing here needs a GPU."""
import json
import os

import numpy as np
import pytest

import tile_ref as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def V():
    import evc_amd  # noqa: F401
    from evc_amd import video_io
    return video_io


@pytest.mark.parametrize("S,O", [(32, 0), (32, 4), (32, 16), (128, 16)])
def test_grid_properties_for_every_length(V, S, O):
    for L in range(1, 4 * S + 4):
        o = V.tile_axis(L, S, O)
        assert o == T.axis(L, S, O)
        assert o[0] == 0 and o[-1] == max(L - S, 0), (L, o)
        if L <= S:
            assert o == [0]
            continue
        assert len(o) == -(-(L - O) // (S - O)) >= 2
        steps = np.diff(o)
        assert steps.min() >= 1 and steps.max() <= S - O, (L, o)          # so neighbours overlap by at least O
        assert all(0 <= v and v + S <= L for v in o), (L, o)               # every tile inside the frame: no padding
        cover = T.cover_counts(L, S, o)
        assert cover.min() >= 1 and cover.max() <= 3, (L, o)


def test_worked_examples(V):
    assert V.tile_grid(288, 352, 128, 16) == ([0, 80, 160], [0, 112, 224])
    assert V.tile_grid(144, 160, 128, 16) == ([0, 16], [0, 32])
    assert V.tile_grid(1080, 1920, 128, 16) == (T.axis(1080, 128, 16), T.axis(1920, 128, 16))
    assert (len(T.axis(1080, 128, 16)), len(T.axis(1920, 128, 16))) == (10, 17)


def test_a_pixel_may_lie_in_three_tiles(V):
    o = V.tile_axis(61, 32, 4)
    assert o == [0, 14, 29]
    assert [k for k, v in enumerate(o) if v <= 30 < v + 32] == [0, 1, 2]
    assert T.cover_counts(61, 32, o)[30] == 3


@pytest.mark.parametrize("bad", [(0, 32, 4), (40, 0, 0), (40, 32, -2), (40, 32, 17)])
def test_tile_axis_refuses(V, bad):
    with pytest.raises(ValueError):
        V.tile_axis(*bad)


@pytest.mark.parametrize("H,W,O,S", T.GEOMETRIES)
def test_blending_gathered_tiles_gives_the_image_back(H, W, O, S):
    """Every tile holds the image's own values, so the blend is a weighted mean of equal numbers: sum(w v) carries one rounding
    per product and per addition (at most 9 tiles: 17 roundings of relative 2^-24 on terms of one sign) and the division one
    more, well inside 2.4e-7 absolute on values in [0, 1] -- and far inside the 1 / 510 that rounding to a byte allows."""
    x = np.random.default_rng(3).integers(0, 256, (2, 3, H, W), dtype=np.uint8)
    oy, ox = T.grid(H, W, S, O)
    out = T.blend(T.gather(x, S, oy, ox).astype(np.float32) / np.float32(255), H, W, oy, ox)
    want = x.astype(np.float32) / np.float32(255)
    assert out.dtype == np.float32 and out.shape == x.shape
    assert np.abs(out.astype(np.float64) - want).max() <= 2.4e-7
    assert np.array_equal(np.rint(out * np.float32(255)).astype(np.uint8), x)


@pytest.mark.parametrize("H,W,O,S", T.GEOMETRIES)
def test_constant_tiles_blend_to_the_constant(H, W, O, S):
    """Constant tiles blend to the constant within 1 ulp -- for the constants for which that follows from the definition: the
    8-bit levels k / 256.  A weight is at most (S / 2)^2 <= 2^12 and at most 9 tiles cover a pixel, so every product w c and
    every partial sum is an integer below 9 * 2^12 * 2^8 < 2^24 in units of 1 / 256: nothing rounds, acc = den c exactly, and
    the correctly rounded division returns c itself.  It is NOT a property of the definition for a constant with a full
    mantissa: each product and each addition rounds, and the restatement gives -1.7000002 for float32(-1.7) on the
    (40, 70, 8) grid, 2 ulp (2.38e-7) away.  Such constants are therefore not asserted here."""
    oy, ox = T.grid(H, W, S, O)
    for c in (0.0, 1.0, 0.5, -1.75, 200 / 256, 255 / 256, 2.0, -1.0):
        c = np.float32(c)
        out = T.blend(np.full((len(oy) * len(ox), 1, 3, S, S), c, dtype=np.float32), H, W, oy, ox)
        assert np.abs(out - c).max() <= np.spacing(max(np.abs(c), np.float32(2.0 ** -126))), (float(c), float(np.abs(out - c).max()))


def test_gather_replicates_the_edge_of_a_short_axis():
    x = np.random.default_rng(4).integers(0, 256, (1, 3, 20, 50), dtype=np.uint8)
    oy, ox = T.grid(20, 50, 32, 0)
    assert (oy, ox) == ([0], [0, 18])
    t = T.gather(x, 32, oy, ox)
    assert t.shape == (2, 1, 3, 32, 32)
    assert np.array_equal(t[0][:, :, :20], x[:, :, :, :32]) and np.array_equal(t[1][:, :, :20], x[:, :, :, 18:])
    assert all(np.array_equal(t[k][:, :, r], t[k][:, :, 19]) for k in (0, 1) for r in range(20, 32))


def test_manifest_round_trip(V, tmp_path):
    m = V.tile_manifest(352, 288, 128, 16, clips=2, frames=30, fps="30000/1001", source="/some/where/foreman_cif.y4m")
    assert m["version"] == 1 and (m["ny"], m["nx"]) == (3, 3) and m["oy"] == [0, 80, 160] and m["ox"] == [0, 112, 224]
    assert m["source"] == "foreman_cif.y4m" and m["clips"] == 2 and m["frames"] == 30 and m["fps"] == "30000/1001"
    assert set(m) == set(V.MANIFEST_KEYS)
    path = V.write_manifest(str(tmp_path / "out"), m)
    assert os.path.basename(path) == "tiles.json"
    with open(path) as fh:
        assert json.load(fh) == m                        # plain JSON
    assert V.read_manifest(path) == m
    assert V.as_fps(m["fps"]) == V.as_fps((30000, 1001))
    for change in (dict(version=2), dict(ox=[0, 100, 224]), dict(nx=2)):
        with open(path, "w") as fh:
            json.dump(dict(m, **change), fh)
        with pytest.raises(V.VideoFormatError):
            V.read_manifest(path)
    with open(path, "w") as fh:
        json.dump({k: v for k, v in m.items() if k != "overlap"}, fh)
    with pytest.raises(V.VideoFormatError, match="overlap"):
        V.read_manifest(path)


def test_parser_accepts_the_tile_flags():
    from evc_amd import cli, receiver
    cfg = ["--config", os.path.join(REPO, "configs", "mine.yml")]
    for parser, lead in ((None, []), (receiver.build_parser(), ["--bitstream-dir", "b"])):
        a = cli.parse_args(lead + cfg + ["--data_yuv", "c.y4m", "--yuv-fit", "tile"], parser)
        assert (a.yuv_fit, a.yuv_tile_overlap) == ("tile", 16)
        a = cli.parse_args(lead + cfg + ["--data_frames", "d/output_%04d.png", "--yuv-fit=tile", "--yuv-tile-overlap=64"], parser)
        assert (a.yuv_fit, a.yuv_tile_overlap) == ("tile", 64)
        a = cli.parse_args(lead + cfg + ["--data_yuv", "c.y4m", "--yuv-fit", "tile", "--yuv-tile-overlap", "0"], parser)
        assert a.yuv_tile_overlap == 0
    assert "yuv_tile_overlap" in cli.YUV_FLAGS and set(cli.YUV_FLAGS) <= set(cli.OPT_IN_FLAGS)     # args.yml without it is what it was


@pytest.mark.parametrize("argv,message", [
    (["--data_yuv", "c.y4m", "--yuv-tile-overlap", "8"], "--yuv-tile-overlap is the overlap of --yuv-fit tile"),
    (["--data_yuv", "c.y4m", "--yuv-fit", "crop", "--yuv-tile-overlap=8"], "--yuv-tile-overlap is the overlap of --yuv-fit tile"),
    (["--data_yuv", "c.y4m", "--yuv-fit", "tile", "--yuv-tile-overlap", "7"], "must be even"),
    (["--data_yuv", "c.y4m", "--yuv-fit", "tile", "--yuv-tile-overlap", "-2"], "must be even and inside"),
    (["--data_yuv", "c.y4m", "--yuv-fit", "tile", "--yuv-tile-overlap", "66"], "[0, 64]"),
    (["--data_yuv", "c.y4m", "--yuv-fit", "tile", "--yuv-resize", "box"], "--yuv-resize names the filter of --yuv-fit crop"),
    (["--yuv-fit", "tile"], "--yuv-fit fits the frames"),
])
def test_parser_refuses(argv, message, capsys):
    from evc_amd import cli, receiver
    cfg = ["--config", os.path.join(REPO, "configs", "mine.yml")]
    for parser, lead in ((None, []), (receiver.build_parser(), ["--bitstream-dir", "b"])):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(lead + cfg + argv, parser)
        assert e.value.code == 2
        assert message in capsys.readouterr().err


def test_overlap_is_checked_against_the_models_size(V):
    for size, overlap in ((128, 66), (32, 18), (128, 15), (128, -2)):
        with pytest.raises(ValueError, match="overlap"):
            V.check_overlap(size, overlap)
    V.check_overlap(128, 64), V.check_overlap(32, 0)
    with pytest.raises(ValueError, match="overlap"):
        V.read_clips("nothing.y4m", fit="tile", size=32, overlap=18)          # said before the file is opened


def test_stitch_names_and_groups():
    from evc_amd import container, stitch
    assert stitch.parse_decoded_name("decoded_v7_q3_thr200.00.npy") == (7, 3, "200.00")
    assert stitch.parse_decoded_name("/a/b/decoded_v12_q5_thr-100.00.npy") == (12, 5, "-100.00")
    assert stitch.parse_decoded_name("decoded_v1_q4_thr0.30.y4m") is None and stitch.parse_decoded_name("stitched_c0_q3_thr1.00.npy") is None
    # the receiver's own naming: decoded_<the job file's stem without "job_">
    for vid, q, thr in ((0, 3, 200.0), (11, 4, 0.3), (5, 5, -100.0)):
        stem = container.job_file_name(vid, q, thr)[len("job_"):-len(".evc")]
        assert stitch.parse_decoded_name(f"decoded_{stem}.npy") == (vid, q, "%.2f" % thr)
    names = [f"decoded_v{v}_q3_thr200.00.npy" for v in (0, 1, 2, 3, 4, 6, 7)] + ["decoded_v5_q4_thr200.00.npy", "notes.txt",
                                                                                   "decoded_v0_q3_thr200.00.y4m"]
    g = stitch.group_decoded(names, 4)
    assert sorted(g) == [(0, 3, "200.00"), (1, 3, "200.00"), (1, 4, "200.00")]
    assert g[(0, 3, "200.00")] == {t: f"decoded_v{t}_q3_thr200.00.npy" for t in range(4)}
    assert stitch.missing_videos(0, g[(0, 3, "200.00")], 4) == []
    assert stitch.missing_videos(1, g[(1, 3, "200.00")], 4) == [5]
    assert stitch.missing_videos(1, g[(1, 4, "200.00")], 4) == [4, 6, 7]
    line = stitch.missing_line(1, 4, "200.00", [4, 6, 7], 4)
    assert "stitched_c1_q4_thr200.00" in line and "3 of 4 tile(s) missing" in line and "4, 6, 7" in line
    assert stitch.stitched_name(0, 3, "200.00") == "stitched_c0_q3_thr200.00"
