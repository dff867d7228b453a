"""Host tests of joint generation (DESIGN.md section 8c "Joint generation"): canvas.json, what the two command lines refuse
before any GPU work, the frame-size check of ``ClipDecoder.decode_jobs`` and the plane view of ``lib.tile_blend_planes``.
Nothing here needs a GPU."""
import json
import os
import types

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = ["--config", os.path.join(REPO, "configs", "mine.yml")]


@pytest.fixture(scope="module")
def V():
    import evc_amd  # noqa: F401
    from evc_amd import video_io
    return video_io


def test_canvas_manifest_round_trip(V, tmp_path):
    m = V.tile_manifest(352, 288, 128, 16, 3, 30, (30000, 1001), "/some/where/foreman_cif.y4m")
    path = V.write_manifest(str(tmp_path / "bits"), m, V.CANVAS_NAME)
    assert os.path.basename(path) == "canvas.json" == V.CANVAS_NAME and os.listdir(tmp_path / "bits") == ["canvas.json"]
    with open(path) as fh:
        raw = json.load(fh)
    assert raw == m
    assert (raw["version"], raw["width"], raw["height"], raw["size"], raw["overlap"]) == (1, 352, 288, 128, 16)
    assert (raw["oy"], raw["ox"], raw["clips"], raw["frames"], raw["source"]) == ([0, 80, 160], [0, 112, 224], 3, 30, "foreman_cif.y4m")
    assert V.as_fps(raw["fps"]) == V.as_fps((30000, 1001))
    assert V.read_canvas(str(tmp_path / "bits")) == m
    assert V.canvas_line(352, 288, 128, 16, m["oy"], m["ox"]) == "352x288 frames, joint generation over 3 x 3 tiles of 128x128 (overlap 16)"
    # a missing file is named; a file whose origins are not the grid's is refused
    with pytest.raises(V.VideoFormatError, match="canvas.json"):
        V.read_canvas(str(tmp_path / "nothing"))
    with open(path, "w") as fh:
        json.dump(dict(m, oy=[0, 81, 160]), fh)
    with pytest.raises(V.VideoFormatError):
        V.read_canvas(str(tmp_path / "bits"))
    # the tile manifest's name is still the default
    assert os.path.basename(V.write_manifest(str(tmp_path / "t"), m)) == "tiles.json"


def test_parser_accepts_joint():
    from evc_amd import cli, receiver
    a = cli.parse_args(CFG + ["--data_yuv", "c.y4m", "--yuv-fit", "joint"])
    assert (a.yuv_fit, a.yuv_tile_overlap) == ("joint", 16)
    a = cli.parse_args(CFG + ["--data_frames", "d/output_%04d.png", "--yuv-fit=joint", "--yuv-tile-overlap=32"])
    assert (a.yuv_fit, a.yuv_tile_overlap) == ("joint", 32)
    # the receiver needs no source: canvas.json names the size
    a = cli.parse_args(["--bitstream-dir", "b"] + CFG + ["--yuv-fit", "joint"], receiver.build_parser(), receiver=True)
    assert a.yuv_fit == "joint" and a.data_yuv is None and a.data_frames is None
    a = cli.parse_args(["--bitstream-dir", "b"] + CFG + ["--yuv-fit", "joint", "--data_yuv", "c.y4m"], receiver.build_parser(), receiver=True)
    assert a.data_yuv == "c.y4m"


@pytest.mark.parametrize("argv,message", [
    (["--data_yuv", "c.y4m", "--yuv-tile-overlap", "8"], "--yuv-tile-overlap is the overlap of --yuv-fit tile / joint"),
    (["--data_yuv", "c.y4m", "--yuv-fit", "crop", "--yuv-tile-overlap=8"], "--yuv-tile-overlap is the overlap of --yuv-fit tile / joint"),
    (["--yuv-fit", "joint"], "--yuv-fit fits the frames of --data_yuv or --data_frames"),
    (["--data_yuv", "c.y4m", "--yuv-fit", "joint", "--range-recovery", "layer"], "--yuv-fit joint does not combine with --range-recovery layer"),
    (["--data_yuv", "c.y4m", "--yuv-fit", "joint", "--yuv-tile-overlap", "7"], "must be even"),
    (["--data_yuv", "c.y4m", "--yuv-fit", "joint", "--yuv-tile-overlap", "66"], "[0, 64]"),
    (["--data_yuv", "c.y4m", "--yuv-fit", "joint", "--yuv-resize", "box"], "--yuv-resize names the filter of --yuv-fit crop"),
])
def test_sender_refuses(argv, message, capsys):
    from evc_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.parse_args(CFG + argv)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_receiver_refuses_joint_with_range_recovery(capsys, monkeypatch):
    from evc_amd import cli, receiver
    lead = ["--bitstream-dir", "b"] + CFG
    with pytest.raises(SystemExit) as e:
        cli.parse_args(lead + ["--yuv-fit", "joint", "--range-recovery", "layer"], receiver.build_parser(), receiver=True)
    assert e.value.code == 2 and "--yuv-fit joint does not combine with --range-recovery layer" in capsys.readouterr().err
    monkeypatch.setenv("EVC_RANGE_RECOVERY", "layer")            # the environment's default is refused as the flag is
    with pytest.raises(SystemExit):
        cli.parse_args(lead + ["--yuv-fit", "joint"], receiver.build_parser(), receiver=True)
    assert "--range-recovery layer" in capsys.readouterr().err


def test_clip_decoder_refuses_range_recovery_over_a_tiled_network():
    from evc_amd.config import default_config
    from evc_amd.decoder import ClipDecoder
    tiled = types.SimpleNamespace(device="cpu", TILED=True)
    with pytest.raises(ValueError, match="TiledScoreNet"):
        ClipDecoder(tiled, None, default_config(32, 32, 32), None, range_recovery="layer")
    assert ClipDecoder(tiled, None, default_config(32, 32, 32), None, range_recovery="off").range_recovery == "off"


def hand_built_job(shape):
    from evc_amd import container
    keys = [[[[[b"y"] for _ in range(2)] for _ in range(5)], [b"z"]] for _ in range(2)]
    blob = container.pack_job([("key", 2)], keys, shape=shape, codec=(0, 3), seed=7, stream_id=0, vid=4, q=3, thr=0.5,
                              sampler="DDPM", subsample=2, denoise=True)
    return container.unpack_job(blob, expect_codec=(0, 3))


@pytest.mark.parametrize("size,shape,ok", [
    ((40, 56), (1, 1), True), ((64, 64), (1, 1), True), ((65, 64), (2, 1), True), ((144, 160), (3, 3), True),
    ((1080, 1920), (17, 30), True), ((128, 128), (2, 2), True),
    ((40, 56), (2, 2), False), ((128, 128), (1, 1), False), ((144, 160), (2, 2), False), ((65, 64), (1, 1), False),
    ((64, 65), (1, 1), False), ((128, 128), (3, 3), False),
])
def test_latent_shape_and_the_stream_size_check(size, shape, ok):
    from evc_amd import decoder as D
    assert (D.latent_shape(size) == shape) == ok
    job = hand_built_job(shape)
    if ok:
        D.check_stream_size(job, size)
        return
    with pytest.raises(D.StreamSizeError, match="was made for frames of") as e:
        D.check_stream_size(job, size)
    lo, hi = (shape[0] - 1) * 64 + 1, shape[0] * 64
    assert f"{lo}..{hi}" in str(e.value) and f"{size[0]} x {size[1]}" in str(e.value) and "v4 q3 thr 0.50" in str(e.value)


def test_decode_jobs_refuses_a_stream_of_another_size_before_any_work():
    """A stream whose hyper-latent shape is (1, 1) -- a 40 x 56 canvas padded to 64 -- at the generator's own 128 x 128 and at a
    wrong canvas size; no model and no network is touched (there is none)."""
    from evc_amd import sampler as S
    from evc_amd.config import default_config
    from evc_amd.decoder import ClipDecoder, StreamSizeError
    cfg = default_config(32, 32, 128, subsample=2)
    dec = ClipDecoder(types.SimpleNamespace(device="cpu"), None, cfg, S.get_sampler("DDPM"))
    job = hand_built_job((1, 1))
    with pytest.raises(StreamSizeError, match="not for the 128 x 128"):
        dec.decode_jobs([job], models={3: None})
    with pytest.raises(StreamSizeError, match="not for the 80 x 56"):
        dec.decode_jobs([job], models={3: None}, size=(80, 56))
    assert issubclass(StreamSizeError, ValueError)


def test_tile_blend_planes_refuses_channels_that_are_no_multiple_of_three():
    from evc_amd import lib
    with pytest.raises(NotImplementedError, match="multiple of 3"):
        lib.tile_blend_planes(torch.zeros(4, 2, 5, 8, 8), 12, 12, [0, 4], [0, 4])
    with pytest.raises(NotImplementedError):
        lib.tile_blend_planes(torch.zeros(4, 2, 1, 8, 8), 12, 12, [0, 4], [0, 4])


def test_tiled_score_net_refuses_other_networks_at_construction():
    from evc_amd.tiled import TiledScoreNet
    ok = types.SimpleNamespace(ARCH="unetmore", SPADE=False, noise_in_cond=False, forward_label=lambda *a: None, device="cpu")
    t = TiledScoreNet(ok, 32, 8, tile_batch=4)
    assert t.TILED and t.device == "cpu" and t.grid(40, 56) == ([0, 8], [0, 24]) and t.eval() is t
    for change in (dict(ARCH="unetmorepseudo3d"), dict(ARCH="unet"), dict(SPADE=True), dict(noise_in_cond=True)):
        with pytest.raises(NotImplementedError, match="joint generation"):
            TiledScoreNet(types.SimpleNamespace(**{**vars(ok), **change}), 32, 8)
    with pytest.raises(NotImplementedError):
        TiledScoreNet(t, 32, 8)
    with pytest.raises(ValueError, match="overlap"):
        TiledScoreNet(ok, 32, 18)
    with pytest.raises(ValueError):
        TiledScoreNet(ok, 32, 8, tile_batch=0)
