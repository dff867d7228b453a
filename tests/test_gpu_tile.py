"""GPU tests of csrc/tile.hip (evc_tile_gather_u8, evc_tile_blend_f32) through lib.tile_gather_u8 / lib.tile_blend, of
video_io's fit="tile" path and of the three command lines that use it (sender, receiver, city_stitch.py).  The reference has
no counterpart, so the yardstick is the numpy restatement tests/tile_ref.py, and every comparison is for equality of bits."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tile_ref as T

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 3


@pytest.fixture(scope="module")
def L():
    import evc_amd  # noqa: F401
    from evc_amd import lib
    lib.hip_lib()
    return lib


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def differing(got, want):
    bad = got != want
    return f"{int(bad.sum())} of {want.size} differ, first at {tuple(int(v[0]) for v in np.nonzero(bad))}"


_cases = {}


def case(H, W, O, S):
    """One geometry's inputs and restated results, computed once and shared: the bytes, their gathered tiles, random float
    tiles in [-1, 2] and their blend."""
    key = (H, W, O, S)
    if key not in _cases:
        rng = np.random.default_rng(1000 + H * W + O)
        oy, ox = T.grid(H, W, S, O)
        x = rng.integers(0, 256, (N, 3, H, W), dtype=np.uint8)
        tiles = (rng.random((len(oy) * len(ox), N, 3, S, S), dtype=np.float32) * np.float32(3) - np.float32(1))
        c = dict(oy=oy, ox=ox, x=x, gathered=T.gather(x, S, oy, ox), tiles=tiles, blended=T.blend(tiles, H, W, oy, ox))
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cases[key] = c
    return _cases[key]


def test_the_geometries_are_what_they_are_meant_to_exercise():
    assert T.grid(40, 70, 32, 8) == ([0, 8], [0, 19, 38])
    assert T.grid(33, 32, 32, 8) == ([0, 1], [0])
    assert T.grid(20, 50, 32, 0) == ([0], [0, 18])
    assert T.grid(64, 96, 32, 0) == ([0, 32], [0, 32, 64])
    assert T.grid(61, 35, 32, 4) == ([0, 14, 29], [0, 3])
    assert T.grid(144, 160, 128, 16) == ([0, 16], [0, 32])


@pytest.mark.parametrize("H,W,O,S", T.GEOMETRIES + T.EXTRA_GEOMETRIES)
def test_gather_equals_the_restatement(L, H, W, O, S):
    c = case(H, W, O, S)
    got = L.tile_gather_u8(torch.tensor(c["x"]).cuda(), S, c["oy"], c["ox"]).cpu().numpy()
    assert got.shape == c["gathered"].shape and got.dtype == np.uint8
    assert np.array_equal(got, c["gathered"]), differing(got, c["gathered"])


@pytest.mark.parametrize("H,W,O,S", T.GEOMETRIES + T.EXTRA_GEOMETRIES)
def test_blend_equals_the_restatement_bit_for_bit(L, H, W, O, S):
    c = case(H, W, O, S)
    got = L.tile_blend(torch.tensor(c["tiles"]).cuda(), H, W, c["oy"], c["ox"]).cpu().numpy()
    assert got.shape == (N, 3, H, W) and got.dtype == np.float32
    assert np.array_equal(got, c["blended"]), differing(got, c["blended"])
    assert same_bits(got, c["blended"])


@pytest.mark.parametrize("H,W,O,S", T.GEOMETRIES + T.EXTRA_GEOMETRIES)
def test_gather_then_blend_gives_the_bytes_back(L, H, W, O, S):
    c = case(H, W, O, S)
    tiles = L.tile_gather_u8(torch.tensor(c["x"]).cuda(), S, c["oy"], c["ox"]).float() / 255.0
    out = L.tile_blend(tiles.contiguous(), H, W, c["oy"], c["ox"]).cpu().numpy()
    assert np.array_equal(np.rint(out * np.float32(255)).astype(np.uint8), c["x"])


def test_nan_and_inf_reach_the_pixels_of_their_tile_only(L):
    H, W, O, S = 40, 70, 8, 32
    c = case(H, W, O, S)
    tiles = c["tiles"].copy()
    tiles[4, 1, 2, 5, 30] = np.nan          # tile (row 1, column 1): frame rows 8 .. 39, columns 19 .. 50 -> pixel (13, 49)
    tiles[4, 2, 0, 31, 0] = np.inf          # -> pixel (39, 19) of frame 2
    want = T.blend(tiles, H, W, c["oy"], c["ox"])
    got = L.tile_blend(torch.from_numpy(tiles).cuda(), H, W, c["oy"], c["ox"]).cpu().numpy()
    bad = ~np.isfinite(want)
    assert int(bad.sum()) == 2 and np.isnan(want[1, 2, 13, 49]) and np.isinf(want[2, 0, 39, 19])
    assert np.array_equal(~np.isfinite(got), bad)
    assert np.isnan(got[1, 2, 13, 49]) and got[2, 0, 39, 19] == np.inf
    assert np.array_equal(got[~bad].view(np.uint32), c["blended"][~bad].view(np.uint32))         # the clean run's bits


@pytest.mark.parametrize("H,W,O,S", [(40, 70, 8, 32), (61, 35, 4, 32)])
def test_a_frame_alone_and_in_a_batch_gives_the_same_bits(L, H, W, O, S):
    c = case(H, W, O, S)
    for n in range(N):
        alone = L.tile_gather_u8(torch.from_numpy(c["x"][n:n + 1].copy()).cuda(), S, c["oy"], c["ox"]).cpu().numpy()
        assert np.array_equal(alone[:, 0], c["gathered"][:, n])
        alone = L.tile_blend(torch.from_numpy(c["tiles"][:, n:n + 1].copy()).cuda(), H, W, c["oy"], c["ox"]).cpu().numpy()
        assert same_bits(alone[0], c["blended"][n])


def test_bad_grids_are_refused_before_any_launch(L):
    x = torch.tensor(case(40, 70, 8, 32)["x"]).cuda()
    tiles = torch.tensor(case(40, 70, 8, 32)["tiles"]).cuda()
    for S, oy, ox in ((32, [0, 9], [0, 19, 38]),            # a row origin beyond H - S = 8
                      (32, [0, 8], [0, 19, 39]),            # a column origin beyond W - S = 38
                      (32, [-1, 8], [0, 19, 38]),
                      (32, [0, 8], [0, 38, 19]),            # not increasing
                      (32, [0, 8], [0, 19, 19]),            # not strictly
                      (64, [0, 0], [0, 6]),                 # an axis shorter than S has one tile
                      ((1 << 24) + 1, [0], [0])):           # S above 2^24: nothing is sized by it
        with pytest.raises(L.EvcKernelError, match="evc_tile_gather_u8"):
            L.tile_gather_u8(x, S, oy, ox)
    for oy, ox in (([0, 9], [0, 19, 38]), ([0, 8], [0, 38, 19]), ([8, 0], [0, 19, 38]),
                   ([0, 8], [0, 19, 37]),                   # the last column is not covered
                   ([0, 8], [1, 19, 38])):                  # nor the first
        with pytest.raises(L.EvcKernelError, match="evc_tile_blend_f32"):
            L.tile_blend(tiles[:len(oy) * len(ox)].contiguous(), 40, 70, oy, ox)
    # the launching entry points themselves refuse: good device origins, bad host origins, and the output keeps its bytes
    lib = L.hip_lib()
    good = [np.asarray(v, dtype=np.int32) for v in ([0, 8], [0, 19, 38])]
    dev = [torch.from_numpy(v).cuda() for v in good]
    bad = np.asarray([0, 9], dtype=np.int32)
    host = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    dst = torch.full((6, N, 3, 32, 32), 7, dtype=torch.uint8, device="cuda")
    out = torch.full((N, 3, 40, 70), 7.0, dtype=torch.float32, device="cuda")
    rc = lib.evc_tile_gather_u8(L.ptr(x), N, 40, 70, 32, 2, 3, host(bad), host(good[1]), L.ptr(dev[0]), L.ptr(dev[1]), L.ptr(dst),
                                L.stream_ptr())
    assert rc == -1
    rc = lib.evc_tile_blend_f32(L.ptr(tiles), N, 40, 70, 32, 2, 3, host(bad), host(good[1]), L.ptr(dev[0]), L.ptr(dev[1]), L.ptr(out),
                                L.stream_ptr())
    assert rc == -1
    rc = lib.evc_tile_gather_u8(L.ptr(x), N, 40, 70, (1 << 24) + 1, 1, 1, host(good[0]), host(good[0]), L.ptr(dev[0]), L.ptr(dev[0]),
                                L.ptr(dst), L.stream_ptr())
    assert rc == -1
    assert lib.evc_tile_gather_u8(None, N, 40, 70, 32, 2, 3, host(good[0]), host(good[1]), L.ptr(dev[0]), L.ptr(dev[1]), L.ptr(dst),
                                  L.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert bool((dst == 7).all()) and bool((out == 7.0).all())


def test_read_clips_tiles_a_y4m_of_another_size(L, tmp_path):
    from evc_amd import video_io as V
    rng = np.random.default_rng(12)
    path = str(tmp_path / "clip.y4m")
    V.write_clip(path, rng.random((34, 3, 144, 160), dtype=np.float32), 30)           # one clip and a dropped tail
    said = []
    got = V.read_clips(path, fit="tile", size=128, overlap=16, log=said.append)
    assert got.shape == (4, 30, 3, 128, 128) and got.dtype == np.uint8
    assert len(said) == 2 and "the last 4 frame(s) are dropped" in said[0]
    assert "160x144 frames as 2x2 tiles of 128x128" in said[1] and "rows at [0, 16], columns at [0, 32]" in said[1] \
        and "video index = clip * 4 + row * 2 + column" in said[1]
    plain = V.read_clips(path, log=lambda m: None)
    assert plain.shape == (1, 30, 3, 144, 160)
    assert np.array_equal(got, T.gather(plain[0], 128, [0, 16], [0, 32]))
    old, V.FIT_GROUP_BYTES = V.FIT_GROUP_BYTES, 1                                   # one frame per group: the same tiles
    try:
        assert np.array_equal(V.read_clips(path, fit="tile", size=128, log=lambda m: None), got)
    finally:
        V.FIT_GROUP_BYTES = old


def test_a_file_of_the_models_size_is_read_as_without_tile(L, tmp_path):
    from evc_amd import video_io as V
    rng = np.random.default_rng(13)
    path = str(tmp_path / "fits.y4m")
    V.write_frames(path, [rng.integers(0, 256, V.frame_bytes(32, 32), dtype=np.uint8).tobytes() for _ in range(30)], 32, 32, 30)
    said = []
    plain = V.read_clips(path, log=said.append)
    assert np.array_equal(V.read_clips(path, fit="tile", size=32, overlap=8, log=said.append), plain) and said == []


# ---- the command lines ------------------------------------------------------------------------------------------------

def test_sender_receiver_and_stitch_code_a_whole_frame(L, tmp_path):
    """city_sender.py --data_yuv clip.y4m --yuv-fit tile on a 34-frame 160x144 file (2x2 tiles = videos 0 .. 3), city_receiver.py
    with the same source flags and city_stitch.py, in fresh processes, with the reduced random-weight generator and flags of
    test_gpu_resize.py::test_sender_and_receiver_fit_a_y4m_of_another_size and one threshold that makes every frame a key
    frame: the manifest is written beside the outputs and the streams, every job matches at the receiver, the stitched clip is
    the restatement's blend of the four decoded tiles bit for bit, a missing tile is named and refused, and a run without the
    tile flags writes no manifest."""
    from evc_amd import video_io as V
    rng = np.random.default_rng(11)
    small = rng.random((34, 3, 9, 10), dtype=np.float32)            # a blocky clip: 16x16 blocks of 160x144
    clip = np.repeat(np.repeat(small, 16, axis=2), 16, axis=3)
    y4m = tmp_path / "clip.y4m"
    V.write_clip(str(y4m), clip, 30)
    model = ["--config", os.path.join(REPO, "configs", "mine.yml"), "--synthetic", "--exp", str(tmp_path / "exp"),
             "--config_mod", "model.ngf=32 model.n_head_channels=32"]
    common = ["--subsample", "2", "--q", "3", "--policy", "psnr", "--thresholds", "200.0", "--bpp-limit", "1e9", "--batch-invariant"]
    send = [sys.executable, os.path.join(REPO, "city_sender.py")] + model + common
    out, bits, rx, full = tmp_path / "out", tmp_path / "bits", tmp_path / "rx", tmp_path / "full"
    run = dict(cwd=tmp_path, capture_output=True, text=True, timeout=600)
    # 1. the sender
    s = subprocess.run(send + ["--data_yuv", str(y4m), "--yuv-fit", "tile", "--start_idx", "0", "--end_idx", "3", "--output_path", str(out),
                               "--bitstream-dir", str(bits)], **run)
    assert s.returncode == 0, s.stdout + s.stderr
    assert "160x144 frames as 2x2 tiles of 128x128" in s.stdout and "the last 4 frame(s) are dropped" in s.stdout
    for d in (out, bits):
        with open(d / "tiles.json") as fh:
            m = json.load(fh)
        assert (m["version"], m["width"], m["height"], m["size"], m["overlap"], m["ny"], m["nx"]) == (1, 160, 144, 128, 16, 2, 2)
        assert (m["oy"], m["ox"], m["clips"], m["frames"], m["source"]) == ([0, 16], [0, 32], 1, 30, "clip.y4m")
        assert V.as_fps(m["fps"]) == 30
    assert sorted(n for n in os.listdir(bits) if n.endswith(".evc")) == ["job_v%d_q3_thr200.00.evc" % v for v in range(4)]
    # 2. the receiver
    r = subprocess.run([sys.executable, os.path.join(REPO, "city_receiver.py")] + model +
                       ["--bitstream-dir", str(bits), "--output_path", str(rx), "--data_yuv", str(y4m), "--yuv-fit", "tile"], **run)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("frames: match") == 4 and "MISMATCH" not in r.stdout, r.stdout
    # 3. the stitch
    stitch = [sys.executable, os.path.join(REPO, "city_stitch.py"), "--tiles", str(out / "tiles.json"), "--decoded", str(rx),
              "--bitstream-dir", str(bits), "--data_yuv", str(y4m), "--ssim"]
    t = subprocess.run(stitch + ["--output_path", str(full)], **run)
    assert t.returncode == 0, t.stdout + t.stderr
    lines = [ln for ln in t.stdout.splitlines() if ln.startswith("stitched_c0_q3_thr200.00:")]
    assert len(lines) == 1, t.stdout
    line = lines[0]
    assert "160x144" in line and "4 tiles" in line and " PSNR " in line and " SSIM " in line and " bpp" in line \
        and "tiles overlap: coded twice" in line, line
    got = np.load(full / "stitched_c0_q3_thr200.00.npy")
    decoded = np.stack([np.load(rx / ("decoded_v%d_q3_thr200.00.npy" % v)) for v in range(4)]).astype(np.float32)
    want = T.blend(decoded, 144, 160, [0, 16], [0, 32])
    assert got.shape == (30, 3, 144, 160) and got.dtype == np.float32 and same_bits(got, want)
    f = V.open_video(str(full / "stitched_c0_q3_thr200.00.y4m"))
    assert (f.width, f.height, f.n_frames, f.fps) == (160, 144, 30, 30)
    # 4. a tile goes missing
    os.remove(rx / "decoded_v2_q3_thr200.00.npy")
    t2 = subprocess.run(stitch + ["--output_path", str(tmp_path / "full2")], **run)
    assert t2.returncode != 0, t2.stdout + t2.stderr
    assert "1 of 4 tile(s) missing: video index(es) 2" in t2.stdout, t2.stdout
    assert not os.path.exists(tmp_path / "full2" / "stitched_c0_q3_thr200.00.npy")
    # 5. without the tile flags nothing new is written
    np.save(tmp_path / "one.npy", V.read_clips(str(y4m), fit="tile", size=128, log=lambda m: None)[:1])
    s2 = subprocess.run(send + ["--data_npy", str(tmp_path / "one.npy"), "--start_idx", "0", "--end_idx", "0", "--output_path",
                                str(tmp_path / "out2"), "--bitstream-dir", str(tmp_path / "bits2")], **run)
    assert s2.returncode == 0, s2.stdout + s2.stderr
    assert "tile manifest" not in s2.stdout and " tiles of " not in s2.stdout
    for d in (tmp_path / "out2", tmp_path / "bits2"):
        assert "tiles.json" not in [n for _, _, names in os.walk(d) for n in names]
    assert sorted(os.listdir(tmp_path / "out2" / "output_0")) == sorted(os.listdir(out / "output_0"))
    for n in sorted(os.listdir(out / "output_0")):          # video 0 is tile 0: the same job either way
        assert (out / "output_0" / n).read_bytes() == (tmp_path / "out2" / "output_0" / n).read_bytes(), n
    assert (bits / "job_v0_q3_thr200.00.evc").read_bytes() == (tmp_path / "bits2" / "job_v0_q3_thr200.00.evc").read_bytes()
