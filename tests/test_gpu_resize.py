"""GPU tests of csrc/resample.hip (evc_resample_h_u8, evc_resample_v_u8) through lib.resample_u8, of video_io's fit="crop"
path and of the command lines that use it.  Pillow's 8-bit resize is integer arithmetic, so every comparison is for equality:
against Pillow's own outputs (tests/golden/resize_pillow.npz) and against the numpy restatement tests/resize_ref.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import resize_ref as R
from conftest import golden

pytestmark = pytest.mark.gpu
CASES, FIXTURES = R.CASES, R.FIXTURES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import evc_amd  # noqa: F401
    from evc_amd import lib
    lib.hip_lib()
    return lib


@pytest.fixture(scope="module")
def G():
    return golden("resize_pillow")


def seeded(seed, *shape, binary=False):
    x = np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    return np.where(x < 128, 0, 255).astype(np.uint8) if binary else x


def differing(got, want):
    return f"{int((got != want).sum())} of {want.size} bytes differ, first at {tuple(int(v[0]) for v in np.nonzero(got != want))}"


@pytest.mark.parametrize("case,kind,filter", FIXTURES)
def test_resample_u8_equals_pillows_output(L, G, case, kind, filter):
    from evc_amd import video_io as V
    n, H, W, oh, ow, _ = CASES[case]
    x = torch.from_numpy(G[f"in_{case}_{kind}"]).cuda()
    got = L.resample_u8(x, oh, ow, filter, box=V.center_box(H, W)).cpu().numpy()
    want = G[f"out_{case}_{kind}_{filter}"]
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), differing(got, want)


# (H, W, box, out_h, out_w, filter): one pass only each, at an odd offset -- the vertical pass on a source that allows no dword
# access (odd width, odd offset), the horizontal pass alone on rows of every alignment; then a row too long for LDS (the direct
# kernel, ksize 6377) and a table too large for LDS beside the rows (ksize 1351: the table read through L2)
GEOMETRIES = [
    (45, 37, (3, 5, 40, 31), 17, 31, "lanczos"),
    (30, 53, (1, 3, 28, 49), 28, 21, "bicubic"),
    (5, 17001, (1, 1, 4, 17000), 4, 16, "lanczos"),
    (9, 3603, (2, 1, 6, 3600), 6, 16, "lanczos"),
]


@pytest.mark.parametrize("H,W,box,oh,ow,filter", GEOMETRIES)
def test_resample_u8_equals_the_restatement(L, H, W, box, oh, ow, filter):
    x = seeded(H * W, 3, 3, H, W, binary=W > 1000)
    want = R.resize(np.ascontiguousarray(R.crop(x, box)), oh, ow, filter)
    got = L.resample_u8(torch.from_numpy(x).cuda(), oh, ow, filter, box=box).cpu().numpy()
    assert np.array_equal(got, want), differing(got, want)


def test_a_frame_alone_and_in_a_batch(L):
    x = torch.from_numpy(seeded(21, 3, 3, 50, 70)).cuda()
    box = (1, 11, 48, 48)
    batch = L.resample_u8(x, 16, 16, "lanczos", box=box)
    for i in range(3):
        assert torch.equal(L.resample_u8(x[i:i + 1].contiguous(), 16, 16, "lanczos", box=box)[0], batch[i])


@pytest.mark.parametrize("box,oh,ow", [((3, 9, 40, 40), 16, 24), ((0, 16, 32, 48), 32, 20), ((5, 1, 41, 63), 20, 63), ((2, 3, 20, 30), 20, 30)])
def test_a_box_equals_its_contiguous_copy(L, box, oh, ow):
    """Plane and row strides: the crop read where it lies against the same crop copied out first."""
    x = torch.from_numpy(seeded(22, 2, 3, 48, 66)).cuda()
    r0, c0, h, w = box
    copy = x[:, :, r0:r0 + h, c0:c0 + w].contiguous()
    for f in ("lanczos", "box"):
        assert torch.equal(L.resample_u8(x, oh, ow, f, box=box), L.resample_u8(copy, oh, ow, f))
    assert np.array_equal(L.resample_u8(x, oh, ow, "lanczos", box=box).cpu().numpy(), R.resize(copy.cpu().numpy(), oh, ow, "lanczos"))


def test_resample_u8_refuses_what_it_cannot_do(L):
    x = torch.zeros((1, 3, 8, 8), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="does not fit"):
        L.resample_u8(x, 4, 4, box=(0, 0, 9, 8))
    with pytest.raises(ValueError, match="filter"):
        L.resample_u8(x, 4, 4, "nearest")


def test_read_clips_fits_a_file_of_another_size(L, tmp_path):
    """A 30-frame 40x24 Y4M -> 16x16: evc_yuv420_to_rgb (uint8) -> centre crop -> the restatement; one line says what was done."""
    import evc_amd  # noqa: F401
    from evc_amd import video_io as V
    rng = np.random.default_rng(8)
    path = str(tmp_path / "wide.y4m")
    V.write_frames(path, [rng.integers(0, 256, V.frame_bytes(40, 24), dtype=np.uint8).tobytes() for _ in range(30)], 40, 24, 25)
    said = []
    clips = V.read_clips(path, fit="crop", size=16, log=said.append)
    assert clips.shape == (1, 30, 3, 16, 16) and clips.dtype == np.uint8
    assert len(said) == 1 and "40x24" in said[0] and "24x24" in said[0] and "lanczos" in said[0] and "16x16" in said[0]
    f = V.open_video(path)
    piece, first, stride = f.chunk(0, 30)
    rgb = L.yuv420_to_rgb(torch.from_numpy(np.array(piece)).cuda(), 30, 24, 40, 8, "bicubic", first=first, stride=stride, dtype=torch.uint8).cpu().numpy()
    assert V.center_box(24, 40) == (0, 8, 24, 24)
    want = R.resize(np.ascontiguousarray(R.crop(rgb, V.center_box(24, 40))), 16, 16, "lanczos")
    assert np.array_equal(clips[0], want), differing(clips[0], want)
    box = V.read_clips(path, fit="crop", size=16, resize="box", log=said.append)
    assert np.array_equal(box[0], R.resize(np.ascontiguousarray(R.crop(rgb, (0, 8, 24, 24))), 16, 16, "box"))
    # frames fitted one at a time are the frames fitted together
    old, V.FIT_GROUP_BYTES = V.FIT_GROUP_BYTES, 1
    try:
        assert np.array_equal(V.read_clips(path, fit="crop", size=16, log=said.append), clips)
    finally:
        V.FIT_GROUP_BYTES = old
    with pytest.raises(ValueError, match="size"):
        V.read_clips(path, fit="crop", log=said.append)


def test_a_file_of_the_models_size_is_read_as_without_fit(L, tmp_path):
    import evc_amd  # noqa: F401
    from evc_amd import video_io as V
    rng = np.random.default_rng(9)
    path = str(tmp_path / "fits.y4m")
    V.write_frames(path, [rng.integers(0, 256, V.frame_bytes(128, 128), dtype=np.uint8).tobytes() for _ in range(30)], 128, 128, 30)
    said = []
    plain = V.read_clips(path, log=said.append)
    assert np.array_equal(V.read_clips(path, fit="crop", size=128, log=said.append), plain) and plain.shape == (1, 30, 3, 128, 128)
    assert said == []


def test_data_frames_of_another_size_take_the_same_path(L, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from evc_amd import video_io as V
    frames = seeded(10, 6, 27, 40, 3)
    for i, f in enumerate(frames):
        Image.fromarray(f).save(tmp_path / ("output_%04d.png" % i))
    said = []
    clips = V.read_frame_clips(str(tmp_path / "output_%04d.png"), frames=3, fit="crop", size=16, log=said.append)
    want = np.stack([np.array(Image.fromarray(np.ascontiguousarray(f[:26, 7:33])).resize((16, 16), Image.LANCZOS)) for f in frames])
    assert np.array_equal(clips.reshape(6, 3, 16, 16), want.transpose(0, 3, 1, 2)) and len(said) == 1


# ---- the command lines ------------------------------------------------------------------------------------------------

def test_sender_and_receiver_fit_a_y4m_of_another_size(L, tmp_path):
    """city_sender.py --data_yuv clip.y4m --yuv-fit crop on a 34-frame 160x144 file, then city_receiver.py with the same two
    flags, in fresh processes, with the reduced random-weight generator and step count of
    test_gpu_yuv.py::test_sender_reads_y4m_and_receiver_writes_the_same_y4m: the sender's .npy outputs and job streams equal
    those of the same run fed the equivalent --data_npy (read_clips(fit="crop", size=128) of the same file), every job prints
    `frames: match` at the receiver, and the same run through --data_frames on PNGs of the file's RGB frames gives the same
    outputs again (that part needs Pillow)."""
    import evc_amd  # noqa: F401
    from evc_amd import video_io as V
    rng = np.random.default_rng(11)
    small = rng.random((34, 3, 9, 10), dtype=np.float32)            # a blocky clip: 16x16 blocks of 160x144
    clip = np.repeat(np.repeat(small, 16, axis=2), 16, axis=3)
    y4m = tmp_path / "clip.y4m"
    V.write_clip(str(y4m), clip, 30)                                 # 34 frames: one clip and a dropped tail
    said = []
    fitted = V.read_clips(str(y4m), fit="crop", size=128, log=said.append)
    assert fitted.shape == (1, 30, 3, 128, 128) and len(said) == 2
    np.save(tmp_path / "clip.npy", fitted)
    model = ["--config", os.path.join(REPO, "configs", "mine.yml"), "--synthetic", "--exp", str(tmp_path / "exp"),
             "--config_mod", "model.ngf=32 model.n_head_channels=32"]
    thresholds = [200.0, -100.0]            # all key frames; everything accepted
    common = ["--start_idx", "0", "--end_idx", "0", "--subsample", "2", "--q", "3", "--policy", "psnr", "--thresholds"] + \
        [str(t) for t in thresholds] + ["--bpp-limit", "1e9", "--batch-invariant"]
    send = [sys.executable, os.path.join(REPO, "city_sender.py")] + model + common
    out, bits, rx = tmp_path / "out", tmp_path / "bits", tmp_path / "rx"
    s = subprocess.run(send + ["--data_yuv", str(y4m), "--yuv-fit", "crop", "--output_path", str(out), "--bitstream-dir", str(bits)],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert s.returncode == 0, s.stdout + s.stderr
    assert "the last 4 frame(s) are dropped" in s.stdout
    assert "160x144 frames, centre crop 144x144 at column 8, row 0, resized to 128x128 (lanczos" in s.stdout
    r = subprocess.run([sys.executable, os.path.join(REPO, "city_receiver.py")] + model +
                       ["--bitstream-dir", str(bits), "--output_path", str(rx), "--data_yuv", str(y4m), "--yuv-fit", "crop"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("frames: match") == len(thresholds) and "MISMATCH" not in r.stdout and "PSNR" in r.stdout, r.stdout
    # the same run from the equivalent .npy: every output file and job stream is the same
    runs = [("npy", ["--data_npy", str(tmp_path / "clip.npy")])]
    try:
        from PIL import Image
        f = V.open_video(str(y4m))
        piece, first, stride = f.chunk(0, 34)
        rgb = L.yuv420_to_rgb(torch.from_numpy(np.array(piece)).cuda(), 34, 144, 160, 8, "bicubic", first=first, stride=stride,
                              dtype=torch.uint8).cpu().numpy()
        (tmp_path / "png").mkdir()
        for i, fr in enumerate(rgb):
            Image.fromarray(np.ascontiguousarray(fr.transpose(1, 2, 0))).save(tmp_path / "png" / ("output_%04d.png" % i))
        runs.append(("png", ["--data_frames", str(tmp_path / "png" / "output_%04d.png"), "--yuv-fit", "crop"]))
    except ImportError:
        pass
    names = sorted(os.listdir(out / "output_0"))
    for tag, flags in runs:
        out2, bits2 = tmp_path / f"out_{tag}", tmp_path / f"bits_{tag}"
        s2 = subprocess.run(send + flags + ["--output_path", str(out2), "--bitstream-dir", str(bits2)], cwd=tmp_path, capture_output=True,
                            text=True, timeout=600)
        assert s2.returncode == 0, s2.stdout + s2.stderr
        assert sorted(os.listdir(out2 / "output_0")) == names
        for n in names:
            assert (out / "output_0" / n).read_bytes() == (out2 / "output_0" / n).read_bytes(), (tag, n)
        for n in sorted(os.listdir(bits)):
            assert (bits / n).read_bytes() == (bits2 / n).read_bytes(), (tag, n)
