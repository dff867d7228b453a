"""GPU tests of joint generation (DESIGN.md section 8c "Joint generation"): evc_tile_gather_f32 through lib.tile_gather_f32,
``tiled.TiledScoreNet`` over a pixelwise stand-in and over the real reduced network, the three samplers and the policy sweep on
a canvas, and the two command lines with ``--yuv-fit joint``.  The yardstick of gather and blend is the numpy restatement
tests/tile_ref.py; every comparison is for equality of bits."""
import ctypes
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import tile_ref as T

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, H, W, O = 32, 40, 56, 8                      # the canvas of the network tests: 2 x 2 tiles of 32 x 32 at rows 0, 8, columns 0, 24
LABEL = 430


@pytest.fixture(scope="module")
def L():
    import evc_amd  # noqa: F401
    from evc_amd import lib
    lib.hip_lib()
    return lib


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(bits(a), bits(b))


# ---- 1. the gather ----------------------------------------------------------------------------------------------------

_planes = {}


def planes(Hh, Ww, Oo, Ss, C):
    """Random fp32 planes (2, C, H, W) with one NaN and one inf planted, and their restated tiles for N = 2; shared, read-only."""
    key = (Hh, Ww, Oo, Ss, C)
    if key not in _planes:
        rng = np.random.default_rng(7000 + Hh * Ww + C)
        x = rng.standard_normal((2, C, Hh, Ww), dtype=np.float32)
        x[1, C - 1, Hh - 1, Ww - 1] = np.nan                # the last sample: in the last tile, and replicated where an axis is short
        x[0, 0, Hh // 2, Ww // 2] = np.inf
        oy, ox = T.grid(Hh, Ww, Ss, Oo)
        c = dict(x=x, oy=oy, ox=ox, tiles=T.gather(x, Ss, oy, ox))
        x.setflags(write=False), c["tiles"].setflags(write=False)
        _planes[key] = c
    return _planes[key]


GATHER_CASES = [g + (C,) for g in T.GEOMETRIES if g[3] != 128 for C in (6, 15)] + [T.EXTRA_GEOMETRIES[1] + (3,)]


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("Hh,Ww,Oo,Ss,C", GATHER_CASES)
def test_gather_f32_equals_the_restatement_bit_for_bit(L, Hh, Ww, Oo, Ss, C, N):
    c = planes(Hh, Ww, Oo, Ss, C)
    x = c["x"][2 - N:].copy()                                # N = 1: sample 1 alone -- the same bits as inside the batch
    got = L.tile_gather_f32(torch.from_numpy(x).cuda(), Ss, c["oy"], c["ox"]).cpu().numpy()
    want = c["tiles"][:, 2 - N:]
    assert got.shape == (len(c["oy"]) * len(c["ox"]), N, C, Ss, Ss)
    assert same_bits(got, np.ascontiguousarray(want)), f"{int((bits(got) != bits(np.ascontiguousarray(want))).sum())} words differ"
    assert np.isnan(got).sum() == np.isnan(want).sum() >= 1 and np.isinf(got).sum() == np.isinf(want).sum()


def test_gather_f32_refuses_bad_grids_before_any_launch(L):
    c = planes(40, 70, 8, 32, 6)
    x = torch.from_numpy(c["x"].copy()).cuda()
    for Ss, oy, ox in ((32, [0, 9], [0, 19, 38]), (32, [0, 8], [0, 19, 39]), (32, [-1, 8], [0, 19, 38]), (32, [0, 8], [0, 38, 19]),
                       (32, [0, 8], [0, 19, 19]), (64, [0, 0], [0, 6]), ((1 << 24) + 1, [0], [0])):
        with pytest.raises(L.EvcKernelError, match="evc_tile_gather_f32"):
            L.tile_gather_f32(x, Ss, oy, ox)
    lib = L.hip_lib()
    good = [np.asarray(v, dtype=np.int32) for v in ([0, 8], [0, 19, 38])]
    dev = [torch.from_numpy(v).cuda() for v in good]
    bad = np.asarray([0, 9], dtype=np.int32)
    host = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    dst = torch.full((6, 2, 6, 32, 32), 7.0, dtype=torch.float32, device="cuda")
    call = lambda src, C, hy: lib.evc_tile_gather_f32(src, 2, C, 40, 70, 32, 2, 3, host(hy), host(good[1]), L.ptr(dev[0]),  # noqa: E731
                                                      L.ptr(dev[1]), L.ptr(dst), L.stream_ptr())
    assert call(L.ptr(x), 6, bad) == -1                       # good device origins, bad host origins
    assert call(L.ptr(x), 0, good[0]) == -1 and call(L.ptr(x), (1 << 24) + 1, good[0]) == -1
    assert call(None, 6, good[0]) == -1
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all())
    assert call(L.ptr(x), 6, good[0]) == 0                    # and the same call with good arguments runs
    torch.cuda.synchronize()
    assert same_bits(dst.cpu().numpy(), np.ascontiguousarray(c["tiles"]))


# ---- 2. a pixelwise stand-in network ----------------------------------------------------------------------------------

class Pixelwise:
    """eps[:, c] = x[:, c] + cond[:, c % 6]: what it returns for a pixel depends on that pixel alone, so the tent-weighted mean
    over the tiles that cover a pixel is the value itself -- exactly, on the k / 256 grid (every weighted partial sum is an
    integer below 2^24 in units of 1 / 256: weights <= 256, at most 9 tiles, |eps| < 2)."""
    ARCH, SPADE, noise_in_cond, batch_invariant = "unetmore", False, False, False

    def __init__(self):
        self.device = torch.device("cuda")
        self.launches = []

    def forward_label(self, x, label, cond=None):
        self.launches.append(x.shape[0])
        assert x.shape[-2:] == cond.shape[-2:] == (S, S) and x.is_contiguous() and cond.is_contiguous()
        return x + cond[:, [c % 6 for c in range(x.shape[1])]]

    def __call__(self, x, labels, cond=None, cond_mask=None):
        assert len(labels) == x.shape[0]
        return self.forward_label(x, labels[0], cond)


def grid_values(seed, *shape):
    k = np.random.default_rng(seed).integers(-255, 256, shape)
    return torch.from_numpy((k / 256.0).astype(np.float32)).cuda()


@pytest.mark.parametrize("Hh,Ww,Oo", [(40, 56, 8), (61, 35, 4), (20, 50, 0)])
def test_a_pixelwise_network_gives_its_own_function_of_the_canvas_exactly(L, Hh, Ww, Oo):
    from evc_amd.tiled import TiledScoreNet
    inner = Pixelwise()
    net = TiledScoreNet(inner, S, Oo, tile_batch=3)
    x, cond = grid_values(Hh + Ww, 2, 15, Hh, Ww), grid_values(Hh * Ww, 2, 6, Hh, Ww)
    want = x + cond[:, [c % 6 for c in range(15)]]
    oy, ox = T.grid(Hh, Ww, S, Oo)
    rows = 2 * len(oy) * len(ox)
    got = net.forward_label(x, LABEL, cond)
    assert got.shape == (2, 15, Hh, Ww) and torch.equal(got, want)
    assert inner.launches == [3] * (rows // 3) + ([rows % 3] if rows % 3 else [])
    # the reference call shape: labels per sample, repeated per tile
    assert torch.equal(net(x, torch.tensor([LABEL, LABEL]), cond=cond), want)
    # the conditioning tiles: gathered once for one tensor however often it is passed, again for a new tensor
    assert net.cond_gathers == 1
    for _ in range(3):
        net.forward_label(x, LABEL - 1, cond)
    assert net.cond_gathers == 1
    other = cond.clone()
    assert torch.equal(net.forward_label(x, LABEL, other), want) and net.cond_gathers == 2
    assert torch.equal(net.forward_label(x, LABEL, cond), want) and net.cond_gathers == 3


def test_at_the_models_own_size_the_wrapper_is_invisible(L):
    from evc_amd.tiled import TiledScoreNet
    inner = Pixelwise()
    net = TiledScoreNet(inner, S, 8, tile_batch=1)
    x, cond = grid_values(1, 3, 15, S, S), grid_values(2, 3, 6, S, S)
    got = net.forward_label(x, LABEL, cond)
    assert inner.launches == [3] and net.cond_gathers == 0          # one inner call on the tensors as they are
    assert torch.equal(got, Pixelwise().forward_label(x, LABEL, cond))


# ---- 3. the real reduced network ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def real(L):
    from evc_amd.scorenet import ScoreNet
    from oracle.scorenet import Dims, seeded_params
    from test_gpu_scorenet import make_config
    from conftest import rnd
    net = ScoreNet(make_config(32, 32, 32), seeded_params(Dims(ngf=32, n_head_channels=32, image_size=32), 41))
    x, cond = rnd(52, 2, 15, H, W), rnd(53, 2, 6, H, W)
    oy, ox = T.grid(H, W, S, O)
    assert (oy, ox) == ([0, 8], [0, 24])
    return types.SimpleNamespace(net=net, inv=net.invariant_view(), x=x, cond=cond, oy=oy, ox=ox,
                                 xt=torch.from_numpy(T.gather(x.numpy(), S, oy, ox)).reshape(8, 15, S, S).cuda(),
                                 ct=torch.from_numpy(T.gather(cond.numpy(), S, oy, ox)).reshape(8, 6, S, S).cuda())


def composed(real, inner, chunk):
    """tile_ref.blend of the inner network's output on tile_ref.gather of the inputs, the inner launches ``chunk`` rows each."""
    eps = torch.cat([inner.forward_label(real.xt[lo:lo + chunk].contiguous(), LABEL, real.ct[lo:lo + chunk].contiguous())
                     for lo in range(0, 8, chunk)], 0)
    return T.blend(eps.cpu().numpy().reshape(4, 2, 15, S, S), H, W, real.oy, real.ox)


def test_real_network_default_mode_is_the_composition_bit_for_bit(L, real):
    from evc_amd.tiled import TiledScoreNet
    net = TiledScoreNet(real.net, S, O, tile_batch=8)                # all T * B tiles in one inner launch, on both sides
    got = net.forward_label(real.x.cuda(), LABEL, real.cond.cuda()).cpu().numpy()
    want = composed(real, real.net, 8)
    assert np.isfinite(want).all() and float(np.abs(want).max()) > 1e-3
    assert same_bits(got, want), f"max abs difference {float(np.abs(got - want).max()):.3e}"
    assert net.alphas is real.net.alphas and net.device == real.net.device      # everything else is the inner network's


def test_real_network_invariant_view_does_not_depend_on_tile_batch(L, real):
    from evc_amd.tiled import TiledScoreNet
    want = composed(real, real.inv, 3)
    for tb in (1, 8):
        net = TiledScoreNet(real.net, S, O, tile_batch=tb).invariant_view()
        assert net.TILED and net.inner.batch_invariant and net.tile_batch == tb and net.invariant_view() is net
        got = net.forward_label(real.x.cuda(), LABEL, real.cond.cuda()).cpu().numpy()
        assert same_bits(got, want), (tb, float(np.abs(got - want).max()))
    # a canvas alone and the same canvas as sample 1 of the pair
    alone = TiledScoreNet(real.inv, S, O, tile_batch=5).forward_label(real.x[1:].cuda().contiguous(), LABEL, real.cond[1:].cuda().contiguous())
    assert same_bits(alone.cpu().numpy()[0], want[1])


def test_a_nan_outside_a_tiles_footprint_leaves_its_exclusive_pixels_finite(L, real):
    """Where every tile is a launch or a sample of its own: the default network one tile per launch, and the batch-invariant
    view (one bound word per sample) with all tiles in one launch.  (The default mode shares its element-bound words across the
    samples of a launch, so there a NaN is only kept inside its launch.)"""
    from evc_amd.tiled import TiledScoreNet
    x = real.x.clone()
    x[0, 7, 39, 55] = float("nan")            # covered by tile 3 alone (rows 8 .. 39, columns 24 .. 55)
    for net in (TiledScoreNet(real.net, S, O, tile_batch=1), TiledScoreNet(real.inv, S, O, tile_batch=8)):
        got = net.forward_label(x.cuda(), LABEL, real.cond.cuda()).cpu().numpy()
        assert np.isfinite(got[0, :, :8, :24]).all()              # tile 0's exclusive pixels: no other tile covers them
        assert np.isfinite(got[0, :, :8, :]).all() and np.isfinite(got[0, :, :, :24]).all()      # nor does tile 3 reach these
        assert not np.isfinite(got[0, :, 32:, 32:]).any()         # tile 3's exclusive pixels carry it
        assert np.isfinite(got[1]).all()                          # and the other sample is untouched
    L.range_events(reset=True)
    L.site_events(real.net, reset=True)


# ---- 4. the samplers ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,steps", [("DDPM", 5), ("DDIM", 5), ("FPNDM", 10)])
def test_samplers_run_on_a_canvas(L, real, name, steps):
    from evc_amd import sampler as Sm
    from evc_amd.tiled import TiledScoreNet
    from conftest import rnd
    fn = Sm.get_sampler(name)
    noises = {i: rnd(300 + i, 2, 15, H, W).cuda() for i in range(steps + 1)}
    x_T = rnd(299, 2, 15, H, W).cuda()

    def run(net, lo, hi):
        out = fn(x_T[lo:hi].contiguous(), net, cond=real.cond[lo:hi].cuda().contiguous(), subsample_steps=steps, denoise=True,
                 clip_before=True, final_only=True, noise_fn=lambda i, x: noises[i][lo:hi].contiguous())
        assert out.shape == (1, hi - lo, 15, H, W) and bool(torch.isfinite(out).all())
        return out

    run(TiledScoreNet(real.net, S, O, tile_batch=8), 0, 2)
    inv = TiledScoreNet(real.net, S, O, tile_batch=3).invariant_view()
    pair, one = run(inv, 0, 2), run(inv, 0, 1)
    assert torch.equal(pair[0, 0], one[0, 0])


# ---- 5. the policy sweep and its streams -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sweep(L, real):
    from evc_amd import sampler as Sm, synthetic
    from evc_amd.config import default_config
    from evc_amd.elic import ElicModel
    cfg = default_config(32, 32, 32, subsample=2)
    rng = np.random.default_rng(77)
    small = rng.random((2, 30, 3, 5, 7), dtype=np.float32)              # blocky 40 x 56 clips
    clips = {v: torch.from_numpy(np.repeat(np.repeat(small[v], 8, axis=2), 8, axis=3)) for v in (0, 1)}
    return types.SimpleNamespace(cfg=cfg, models={3: ElicModel(synthetic.elic_state_dict(3))}, clips=clips,
                                 sampler=Sm.get_sampler("DDPM"))


def decoder_of(sweep, real, tile_batch):
    from evc_amd.decoder import ClipDecoder
    from evc_amd.tiled import TiledScoreNet
    return ClipDecoder(TiledScoreNet(real.net, S, O, tile_batch=tile_batch), None, sweep.cfg, sweep.sampler)


def stream_of(L, sweep, r, vid):
    from evc_amd import container
    extra = dict(plan=(container.PLAN_INVARIANT, L.invariant_plan_revision()), crc=container.frames_crc(r["x"]))
    if r["n_trials"] > 1:
        extra.update(trials=r["trials"], n_trials=r["n_trials"])
    tag = sweep.models[3].codec_tag()
    blob = container.pack_job(r["segments"], r["key_strings"], r["shape"], tag, r["seed"], r["stream_id"], vid, 3, r["thr"],
                              "DDPM", sweep.cfg.sampling.subsample, sweep.cfg.sampling.denoise, **extra)
    return container.unpack_job(blob, expect_codec=tag, expect_plan_revision=L.invariant_plan_revision())


@pytest.mark.parametrize("shared", [{}, dict(trials=2, noise_streams="group", share=True)], ids=["plain", "trials-shared"])
def test_policy_on_a_canvas_and_any_receiver_reproduces_it(L, real, sweep, shared):
    from evc_amd import container, policy as P
    from evc_amd.decoder import StreamSizeError
    res = P.run_policy(decoder_of(sweep, real, 4), sweep.models, sweep.clips, [3], [0.0, 200.0], P.PsnrMetric(), patch=64,
                       max_batch=8, seed=5, bpp_limit=1e9, noise="evc", batch_invariant=True, **shared)
    sent = [(vid, r) for vid in (0, 1) for r in res[(vid, 3)]]
    assert [r["thr"] for _, r in sent] == [0.0, 200.0] * 2
    for vid, r in sent:
        assert r["x"].shape == (30, 3, H, W) and np.isfinite(r["x"]).all() and r["shape"] == (1, 1) and r["invariant"]
        assert r["d"].tolist() == ([1, 1] + [0] * 28 if r["thr"] == 0.0 else [1] * 30)
        assert r["bpp"] == (sum(r["bits"]) + r["trial_bits"]) / H / W / 30
    jobs = [stream_of(L, sweep, r, vid) for vid, r in sent]
    for tile_batch, max_batch in ((1, 5), (4, 1), (4, 5)):
        out = decoder_of(sweep, real, tile_batch).decode_jobs(jobs, max_batch=max_batch, models=sweep.models, size=(H, W),
                                                             share=bool(shared))
        for (vid, r), job, x in zip(sent, jobs, out):
            x = x.cpu().numpy()
            assert x.shape == (30, 3, H, W) and np.array_equal(x, r["x"]), (tile_batch, max_batch, vid, r["thr"])
            assert container.frames_crc(x) == job["crc"]
    for wrong in ((128, 128), (H, 72), (72, W)):
        with pytest.raises(StreamSizeError, match="was made for frames of 1..64 x 1..64"):
            decoder_of(sweep, real, 4).decode_jobs(jobs, models=sweep.models, size=wrong)


def test_decode_with_a_mask_generates_at_the_canvas_size(L, real, sweep):
    """``ClipDecoder.decode(size=)`` (the mask policy under --yuv-fit joint): the key frames come out of ELIC padded to 64 x 64
    and are cropped to the canvas before anything is generated from them, so the generated frames are those of ``generate`` on
    the cropped pair."""
    from evc_amd.decoder import ClipDecoder, all_generated_mask
    from evc_amd.elic import compress_padded
    from evc_amd.tiled import TiledScoreNet
    model = sweep.models[3]
    dec = ClipDecoder(TiledScoreNet(real.net, S, O, tile_batch=8), model, sweep.cfg, sweep.sampler)
    gt = torch.stack([sweep.clips[0][:2], sweep.clips[1][:2]]).cuda()                 # (2 clips, 2 key frames, 3, 40, 56)
    enc = [compress_padded(model, gt[:, f], 64) for f in (0, 1)]
    noises = {}

    def noise(tag, shape):
        if tag not in noises:
            noises[tag] = torch.randn(shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(len(noises)))
        return noises[tag]

    mask = all_generated_mask(frames=7)
    out = dec.decode(mask, [e["strings"] for e in enc], enc[0]["shape"], frames=7, noise_fn=noise, size=(H, W))
    assert out.shape == (2, 7, 3, H, W) and bool(torch.isfinite(out).all())
    from evc_amd import keystrings as KS
    both = model.decompress(KS.merge([e["strings"] for e in enc]), enc[0]["shape"])["x_hat"]         # the decoder's own call
    assert both.shape == (4, 3, 64, 64)
    keys = both[:, :, :H, :W].reshape(2, 2, 3, H, W).permute(1, 0, 2, 3, 4)
    assert torch.equal(out[:, :2], keys)
    assert torch.equal(out[:, 2:], dec.generate(keys.contiguous(), noise_fn=noise))


# ---- 6. the command lines ----------------------------------------------------------------------------------------------

def test_sender_and_receiver_generate_a_whole_frame_jointly(L, tmp_path):
    """city_sender.py --data_yuv clip.y4m --yuv-fit joint on the 34-frame 160x144 file of
    test_gpu_tile.py::test_sender_receiver_and_stitch_code_a_whole_frame, with its reduced generator and flags and the
    thresholds 0.0 (everything after the first pair generated) and 200.0 (key frames only): the grid line, canvas.json beside
    the outputs and the streams, one stream per threshold; city_receiver.py --yuv-fit joint with no source reproduces both;
    without canvas.json it names the file; and on a source of the model's own size the flag changes no byte."""
    from evc_amd import video_io as V
    rng = np.random.default_rng(11)
    small = rng.random((34, 3, 9, 10), dtype=np.float32)
    V.write_clip(str(tmp_path / "clip.y4m"), np.repeat(np.repeat(small, 16, axis=2), 16, axis=3), 30)
    model = ["--config", os.path.join(REPO, "configs", "mine.yml"), "--synthetic", "--exp", str(tmp_path / "exp"),
             "--config_mod", "model.ngf=32 model.n_head_channels=32"]
    common = ["--subsample", "2", "--q", "3", "--policy", "psnr", "--bpp-limit", "1e9", "--batch-invariant", "--start_idx", "0",
              "--end_idx", "0"]
    send = [sys.executable, os.path.join(REPO, "city_sender.py")] + model + common
    receive = [sys.executable, os.path.join(REPO, "city_receiver.py")] + model
    out, bits_dir, rx = tmp_path / "out", tmp_path / "bits", tmp_path / "rx"
    run = dict(cwd=tmp_path, capture_output=True, text=True, timeout=600)
    # 1. the sender
    s = subprocess.run(send + ["--thresholds", "0.0", "200.0", "--data_yuv", str(tmp_path / "clip.y4m"), "--yuv-fit", "joint",
                               "--output_path", str(out), "--bitstream-dir", str(bits_dir)], **run)
    assert s.returncode == 0, s.stdout + s.stderr
    assert "160x144 frames, joint generation over 2 x 2 tiles of 128x128 (overlap 16)" in s.stdout, s.stdout
    assert "the last 4 frame(s) are dropped" in s.stdout
    for d in (out, bits_dir):
        with open(d / "canvas.json") as fh:
            m = json.load(fh)
        assert (m["version"], m["width"], m["height"], m["size"], m["overlap"]) == (1, 160, 144, 128, 16)
        assert (m["oy"], m["ox"], m["clips"], m["frames"], m["source"]) == ([0, 16], [0, 32], 1, 30, "clip.y4m")
        assert V.as_fps(m["fps"]) == 30 and not os.path.exists(d / "tiles.json")
    assert sorted(n for n in os.listdir(bits_dir) if n.endswith(".evc")) == ["job_v0_q3_thr0.00.evc", "job_v0_q3_thr200.00.evc"]
    sent = np.load(out / "output_0" / "city_output_npy_idx0_q3_thr0.00.npy")           # originals over decoded, frames side by side
    assert sent.shape == (2 * 144, 30 * 160, 3)
    # 2. the receiver: no source flags
    r = subprocess.run(receive + ["--bitstream-dir", str(bits_dir), "--output_path", str(rx), "--yuv-fit", "joint"], **run)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("frames: match") == 2 and "MISMATCH" not in r.stdout, r.stdout
    for thr in ("0.00", "200.00"):
        x = np.load(rx / f"decoded_v0_q3_thr{thr}.npy")
        assert x.shape == (30, 3, 144, 160) and x.dtype == np.float32
    assert np.array_equal(np.concatenate(list(x.transpose(0, 2, 3, 1)), axis=1),
                          np.load(out / "output_0" / "city_output_npy_idx0_q3_thr200.00.npy")[144:])
    # 3. without the manifest the receiver names it; without the flag it names the size the streams were made for
    os.rename(bits_dir / "canvas.json", tmp_path / "canvas.json")
    r2 = subprocess.run(receive + ["--bitstream-dir", str(bits_dir), "--output_path", str(tmp_path / "rx2"), "--yuv-fit", "joint"], **run)
    assert r2.returncode != 0 and "canvas.json" in r2.stderr and str(bits_dir) in r2.stderr, r2.stdout + r2.stderr
    r3 = subprocess.run(receive + ["--bitstream-dir", str(bits_dir), "--output_path", str(tmp_path / "rx3")], **run)
    assert r3.returncode != 0 and "was made for frames of 129..192 x 129..192" in r3.stderr, r3.stdout + r3.stderr
    # 4. a source of the model's own size: the flag changes nothing and writes no manifest
    V.write_clip(str(tmp_path / "own.y4m"), np.repeat(np.repeat(small[:30, :, :8, :8], 16, axis=2), 16, axis=3), 30)
    dirs = []
    for k, flag in enumerate(([], ["--yuv-fit", "joint"])):
        o, b = tmp_path / f"own_out{k}", tmp_path / f"own_bits{k}"
        s2 = subprocess.run(send + ["--thresholds", "200.0", "--data_yuv", str(tmp_path / "own.y4m"), "--output_path", str(o),
                                    "--bitstream-dir", str(b)] + flag, **run)
        assert s2.returncode == 0, s2.stdout + s2.stderr
        assert "joint generation" not in s2.stdout and "canvas manifest" not in s2.stdout
        for d in (o, b):
            assert "canvas.json" not in [n for _, _, names in os.walk(d) for n in names]
        dirs.append((o, b))
    (o0, b0), (o1, b1) = dirs
    assert sorted(os.listdir(o0 / "output_0")) == sorted(os.listdir(o1 / "output_0")) and len(os.listdir(o0 / "output_0")) >= 4
    for n in sorted(os.listdir(o0 / "output_0")):
        assert (o0 / "output_0" / n).read_bytes() == (o1 / "output_0" / n).read_bytes(), n
    assert (b0 / "job_v0_q3_thr200.00.evc").read_bytes() == (b1 / "job_v0_q3_thr200.00.evc").read_bytes()
