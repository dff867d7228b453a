"""Host tests of the reporting module (evc_amd/report.py): the files ``Collector`` writes per video for every combination of
reporting flags, their shapes, dtypes and contents, the printed lines of the sender, the receiver and the stitcher, and how often
``Measurer`` asks its backends for the originals' features.  Every metric backend is a stub that returns seeded numbers and
logs them.  No GPU."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import evc_amd  # noqa: F401
from evc_amd import cli, policy as P, report as R

BPPS = {0: [0.10, 0.25, 0.18, 0.40], 1: [0.30, 0.20]}      # video 0: four jobs (rd_envelope's hull path); video 1: pass-through
HIGHER = {"psnr": True, "psnr_yuv": True, "ssim": True, "ssim_yuv": True, "lpips_vgg": False, "fid": False, "fvd": False,
          "lpips": False}


class Stubs:
    """Backend, LPIPS, Inception and I3D stand-ins: seeded numbers, every returned value logged under its metric's name."""
    net = "vgg"

    def __init__(self):
        self.rng = np.random.default_rng(7)
        self.log = {}
        self.i3d_batches, self.pairs = [], 0

    def _out(self, name, value):
        self.log.setdefault(name, []).append(value)
        return value

    def ssim_frames(self, x, gt):
        assert x.dtype == gt.dtype == torch.float32 and x.is_contiguous() and gt.is_contiguous()
        return self._out("ssim", self.rng.random(len(x)))

    def spatial_mean(self, x, gt):                       # the LPIPS object
        assert x.dtype == gt.dtype == torch.float32 and x.shape == gt.shape
        v = torch.from_numpy(self.rng.random(len(x)).astype(np.float32))
        self._out("lpips_vgg", v.double().numpy())
        return v

    def inception_features(self, images, net, dims):
        assert net == "inception" and dims == 192 and images.dtype == torch.float32
        return self._out("features", self.rng.standard_normal((len(images), 4)).astype(np.float32))

    def fid_and_pr(self, real, gen, k=3):
        assert k == 3 and real.shape == gen.shape
        fv, pv, rv = (float(t) for t in self.rng.random(3))
        self._out("fid", fv), self._out("pr", (pv, rv))
        return fv, pv, rv

    def i3d(self, clips):
        assert clips.dtype == torch.float32 and clips.shape[1:] == (30, 3, 8, 8)
        self.i3d_batches.append(len(clips))
        return torch.from_numpy(self.rng.standard_normal((len(clips), 5)).astype(np.float32))

    def frechet_distance(self, a, b):
        assert a.shape == b.shape == (2, 5) and (a[0] == a[1]).all() and (b[0] == b[1]).all()     # the twice-repeated features
        return self._out("fvd", float(np.abs(a[0] - b[0]).sum()))

    def yuv_metric_clips(self, x, gt):
        self.pairs += 1
        return ("pair", self.pairs)

    def psnr_yuv(self, x, gt, clips=None):
        assert clips == ("pair", self.pairs)
        return self._out("psnr_yuv", 30 + self.rng.random(len(x)))

    def ssim_yuv(self, x, gt, clips=None):
        assert clips == ("pair", self.pairs)
        return self._out("ssim_yuv", self.rng.random(len(x)))


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"metric backend {name} touched")


def clips(seed, n=1):
    return np.random.default_rng(seed).random((n, 30, 3, 8, 8)).astype(np.float32)


def run_videos(root, ssim=False, yuv=False, lpips=False, fid=False, fvd=False, rule=False):
    """Two videos through Measurer and Collector as the sender drives them: one ``measure_jobs`` call per video, the jobs added
    in report order, then ``save``.  -> (stubs, {vid: [psnr of every job]}, {vid: [the rule's distances]})."""
    s = Stubs()
    m = R.Measurer(ssim=ssim, lpips=s if lpips else None, inception="inception" if fid else None, fid_dims=192,
                   i3d=s.i3d if fvd else None, yuv=yuv, backend=s)
    c = R.Collector(net=m.net)
    psnr, rule_vals = {}, {}
    for vid, bpps in BPPS.items():
        gt, xs = clips(100 + vid)[0], clips(200 + vid, len(bpps))
        for bpp, x, v in zip(bpps, xs, m.measure_jobs([(vid, x, gt) for x in xs])):
            psnr.setdefault(vid, []).append([10 * np.log10(1.0 / np.mean((x[t].astype(np.float64) - gt[t]) ** 2)) for t in range(30)])
            if rule:
                rule_vals.setdefault(vid, []).append(s.rng.random(30))
                v = {**v, "policy_lpips": rule_vals[vid][-1]}
            c.add(vid, bpp, v)
    c.save(str(root))
    return s, psnr, rule_vals


FRAMES = lambda stem: {f"{stem}_%d.npy", f"{stem}_frames_%d.npy"}          # noqa: E731
ALWAYS = FRAMES("psnr") | {"bpp_%d.npy"}
FID_FILES = {"fid_%d.npy", "fid_values_%d.npy", "pr_values_%d.npy"}
FVD_FILES = {"fvd_%d.npy", "fvd_values_%d.npy"}
COMBINATIONS = [
    (dict(), ALWAYS),
    (dict(ssim=True), ALWAYS | FRAMES("ssim")),
    (dict(ssim=True, yuv=True), ALWAYS | FRAMES("ssim") | FRAMES("psnr_yuv") | FRAMES("ssim_yuv")),
    (dict(lpips=True), ALWAYS | FRAMES("lpips_vgg")),
    (dict(fid=True), ALWAYS | FID_FILES),
    (dict(fvd=True), ALWAYS | FVD_FILES),
    (dict(rule=True), ALWAYS | FRAMES("lpips")),
    (dict(ssim=True, yuv=True, lpips=True, fid=True, fvd=True, rule=True),
     ALWAYS | FRAMES("ssim") | FRAMES("psnr_yuv") | FRAMES("ssim_yuv") | FRAMES("lpips_vgg") | FID_FILES | FVD_FILES | FRAMES("lpips")),
]


@pytest.mark.parametrize("flags,names", COMBINATIONS, ids=["none", "ssim", "ssim+yuv", "lpips", "fid", "fvd", "rule", "all"])
def test_files_of_every_flag_combination(flags, names, tmp_path):
    s, psnr, rule_vals = run_videos(tmp_path, **flags)
    assert sorted(os.listdir(tmp_path)) == ["output_0", "output_1"]
    first = 0
    for vid, bpps in BPPS.items():
        root = tmp_path / f"output_{vid}"
        assert set(os.listdir(root)) == {n % vid for n in names}
        got = {n: np.load(root / (n % vid)) for n in names}
        assert all(a.dtype == np.float64 for a in got.values())
        jobs = slice(first, first + len(bpps))
        first += len(bpps)
        assert np.array_equal(got["bpp_%d.npy"], np.asarray(bpps))
        logged = {k: np.asarray(v[jobs]) for k, v in s.log.items()}
        logged["psnr"] = np.asarray(psnr[vid])
        if rule_vals:
            logged["lpips"] = np.asarray(rule_vals[vid])
        for stem, higher in HIGHER.items():
            if f"{stem}_%d.npy" not in names:
                continue
            scalar = stem in ("fid", "fvd")
            raw = got[f"{stem}_values_%d.npy" if scalar else f"{stem}_frames_%d.npy"]
            assert raw.shape == ((len(bpps),) if scalar else (len(bpps), 30))
            assert np.array_equal(raw, logged[stem])                      # the stub's numbers, in report order
            want = P.rd_envelope(bpps, logged[stem] if scalar else np.mean(logged[stem], 1), higher)
            assert got[f"{stem}_%d.npy"].shape == want.shape and want.shape[0] == 2 and np.array_equal(got[f"{stem}_%d.npy"], want)
        if "pr_values_%d.npy" in names:
            assert got["pr_values_%d.npy"].shape == (len(bpps), 2) and np.array_equal(got["pr_values_%d.npy"], logged["pr"])


def test_the_originals_features_are_computed_once_per_video(tmp_path):
    s, _, _ = run_videos(tmp_path, fid=True, fvd=True, yuv=True)
    jobs = sum(len(b) for b in BPPS.values())
    assert len(s.log["features"]) == jobs + len(BPPS)                  # Inception: every decoded clip, every original once
    assert s.i3d_batches == [1, 4, 1, 2]                               # I3D per call: the new original, then all decoded clips
    assert s.pairs == jobs                                             # one YUV round-trip pair per job
    m = R.Measurer(inception="inception", fid_dims=192, i3d=s.i3d, backend=s)
    for _ in range(2):                                                 # a second call on the same video: no new original
        m.measure_jobs([(0, clips(1)[0], clips(2)[0])])
    assert len(s.log["features"]) == jobs + len(BPPS) + 3 and s.i3d_batches[4:] == [1, 1, 1]


def test_a_run_without_opt_in_flags_touches_no_backend(tmp_path):
    m = R.Measurer(backend=Untouchable())
    x, gt = clips(3)[0], clips(4)[0]
    (v,) = m.measure_jobs([(0, x, gt)])
    assert list(v) == ["psnr"] and len(v["psnr"]) == 30 and v["psnr"][0] == R.cal_psnr(x[0], gt[0]) == cli.cal_psnr(x[0], gt[0])
    assert P.cal_psnr is R.cal_psnr and m.net is None


VALUES = {"psnr": [30.0] * 30, "fvd": 3.25, "ssim": np.full(30, 0.9), "lpips": np.full(30, 0.125), "fid": 12.5, "pr": (0.5, 0.25)}


def test_sender_lines(tmp_path):
    class Fixed:
        net = "vgg"

        def measure_jobs(self, jobs):
            return [dict(VALUES) for _ in jobs]
    lines = []
    run = SimpleNamespace(args=SimpleNamespace(output_path=str(tmp_path), yuv_out=False), fps=30, measurer=Fixed(),
                          collector=R.Collector(net="vgg"), log=lambda m: lines.append(f"[rank 1] {m}"))
    x = clips(5)[0]
    d = [1, 1] + [0] * 28
    cli.report_jobs(run, [(7, 3, 0.5, x, x, [1000, 2000], d)], more=[{"policy_lpips": np.zeros(30)}])
    head = "[rank 1] video 7 q3 thr 0.50: "
    assert lines == [head + "d=[1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0] BPP 0.00610 PSNR 30.000",
                     head + "FVD: 3.250000",
                     head + "SSIM: 0.90000",
                     head + "LPIPS(vgg): 0.12500",
                     head + "FID: 12.500000 precision: 0.50000 recall: 0.25000"]
    assert os.path.isfile(tmp_path / "output_7" / "city_output_npy_idx7_q3_thr0.50.npy")
    (bpp, v), = run.collector.jobs[7]
    assert bpp == 3000 / 128 / 128 / 30 and set(v) == set(VALUES) | {"policy_lpips"}
    assert R.sender_lines({"psnr": [30.0] * 30}, d, bpp) == [lines[0][len(head):]]          # no opt-in flag: the one line


def test_receiver_lines():
    job = ("job_v0_q3_thr0.50.evc", 30, 4, 12345, "DDPM", 2)
    assert R.receiver_lines(*job, VALUES, "vgg", True) == [
        "job_v0_q3_thr0.50.evc: 30 frames, 4 key frames, 12345 bits, DDPM-2 PSNR 30.000 SSIM 0.90000 LPIPS(vgg) 0.12500, frames: match",
        "job_v0_q3_thr0.50.evc: FID: 12.500000 precision: 0.50000 recall: 0.25000"]
    assert R.receiver_lines(*job, {"psnr": [30.0] * 30}, None, False) == [
        "job_v0_q3_thr0.50.evc: 30 frames, 4 key frames, 12345 bits, DDPM-2 PSNR 30.000, frames: MISMATCH"]
    assert R.receiver_lines(*job, {}) == ["job_v0_q3_thr0.50.evc: 30 frames, 4 key frames, 12345 bits, DDPM-2"]


def test_stitcher_line():
    v = {"psnr": [30.0] * 30, "ssim": np.full(30, 0.9)}
    assert R.stitcher_line("stitched_c0_q3_thr0.50", 200, 136, 6, v, 1000, 30) == \
        "stitched_c0_q3_thr0.50: 200x136, 6 tiles PSNR 30.000 SSIM 0.90000, 1000 bits = 0.0012 bpp (tiles overlap: coded twice)"
    assert R.stitcher_line("stitched_c0_q3_thr0.50", 200, 136, 6, {"psnr": [30.0] * 30}) == "stitched_c0_q3_thr0.50: 200x136, 6 tiles PSNR 30.000"
    assert R.stitcher_line("stitched_c0_q3_thr0.50", 200, 136, 6, {}) == "stitched_c0_q3_thr0.50: 200x136, 6 tiles"
