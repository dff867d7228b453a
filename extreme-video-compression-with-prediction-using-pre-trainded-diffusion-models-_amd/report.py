"""Per-job metric reporting of city_sender.py, city_receiver.py and city_stitch.py: the flags, the check of their weight files
before any GPU work, the metric networks, the measurement of a decoded clip against its original, the printed lines and the
``.npy`` files the reference's plotting code reads (function.py:148-230).

``Measurer`` runs the metrics a run asked for -- PSNR always; SSIM (ssim.py), MS-SSIM (msssim.py), the benchmark's LPIPS
(lpips.py), FID with precision / recall (fid.py), FVD (fvd.py) and the YUV round-trip metrics (video_io.py) on request -- and returns one job's
values as a dict keyed by the names of ``METRICS``.  ``Collector`` keeps ``(bpp, values)`` per video in report order and writes
the files ``METRICS`` describes.  Only numpy is imported here: everything that needs the device is reached through
``Measurer.backend``, so host tests drive both with stubs.
"""
import os
import sys

import numpy as np

# name in a job's values, file stem, kind, higher is better.  "frames": (jobs, n) per-frame values saved as <stem>_frames_<v>.npy
# and the RD envelope [bpp; per-job mean] as <stem>_<v>.npy; "values": one number per job, <stem>_values_<v>.npy and the
# envelope <stem>_<v>.npy; "raw": <stem>_values_<v>.npy alone.  A file is written when the video's jobs carry the name.
METRICS = (
    ("psnr", "psnr", "frames", True),                # reference names (function.py:148-230)
    ("psnr_yuv", "psnr_yuv", "frames", True),        # --yuv-metrics: the codec benchmark's PSNR (bench_uvg.py:487,508-509)
    ("ssim", "ssim", "frames", True),                # --ssim
    ("ssim_yuv", "ssim_yuv", "frames", True),        # --ssim with --yuv-metrics
    ("ms_ssim", "ms_ssim", "frames", True),          # --ms-ssim
    ("ms_ssim_yuv", "ms_ssim_yuv", "frames", True),  # --ms-ssim with --yuv-metrics
    ("lpips", "lpips_{net}", "frames", False),       # --lpips NET:...
    ("fid", "fid", "values", False),                 # --fid
    ("pr", "pr", "raw", None),                       # --fid: (precision, recall)
    ("fvd", "fvd", "values", False),                 # I3D weights present
    ("policy_lpips", "lpips", "frames", False),      # --policy lpips: the rule's own distances (city_sender.py:570-571)
)

FID_HELP = ("pytorch-fid's pt_inception-2015-12-05-6726825d.pth (never fetched): also report each job's FID and k-NN "
            "precision / recall (k = 3) of the decoded clip's 30 frames against the original's, on the HIP Inception-v3 "
            "(evaluation/fid_PR.py, pr.py; fid.py, DESIGN.md section 8f); prints one 'FID: <v> precision: <p> recall: "
            "<r>' line per job and saves fid_<idx>.npy (RD envelope, lower is better), fid_values_<idx>.npy (jobs,) and "
            "pr_values_<idx>.npy (jobs, 2)")


MS_SSIM_HELP = ("also report each job's MS-SSIM against the original clip (pytorch_msssim.ms_ssim as CompressAI and ELIC evaluate "
                "it: 11-tap Gaussian window, five levels with the standard weights, float64; msssim.py, DESIGN.md section 8g), the "
                "mean over the frames and its -10 log10(1 - v) in dB.  The frames' shorter side must be > 160 (whole frames: "
                "--yuv-fit joint, or city_stitch.py --ms-ssim); a reported value only")


def add_metric_flags(p, ssim_help, lpips_help, ms_ssim_help=MS_SSIM_HELP):
    """--ssim / --ms-ssim / --lpips / --fid / --fid-dims of city_sender.py and city_receiver.py."""
    p.add_argument("--ssim", action="store_true", help=ssim_help)
    p.add_argument("--ms-ssim", action="store_true", help=ms_ssim_help)
    p.add_argument("--lpips", type=str, default=None, metavar="NET:BACKBONE.pth,LIN.pth", help=lpips_help)
    p.add_argument("--fid", type=str, default=None, metavar="WEIGHTS.pth", help=FID_HELP)
    p.add_argument("--fid-dims", type=int, choices=[64, 192, 768, 2048], default=2048,
                   help="--fid: the Inception block whose features are compared (64, 192, 768: a map's spatial mean; default 2048)")


def check_metric_flags(args):
    """The weight files of ``--lpips`` and ``--fid`` must exist; said before any GPU work."""
    if args.lpips:
        from .lpips import parse_spec
        parse_spec(args.lpips)           # FileNotFoundError names the missing file
    if args.fid and not os.path.isfile(args.fid):
        sys.exit(f"--fid {args.fid}: no such file")


def check_ms_ssim_size(args, H, W):
    """``--ms-ssim`` on frames too small for five levels ends the run, before anything is generated."""
    if getattr(args, "ms_ssim", False):
        from .msssim import size_message
        if size_message(H, W):
            sys.exit(size_message(H, W))


def load_networks(args, device, fvd_path=None):
    """The metric networks this run asked for, on ``device`` -> the keyword arguments of ``Measurer`` that hold them."""
    nets = {}
    if fvd_path:
        from .fvd import I3d
        nets["i3d"] = I3d.from_file(fvd_path, device=device)
    if args.lpips:
        from .lpips import Lpips
        nets["lpips"] = Lpips.from_spec(args.lpips, device=device)
    if args.fid:
        from .fid import InceptionV3
        nets["inception"] = InceptionV3.from_file(args.fid, device=device, max_images=30)
    return nets


def cal_psnr(a, b, maxvalue=1.0):
    """city_sender.py:257-260 (float64)."""
    mse = np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2)
    return 10 * np.log10((maxvalue ** 2) / mse)


class HipBackend:
    """The metric modules' functions ``Measurer`` calls, imported when first used."""

    def __getattr__(self, name):
        from . import fid, fvd, msssim, ssim, video_io
        self.__dict__.update(ssim_frames=ssim.ssim_frames, inception_features=fid.features, fid_and_pr=fid.fid_and_pr,
                             frechet_distance=fvd.frechet_distance, yuv_metric_clips=video_io.yuv_metric_clips,
                             psnr_yuv=video_io.psnr_yuv, ssim_yuv=video_io.ssim_yuv, ms_ssim_frames=msssim.ms_ssim_frames,
                             ms_ssim_yuv=video_io.ms_ssim_yuv)
        return object.__getattribute__(self, name)


def _tensor(x):
    """The one place where a clip becomes a contiguous float32 host tensor."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))


class Measurer:
    """Measures decoded clips against their originals.  ssim / ms_ssim / yuv: bool; lpips: ``lpips.Lpips``; inception: ``fid.InceptionV3``
    (features of block ``fid_dims``); i3d: ``fvd.I3d``.  What is None / False is not computed and its name is absent from the
    values.  The originals' Inception and I3D features are computed once per video index and kept."""

    def __init__(self, ssim=False, lpips=None, inception=None, fid_dims=2048, i3d=None, yuv=False, backend=None, ms_ssim=False):
        self.ssim, self.lpips, self.inception, self.fid_dims, self.i3d, self.yuv = ssim, lpips, inception, fid_dims, i3d, yuv
        self.ms_ssim = ms_ssim
        self.net = getattr(lpips, "net", None)             # the --lpips backbone's name, part of its lines and files
        self.backend = backend or HipBackend()
        self.gt_inception, self.gt_i3d = {}, {}

    def measure(self, vid, x, gt):
        """x, gt: numpy (n, 3, H, W) in [0, 1], the decoded clip and the original of video ``vid`` -> the job's values: psnr
        [n], ssim (n,), ms_ssim (n,), lpips (n,) float64, fid, pr (precision, recall), psnr_yuv, ssim_yuv, ms_ssim_yuv.  FVD:
        ``measure_jobs``."""
        B = self.backend
        v = {"psnr": [cal_psnr(x[t], gt[t]) for t in range(len(x))]}
        tx, tg = _tensor(x), _tensor(gt)
        if self.ssim:
            v["ssim"] = B.ssim_frames(tx, tg)
        if self.ms_ssim:
            v["ms_ssim"] = B.ms_ssim_frames(tx, tg)
        if self.lpips is not None:       # the benchmark's LPIPS (calculate_lpips.py:35-58), one value per frame
            v["lpips"] = self.lpips.spatial_mean(tx, tg).double().cpu().numpy()
        if self.inception is not None:   # FID and precision / recall of the clip's frames against the original's (fid_PR.py, pr.py)
            if vid not in self.gt_inception:
                self.gt_inception[vid] = B.inception_features(tg, self.inception, self.fid_dims)
            fv, pv, rv = B.fid_and_pr(self.gt_inception[vid], B.inception_features(tx, self.inception, self.fid_dims), k=3)
            v["fid"], v["pr"] = fv, (pv, rv)
        if self.yuv:
            pair = B.yuv_metric_clips(x, gt)
            v["psnr_yuv"] = B.psnr_yuv(x, gt, clips=pair)
            if self.ssim:
                v["ssim_yuv"] = B.ssim_yuv(x, gt, clips=pair)
            if self.ms_ssim:
                v["ms_ssim_yuv"] = B.ms_ssim_yuv(x, gt, clips=pair)
        return v

    def fvds(self, jobs):
        """FVD of each decoded clip against its video's original, as city_sender.py:575-577 computes it: calculate_fvd of
        x_ge.repeat(2) against x_gt.repeat(2).  jobs: [(vid, x, gt)].  I3D runs once per original video and once per decoded
        clip, all clips of the call batched."""
        import torch
        feats = lambda clips: self.i3d(torch.stack([_tensor(c) for c in clips])).double().cpu().numpy()  # noqa: E731
        new = {vid: gt for vid, _, gt in jobs if vid not in self.gt_i3d}
        if new:
            self.gt_i3d.update(zip(new, feats(new.values())))
        return [self.backend.frechet_distance(np.stack([f, f]), np.stack([self.gt_i3d[vid]] * 2))
                for f, (vid, _, _) in zip(feats([x for _, x, _ in jobs]), jobs)]

    def measure_jobs(self, jobs):
        """jobs: [(vid, x, gt)] -> [values], ``measure`` of each plus ``fvd`` when there are I3D weights."""
        out = [self.measure(*j) for j in jobs]
        if self.i3d is not None and jobs:
            for v, f in zip(out, self.fvds(jobs)):
                v["fvd"] = f
        return out


def fid_text(v):
    return "FID: %f precision: %.5f recall: %.5f" % ((v["fid"],) + tuple(v["pr"]))


def sender_lines(v, d, bpp, net=None):
    """The sender's lines of one job, without their ``[rank R] video V qQ thr T.TT: `` prefix."""
    lines = [f"d={[int(k) for k in d[:30]]} BPP {bpp:.5f} PSNR {np.mean(v['psnr']):.3f}"]
    if "fvd" in v:
        lines.append(f"FVD: {v['fvd']:f}")
    if "ssim" in v:
        lines.append(f"SSIM: {np.mean(v['ssim']):.5f}")
    if "ms_ssim" in v:
        from .msssim import to_db
        lines.append("MS-SSIM: %.5f (%.2f dB)" % (np.mean(v["ms_ssim"]), to_db(np.mean(v["ms_ssim"]))))
    if "lpips" in v:
        lines.append(f"LPIPS({net}): {np.mean(v['lpips']):.5f}")
    if "fid" in v:
        lines.append(fid_text(v))
    return lines


def quality_text(v, net=None):
    """`` PSNR %.3f SSIM %.5f MS-SSIM %.5f LPIPS(<net>) %.5f`` of the receiver's and the stitcher's line: the parts ``v`` holds."""
    s = " PSNR %.3f" % np.mean(v["psnr"]) if "psnr" in v else ""
    s += " SSIM %.5f" % np.mean(v["ssim"]) if "ssim" in v else ""
    s += " MS-SSIM %.5f" % np.mean(v["ms_ssim"]) if "ms_ssim" in v else ""
    return s + (" LPIPS(%s) %.5f" % (net, np.mean(v["lpips"])) if "lpips" in v else "")


def receiver_lines(name, frames, key_frames, bits, sampler, subsample, v, net=None, same=None):
    """The receiver's lines of the job stream ``name``; v: the job's values ({} without the originals); same: ``frames_match``."""
    line = f"{name}: {frames} frames, {key_frames} key frames, {bits} bits, {sampler}-{subsample}" + quality_text(v, net)
    if same is not None:             # format 4: the receiver's frames against the sender's checksum
        line += ", frames: match" if same else ", frames: MISMATCH"
    return [line] + ([f"{name}: {fid_text(v)}"] if "fid" in v else [])


def stitcher_line(name, W, H, tiles, v, bits=None, frames=30):
    line = f"{name}: {W}x{H}, {tiles} tiles" + quality_text(v)
    if bits is not None:
        line += ", %d bits = %.4f bpp (tiles overlap: coded twice)" % (bits, bits / (frames * W * H))
    return line


class Collector:
    """Per video, the ``(bpp, values)`` of its jobs in report order; ``save`` writes the files of ``METRICS`` and ``bpp_<v>.npy``
    under ``output_<v>/``.  net: the ``--lpips`` backbone's name, part of its files' names."""

    def __init__(self, net=None):
        self.net, self.jobs = net, {}

    def add(self, vid, bpp, values):
        self.jobs.setdefault(vid, []).append((bpp, values))

    def save(self, output_path):
        from .policy import rd_envelope
        for vid, jobs in self.jobs.items():
            root = os.path.join(output_path, f"output_{vid}")
            os.makedirs(root, exist_ok=True)
            bpps = [b for b, _ in jobs]
            np.save(os.path.join(root, f"bpp_{vid}.npy"), np.asarray(bpps))
            for name, stem, kind, higher in METRICS:
                if name not in jobs[0][1]:
                    continue
                stem = stem.format(net=self.net)
                vals = np.asarray([v[name] for _, v in jobs])
                np.save(os.path.join(root, f"{stem}_{'frames' if kind == 'frames' else 'values'}_{vid}.npy"), vals)
                if kind != "raw":
                    np.save(os.path.join(root, f"{stem}_{vid}.npy"),
                            rd_envelope(bpps, np.mean(vals, 1) if kind == "frames" else vals, higher))
