"""Command line with the reference's surface (city_sender.py:47-223, 467-617): same flags, same
``configs/mine.yml`` schema and ``--config_mod`` grammar, same checkpoint layouts, same output file names.

    python city_sender.py --data_npy data_npy/city_bonn.npy --output_path out/ --start_idx 0 --end_idx 8

Differences, all additive: ``--q`` selects ELIC quality indexes (the reference hard-codes 4 and 5,
city_sender.py:504), ``--sampler DDPM|DDIM|FPNDM``, ``--policy mask|psnr|lpips`` (+ ``--thresholds``, ``--metric``):
``lpips`` is the reference's rule (``decide_5to5_lpips``, city_sender.py:376-406, thresholds 0.30 ... 0.03 x q in {4, 5}) and
the DEFAULT whenever a perceptual metric is available -- ``--metric`` (weight files of the HIP LPIPS-AlexNet or
``pkg.module:callable``) or LPIPS weight files found where the reference keeps them (``find_lpips_weights``); without one
the explicit fallback ``mask`` (fixed transmit mask) runs and the CLI says so; ``psnr`` is the reference's own
``decide_5to5`` (city_sender.py:353-374); ``--synthetic`` builds seeded stand-ins when checkpoints / data are
absent.  ``--fvd`` (or ``i3d_pretrained_400.pt`` found where the reference keeps it, ``find_i3d_weights``) adds the
reference's third per-job number, the FVD of the decoded clip against the original (city_sender.py:575-589), computed by the
HIP I3D network (fvd.py) and saved as ``fvd_<idx>.npy``.  Under a decision rule ``--bitstream-dir DIR`` writes one replayable
job stream per reported job (container format 3; format 4 with ``--batch-invariant``) for ``city_receiver.py`` and runs the sweep on noise specification N1
(``--noise evc``).  ``--noise-trials K`` draws every generation round K times and keeps, per job, the draw
that serves it best (``policy.choose_trial``); the job stream names it (formats 5 / 6) and its bits are part of the reported BPP.  ``--gpus N`` (or ``torch.distributed.run``) block-shards the video range over N ranks, one GPU each.
``--data_yuv FILE`` reads the clips from a Y4M or raw planar YUV 4:2:0 file instead of ``--data_npy`` (video_io.py: the
reference's benchmark conventions, converted by the HIP kernels of csrc/yuv.hip), ``--yuv-out`` writes each job's decoded clip
as ``.y4m`` and ``--yuv-metrics`` adds the PSNR of the reference's codec benchmark.  ``--yuv-fit crop``
takes a file of any frame size: every frame is centre-cropped and resized as the reference's read_video does with Pillow, bit
for bit, on the GPU (csrc/resample.hip); ``--data_frames 'DIR/output_%04d.png'`` reads RGB image files.
``--yuv-fit tile`` codes the whole frame instead: it is cut into overlapping tiles of the model's size on the GPU (csrc/tile.hip),
every tile's frames are a video of their own (video index = clip * tiles + tile), ``tiles.json`` records the grid and
``city_stitch.py`` (stitch.py) blends the receiver's decoded tiles back into full frames.
``--yuv-fit joint`` codes the whole frame as one video of its own size: the score network is wrapped in ``tiled.TiledScoreNet``,
whose eps at a pixel is the tent-weighted mean over the overlapping tiles that cover it, so the tiles are generated jointly, key
frames are coded once at the frame's size, ``canvas.json`` records size and grid for ``city_receiver.py --yuv-fit joint`` and
nothing is stitched (DESIGN.md section 8c "Joint generation").
``--entropy-estimation`` (a reference flag) reports every key frame's rate as the sum of -log2(likelihood), computed on the GPU
(``ElicModel.estimate``) instead of the length of range-coded strings: same frames, fractional bits.
``--ssim`` adds the reference's SSIM (fvd_utils/calculate_ssim.py; ssim.py, csrc/ssim.hip) of every job:
one more printed line and ``ssim_<idx>.npy`` / ``ssim_frames_<idx>.npy``; a reported value, never a decision rule.
``--ms-ssim`` adds MS-SSIM (pytorch_msssim.ms_ssim; msssim.py, csrc/msssim.hip) the same way, for frames
whose shorter side is > 160 (``--yuv-fit joint``): ``MS-SSIM: <v> (<dB> dB)`` per job, ``ms_ssim_<idx>.npy`` / ``ms_ssim_frames_<idx>.npy``.
``--lpips NET:BACKBONE.pth,LIN.pth`` adds the benchmark's LPIPS (fvd_utils/calculate_lpips.py; lpips.py ``Lpips``, DESIGN.md section
8e) of every job on the alex, vgg or squeeze backbone: one more printed line and ``lpips_<net>_<idx>.npy`` /
``lpips_<net>_frames_<idx>.npy``; ``--lpips-net`` picks the backbone of the ``--policy lpips`` rule (default alex).
``--fid WEIGHTS.pth`` (pytorch-fid's Inception-v3 file, never fetched) adds the FID and the k-NN precision / recall (evaluation/;
fid.py, csrc/inception.hip) of every job's 30 decoded frames against the original clip's: one more printed
line and ``fid_<idx>.npy`` / ``fid_values_<idx>.npy`` / ``pr_values_<idx>.npy``; ``--fid-dims`` picks the Inception block.
Every reported number is measured, printed and saved by report.py (``Measurer``, ``sender_lines``, ``Collector``); ``main`` parses
and refuses, starts the ranks, loads weights and data, and runs ``run_mask_policy`` or ``run_policy_sweep``.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

from .recovery import NumericsError  # noqa: F401  (raised by check_numerics and by the decoder's range recovery)
from . import report as R
from .report import cal_psnr  # noqa: F401  (defined there; importable from here as before)

DEFAULT_PATHS = [f"checkpoints/neural network/{i}.pth.tar" for i in range(6)]


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    # --- the reference's flags (city_sender.py:50-130) ---
    p.add_argument("--config", type=str, default="configs/mine.yml", help="Path to the config file")
    p.add_argument("--seed", type=int, default=1234, help="Random seed")
    p.add_argument("--exp", type=str, default="checkpoints/sender", help="Path for saving running related data.")
    p.add_argument("--ni", default=True, action="store_true", help="No interaction")
    p.add_argument("--video_gen", default=True, action="store_true")
    p.add_argument("-v", "--video_folder", type=str, default="arg_config")
    p.add_argument("--subsample", type=int, default=None, help="override config.sampling.subsample")
    p.add_argument("--ckpt", type=int, default=900000, help="Model checkpoint # to load from")
    p.add_argument("--config_mod", nargs="*", type=str, default="model.ngf=192 model.n_head_channels=192")
    p.add_argument("--data_npy", type=str, default="city_bonn.npy", help="data_npy path, shape = B, T, C, H, W")
    p.add_argument("--output_path", type=str, default="test_out/", help="result output path")
    p.add_argument("-c", "--entropy-coder", choices=["ans"], default="ans", help="entropy coder")
    p.add_argument("--cuda", default=True, help="enable the GPU (always on: there is no CPU path)")
    p.add_argument("--plot", default=True, help="kept for compatibility (RD plots are out of scope)")
    p.add_argument("--entropy-estimation", action="store_true",
                   help="key-frame rate from the likelihoods (sum of -log2, TestModel.inference of the reference) instead of the "
                        "length of range-coded strings: same decoded frames, fractional bits, no host coder on the key-frame path. "
                        "Needs the entropy bottleneck's density parameters in the ELIC checkpoints; writes no strings, so it does "
                        "not combine with --bitstream-dir")
    p.add_argument("-p", "--path", dest="paths", type=str, nargs="+", default=DEFAULT_PATHS, help="ELIC checkpoints")
    p.add_argument("--patch", type=int, default=64, help="padding patch size")
    p.add_argument("--start_idx", type=int, default=0, help="Start video index")
    p.add_argument("--end_idx", type=int, default=0, help="End video index (inclusive, city_sender.py:495)")
    # --- additions ---
    p.add_argument("--q", type=int, nargs="+", default=[4, 5], help="ELIC quality indexes (reference loop: 4 5)")
    p.add_argument("--sampler", default="DDPM", choices=["DDPM", "DDIM", "FPNDM"])
    p.add_argument("--policy", default=None, choices=["mask", "psnr", "lpips"],
                   help="default: lpips -- the reference's rule (decide_5to5_lpips over thresholds 0.30 ... 0.03 x q in {4, 5}, "
                        "city_sender.py:376-406,504-548) -- when --metric is given or LPIPS weight files are found "
                        "(weights/v0.1/alex.pth + an alexnet-owt-*.pth backbone beside it or in the torch hub cache); "
                        "otherwise the explicit fallback `mask` (fixed transmit mask).  The rule that ran is printed.")
    p.add_argument("--thresholds", type=float, nargs="+", default=None,
                   help="psnr policy: dB thresholds; lpips policy: distances (default: the reference's sweep "
                        "0.30, 0.29 ... 0.03, city_sender.py:508)")
    p.add_argument("--metric", type=str, default=None,
                   help="lpips policy: weight files of the HIP LPIPS-AlexNet, 'alexnet-owt-*.pth,alex.pth' (torchvision backbone + "
                        "lpips v0.1 linear layers) or one saved LPIPS state dict; or package.module:callable, fn(pred, gt) -> "
                        "distances for (n,3,H,W) tensors in [0,1]")
    p.add_argument("--policy-batch", type=int, default=32,
                   help="psnr / lpips policy: (video, q, threshold) jobs stacked per score-network launch")
    p.add_argument("--bpp-limit", type=float, default=1.0,
                   help="psnr / lpips policy: a (video, q) sweep stops at the first threshold whose rate reaches this "
                        "many bits per pixel (city_sender.py:563-564)")
    p.add_argument("--gpus", type=int, default=1,
                   help="ranks (one per GPU) to shard the video range over; > 1 outside torchrun starts them itself")
    p.add_argument("--synthetic", action="store_true", help="seeded stand-ins for missing checkpoints / data")
    p.add_argument("--batch", type=int, default=8,
                   help="mask policy: clips decoded together per GPU (the reference runs one clip at a time)")
    p.add_argument("--groups", type=int, default=1, help="concurrent clip groups (HIP streams) inside a batch")
    p.add_argument("--bitstream-dir", type=str, default=None,
                   help="mask policy: write each batch's key-frame strings + mask as an EVC1 container here and "
                        "decode from the bytes read back (container.py); psnr / lpips policy: write one job stream "
                        "job_v<vid>_q<q>_thr<thr>.evc per reported job (container format 3, or 4 with --batch-invariant) for city_receiver.py -- the "
                        "sweep then runs on the replayable noise (--noise evc)")
    p.add_argument("--noise", choices=["torch", "evc"], default=None,
                   help="psnr / lpips policy: torch (default) = one seeded torch.Generator per (job, round, step); evc = noise "
                        "specification N1 drawn by one HIP launch per step (DESIGN.md section 5), the only noise a receiver "
                        "can replay: --bitstream-dir selects it")
    p.add_argument("--batch-invariant", action="store_true",
                   help="psnr / lpips policy: generate in the score network's batch-invariant mode (DESIGN.md section 4): a "
                        "job's frames do not depend on the launches it rides in, so city_receiver.py reproduces them bit for "
                        "bit at any --batch.  Job streams are then container format 4 (plan revision + CRC-32 of the frames). "
                        "Needs the replayable noise (--noise evc, selected when --noise is not given); refuses "
                        "--range-recovery layer")
    p.add_argument("--share-generations", action="store_true",
                   help="psnr / lpips policy: all thresholds of one (video, q) draw from one noise stream (stream id = index "
                        "of the (video, q) pair) and each round generates once per distinct state -- the jobs that hold the "
                        "same last two frames -- instead of once per job (DESIGN.md section 1).  The jobs of one (video, q) "
                        "are then correlated samples; each is still what a receiver decodes from its own stream")
    p.add_argument("--noise-trials", type=int, default=1, metavar="K",
                   help="psnr / lpips policy: draw every generation round K times (noise trial t keys specification N1 with start "
                        "frame + 65536 t; trial 0 is the plain key), keep per job the draw whose accepted prefix is longest "
                        "(ties: the better mean metric, then the lowest trial) and name it in the job stream for ceil(log2 K) "
                        "bits per generated segment, which BPP includes (DESIGN.md sections 1 and 5).  The sender generates K "
                        "times as much; the receiver generates the chosen draw only.  Needs the replayable noise (--noise evc, "
                        "selected when --noise is not given); --policy psnr then sums the squared error on the GPU "
                        "(csrc/metric.hip); job streams are container formats 5 / 6.  1 <= K <= 255, K <= --policy-batch")
    p.add_argument("--range-recovery", choices=["off", "layer"], default=None,
                   help="layer: when a chunk raises an fp16-split range event, demote only the layers that raised it to the "
                        "bf16x6 split and regenerate the chunk with the same noise (default: EVC_RANGE_RECOVERY, else off: "
                        "the run stops with the remedy)")
    p.add_argument("--fvd", type=str, default=None,
                   help="i3d_pretrained_400.pt (InceptionI3d state dict): report each job's FVD against the original clip "
                        "(city_sender.py:575-589) and save fvd_<idx>.npy; default: the file under models/fvd/, "
                        "fvd_utils/models/fvd/ or benchmark/fvd_utils/models/fvd/ when present, else FVD is skipped")
    add_yuv_input_flags(p)
    p.add_argument("--yuv-out", action="store_true",
                   help="write each job's decoded 30 frames as city_idx<idx>_q<q>_thr<thr>.y4m (8-bit 4:2:0, full-range BT.709) "
                        "beside its .npy; the frame rate is the --data_yuv file's, else 30")
    p.add_argument("--yuv-metrics", action="store_true",
                   help="also save psnr_yuv_frames_<idx>.npy and psnr_yuv_<idx>.npy: the PSNR of the reference's codec benchmark "
                        "(bench_uvg.py:487,508-509) -- original and decoded clip both go RGB -> 8-bit 4:2:0 -> RGB (bicubic) -> "
                        "rounded to 8 bits")
    p.add_argument("--lpips-net", choices=["alex", "vgg", "squeeze"], default="alex",
                   help="lpips policy: the backbone whose weight files --metric names (the HIP LPIPS family, lpips.py); frames are "
                        "passed to it as they are, as with the default")
    R.add_metric_flags(
        p,
        ssim_help="also report each job's SSIM against the original clip (fvd_utils/calculate_ssim.py: 11x11 Gaussian window, "
                  "float64, mean over the valid region and the 3 channels) and save ssim_frames_<idx>.npy (jobs, 30) and "
                  "ssim_<idx>.npy; with --yuv-metrics also ssim_yuv_frames_<idx>.npy and ssim_yuv_<idx>.npy, on the two 8-bit "
                  "clips psnr_yuv compares.  A reported value only: no --policy decides by it",
        lpips_help="also report each job's LPIPS against the original clip as the reference's benchmark computes it "
                   "(fvd_utils/calculate_lpips.py:9-58: frames mapped to [-1, 1], spatial map, its mean), under any --policy: "
                   "NET = alex, vgg or squeeze, then torchvision's checkpoint of the backbone and lpips' weights/v0.1/NET.pth, "
                   "or NET:ONE_SAVED_STATE_DICT.pth; prints one LPIPS(NET): line per job and saves lpips_NET_frames_<idx>.npy "
                   "(jobs, 30) and lpips_NET_<idx>.npy (RD envelope, lower is better)")
    return p


YUV_FLAGS = ("data_yuv", "yuv_geometry", "yuv_upsample", "yuv_out", "yuv_metrics", "yuv_fit", "yuv_resize", "data_frames",
             "yuv_tile_overlap")
OPT_IN_FLAGS = YUV_FLAGS + ("ssim", "ms_ssim", "lpips", "lpips_net", "fid", "fid_dims", "noise_trials")       # written to args.yml only when used: a run without them leaves what it always left


def add_yuv_input_flags(p):
    p.add_argument("--data_yuv", type=str, default=None,
                   help="read the clips from a .y4m or raw planar YUV 4:2:0 file (8 or 10 bits) instead of --data_npy: consecutive "
                        "30-frame clips are videos 0, 1, ...; the frame size must be config.data.image_size unless --yuv-fit "
                        "crop or tile is given")
    p.add_argument("--yuv-geometry", type=str, default=None,
                   help="raw .yuv only: WxH[@fps][:bits], e.g. 128x128@30:8 (default: from a _<W>x<H>_<fps>Hz_<bits>bit_ file name)")
    p.add_argument("--yuv-upsample", choices=["bicubic", "bilinear", "nearest"], default="bicubic",
                   help="chroma up-sampling of --data_yuv (torch semantics, align_corners=False; the reference uses bicubic)")
    p.add_argument("--yuv-fit", choices=["refuse", "crop", "tile", "joint"], default="refuse",
                   help="--data_yuv / --data_frames of another frame size than config.data.image_size: refuse (default) ends the "
                        "run; crop fits every frame as the reference's read_video does (bench_uvg.py:577-598) -- the 8-bit RGB "
                        "frame is centre-cropped to a square and resized as PIL.Image.resize does, bit for bit, on the GPU "
                        "(csrc/resample.hip); tile codes the whole frame: it is cut into overlapping image_size x image_size "
                        "tiles on the GPU (csrc/tile.hip) and every tile's 30 frames are a video of their own, video index = "
                        "clip * tiles + tile (--start_idx / --end_idx count these); the sender writes tiles.json, and "
                        "city_stitch.py blends the receiver's decoded tiles back into full frames; joint codes the whole "
                        "frame as ONE video of its own size (video index = clip): the score network's eps at a pixel is the "
                        "tent-weighted mean over the overlapping tiles that cover it (tiled.py), so the tiles are generated "
                        "jointly, key frames are coded once at the frame's size and nothing is stitched; the sender writes "
                        "canvas.json, which city_receiver.py --yuv-fit joint reads.  A file that already has the size is read "
                        "as without the flag")
    p.add_argument("--yuv-tile-overlap", type=int, default=16, metavar="O",
                   help="--yuv-fit tile / joint: samples by which neighbouring tiles overlap at least (even, 0 .. image_size / 2; "
                        "default 16)")
    p.add_argument("--yuv-resize", choices=["lanczos", "bicubic", "bilinear", "hamming", "box"], default="lanczos",
                   help="--yuv-fit crop: Pillow's resampling filter (the reference uses lanczos)")
    p.add_argument("--data_frames", type=str, default=None, metavar="PATTERN",
                   help="'DIR/output_%%04d.png': read the clips from RGB image files instead of --data_npy / --data_yuv (the reference's process_images): "
                        "frames 0, 1, ... are opened with Pillow until one is missing, consecutive 30-frame clips are videos "
                        "0, 1, ...; a frame size other than config.data.image_size takes --yuv-fit")


def _given(argv, flag):
    return any(a == flag or a.startswith(flag + "=") for a in argv)


def parse_args(argv=None, parser=None, receiver=False):
    """``build_parser().parse_args`` plus what argparse cannot say: --data_yuv replaces --data_npy, it does not join it.
    receiver: the arguments are city_receiver.py's, where ``--yuv-fit joint`` needs no source (canvas.json names the size)."""
    p = parser or build_parser()
    argv = sys.argv[1:] if argv is None else list(argv)
    args = p.parse_args(argv)
    if args.data_yuv and _given(argv, "--data_npy"):
        p.error("--data_yuv replaces --data_npy: pass one of them")
    if args.data_frames and (args.data_yuv or _given(argv, "--data_npy")):
        p.error("--data_frames replaces --data_npy and --data_yuv: pass one of the three")
    if args.yuv_geometry and not args.data_yuv:
        p.error("--yuv-geometry describes the --data_yuv file: pass --data_yuv")
    if (args.yuv_fit in ("crop", "tile") or args.yuv_fit == "joint" and not receiver) and not (args.data_yuv or args.data_frames):
        p.error("--yuv-fit fits the frames of --data_yuv or --data_frames: pass one of them")
    if _given(argv, "--yuv-resize") and args.yuv_fit != "crop":
        p.error("--yuv-resize names the filter of --yuv-fit crop: pass --yuv-fit crop")
    if _given(argv, "--yuv-tile-overlap") and args.yuv_fit not in ("tile", "joint"):
        p.error("--yuv-tile-overlap is the overlap of --yuv-fit tile / joint: pass --yuv-fit tile or --yuv-fit joint")
    if args.yuv_fit == "joint":
        from .recovery import recovery_mode
        if recovery_mode(getattr(args, "range_recovery", None)) == "layer":
            p.error("--yuv-fit joint does not combine with --range-recovery layer: recovery is not built for a network that runs "
                    "a frame as several launches per step; set EVC_CONV_ARITH=bf16x6 (no range assumption) instead")
    if args.yuv_fit in ("tile", "joint"):
        size = _config_image_size(args)
        if args.yuv_tile_overlap < 0 or args.yuv_tile_overlap % 2 or (size is not None and 2 * args.yuv_tile_overlap > size):
            p.error(f"--yuv-tile-overlap {args.yuv_tile_overlap} must be even and inside [0, image_size / 2]"
                    + (f" = [0, {size // 2}]" if size is not None else ""))
    return args


def _config_image_size(args):
    """config.data.image_size of the run these arguments describe, or None when the config cannot be read yet (the run says
    so itself, later)."""
    from . import config as C
    try:
        return int(C.load_config(args.config, args.config_mod)[0].data.image_size)
    except Exception:
        return None


def load_yuv_clips(args, image_size, log=print):
    """The clips of ``--data_yuv`` (or ``--data_frames``) as the (B, 30, 3, H, W) uint8 array --data_npy would have held, and the
    file's frame rate (30 for image frames).  Under ``--yuv-fit tile`` the videos are the tiles' (video_io.read_clips); under
    ``--yuv-fit joint`` the frames keep their own size (H, W), whatever the model's."""
    from . import video_io as V
    fit = dict(fit="crop", size=image_size, resize=args.yuv_resize) if args.yuv_fit == "crop" else {}
    if args.yuv_fit == "tile":
        try:
            V.check_overlap(image_size, args.yuv_tile_overlap)
        except ValueError as e:
            sys.exit(f"--yuv-tile-overlap: {e}")
        fit = dict(fit="tile", size=image_size, overlap=args.yuv_tile_overlap)
    joint = args.yuv_fit == "joint"          # the frames are read at their own size: one video per clip (tiled.py)
    if joint:
        try:
            V.check_overlap(image_size, args.yuv_tile_overlap)
        except ValueError as e:
            sys.exit(f"--yuv-tile-overlap: {e}")
    if args.data_frames:
        try:
            data = V.read_frame_clips(args.data_frames, log=log, **fit)
        except V.VideoFormatError as e:
            sys.exit(f"--data_frames: {e}")
        if data.shape[-2:] != (image_size, image_size) and not joint:
            sys.exit(f"--data_frames {args.data_frames}: frames are {data.shape[-1]}x{data.shape[-2]}, the model's "
                     f"config.data.image_size is {image_size}: pass --yuv-fit crop to centre-crop and resize them")
        return data, 30
    try:
        v = V.open_video(args.data_yuv, args.yuv_geometry)
        if (v.height, v.width) != (image_size, image_size) and not fit and not joint:
            sys.exit(f"--data_yuv {args.data_yuv}: frames are {v.width}x{v.height}, the model's config.data.image_size is "
                     f"{image_size}; resizing is not built (the reference resizes with ffmpeg / PIL, which cannot be reproduced "
                     f"here): scale the file to {image_size}x{image_size} first, or pass --yuv-fit crop to centre-crop and "
                     f"resize every frame as the reference's read_video does")
        return V.read_clips(v, upsample=args.yuv_upsample, log=log, **fit), v.fps
    except V.VideoFormatError as e:
        sys.exit(f"--data_yuv: {e}")


def source_frame_size(args):
    """(width, height) of the frames of ``--data_yuv`` / ``--data_frames``, from the file's header or the first image."""
    from . import video_io as V
    if args.data_frames:
        from PIL import Image
        with Image.open(V.frame_path(args.data_frames, 0)) as im:
            return im.size
    v = V.open_video(args.data_yuv, args.yuv_geometry)
    return v.width, v.height


def write_tile_manifests(args, image_size, videos, fps, log=print):
    """``--yuv-fit tile``: tiles.json into --output_path and --bitstream-dir, what city_stitch.py reads.  videos: the number of
    tile-videos ``load_yuv_clips`` returned."""
    from . import video_io as V
    width, height = source_frame_size(args)
    m = V.tile_manifest(width, height, image_size, args.yuv_tile_overlap, 0, 30, fps, args.data_yuv or args.data_frames)
    m["clips"] = videos // (m["ny"] * m["nx"])
    for d in filter(None, (args.output_path, args.bitstream_dir)):
        log(f"tile manifest: {V.write_manifest(d, m)}")
    return m


def joint_canvas(args, image_size, data, fps, rank=0, log=print):
    """``--yuv-fit joint`` on frames of another size than the model's: the grid line, canvas.json into --output_path and
    --bitstream-dir (rank 0) and the manifest; None when the flag is absent or the source already has the model's size (the run
    is then what it is without the flag, and nothing is written)."""
    from . import video_io as V
    if args.yuv_fit != "joint" or tuple(data.shape[-2:]) == (image_size, image_size):
        return None
    height, width = data.shape[-2:]
    m = V.tile_manifest(width, height, image_size, args.yuv_tile_overlap, len(data), 30, fps, args.data_yuv or args.data_frames)
    log(V.canvas_line(width, height, image_size, args.yuv_tile_overlap, m["oy"], m["ox"]))
    if rank == 0:
        for d in filter(None, (args.output_path, args.bitstream_dir)):
            log(f"canvas manifest: {V.write_manifest(d, m, V.CANVAS_NAME)}")
    return m


def resolve_fvd(args, log=print):
    """The I3D weight file of this run's FVD, or None (FVD skipped, said once)."""
    from .fvd import WEIGHT_DIRS, WEIGHT_FILE, find_i3d_weights
    path = args.fvd or find_i3d_weights()
    if path is None:
        log(f"FVD: skipped (no --fvd and no {WEIGHT_FILE} under {', '.join(d + '/' for d in WEIGHT_DIRS)})")
    elif not os.path.isfile(path):
        sys.exit(f"--fvd {path}: no such file")
    else:
        log(f"FVD: I3D weights {path}")
    return path


def find_lpips_weights(roots=(".",)):
    """The LPIPS weight files the reference's rule needs, where the reference keeps / fetches them: the trained linear
    layers ``weights/v0.1/alex.pth`` (shipped in the reference tree, also under models/ and benchmark/) and torchvision's
    AlexNet backbone ``alexnet-owt-*.pth`` (beside it, or in the torch hub cache where ``lpips.LPIPS(net='alex')`` downloads
    it).  -> "backbone.pth,alex.pth" (the ``--metric`` spec of the HIP LPIPS network) or None."""
    import glob as _glob
    for root in roots:
        for sub in ("weights/v0.1", "models/weights/v0.1", "benchmark/weights/v0.1"):
            lin = os.path.join(root, sub, "alex.pth")
            if not os.path.isfile(lin):
                continue
            hub = os.path.join(os.environ.get("TORCH_HOME", os.path.expanduser("~/.cache/torch")), "hub", "checkpoints")
            for d in (os.path.join(root, sub), hub):
                back = sorted(_glob.glob(os.path.join(d, "alexnet-owt-*.pth")))
                if back:
                    return f"{back[0]},{lin}"
    return None


def resolve_policy(args, log=print):
    """The decision rule of this run.  An explicit ``--policy`` wins; otherwise the reference's own rule (LPIPS thresholds
    0.30 ... 0.03, city_sender.py:376-406,504-548) whenever a perceptual metric is available, else ``mask``."""
    if args.policy is None:
        if args.metric is None:
            args.metric = find_lpips_weights()
        args.policy = "lpips" if args.metric else "mask"
        why = (f"metric {args.metric}" if args.metric else
               "no --metric and no LPIPS weight files (weights/v0.1/alex.pth + alexnet-owt-*.pth) found: explicit fallback")
        log(f"decision rule: {args.policy} ({why})")
    else:
        log(f"decision rule: {args.policy} (--policy)")
    return args.policy


def check_numerics(frames, where, note=""):
    """The fp16-split arithmetic clamps nothing (include/evc_hip.h EVC_RANGE_*): an operand beyond fp16's range becomes NaN
    and the sticky range-event word says so.  Never write such frames: stop with the remedy."""
    from . import lib as L
    ev = L.range_events(reset=True)
    finite = bool(torch.isfinite(frames).all()) if torch.is_tensor(frames) else bool(np.isfinite(frames).all())
    if ev or not finite:
        raise NumericsError(
            f"{where}: range-event word {ev:#x}, frames finite: {finite}.  A GroupNorm-ed or moment-bounded operand of the "
            f"score network left fp16's range (or a tensor held NaN / inf) under the default f16x3 arithmetic; rerun with "
            f"EVC_CONV_ARITH=bf16x6 (exact 3-way bf16 split, no range assumption; about half the throughput) or =f32"
            + (f", or with --range-recovery layer (only the layers that raise the event move to bf16x6)" if not note else "")
            + note)


def recovery_note(dec):
    """check_numerics' remark when recovery was asked for but the network has no event sites to demote."""
    if dec.range_recovery == "layer" and not dec.recovers():
        return (f".  Range recovery (--range-recovery layer) is built for the unetmore score networks only, not for "
                f"{type(dec.net).__name__}: this network keeps stopping here")
    return ""


def save_output(gt, xge, q, thr, idx, output_dir):
    """function.py:41-52 (npy always; png when PIL is importable -- the reference uses cv2)."""
    os.makedirs(output_dir, exist_ok=True)
    output = np.concatenate([gt, xge], axis=0)
    np.save(os.path.join(output_dir, "city_output_npy_idx%d_q%d_thr%.2f.npy" % (idx, q, thr)), output)
    try:
        from PIL import Image
        Image.fromarray((output * 255).astype(np.uint8)).save(
            os.path.join(output_dir, "city_idx%d_q%d_thr%.2f.png" % (idx, q, thr)))
    except Exception:
        pass


def diffusion_weights(args, cfg):
    """The score network's state dict: ``checkpoint_<ckpt>.pt`` under --exp, else --synthetic's seeded stand-in, else exit."""
    from . import ckpt, synthetic
    ck = os.path.join(args.exp, f"checkpoint_{cfg.sampling.ckpt_id}.pt")
    if os.path.exists(ck):
        return ckpt.load_diffusion_checkpoint(ck, ema=cfg.model.ema)
    if args.synthetic:
        return synthetic.diffusion_state_dict(cfg, args.seed)
    sys.exit(f"missing {ck} (pass --synthetic for seeded stand-in weights)")


def elic_weights(args, paths, q, missing, density=False):
    """The ELIC state dict of quality q: ``paths[q]``, else --synthetic's stand-in (density: with the density behind the
    bottleneck's tables, which entropy estimation needs; the same weights either way), else exit with ``missing``."""
    from . import ckpt, synthetic
    if q < len(paths) and os.path.exists(paths[q]):
        return ckpt.load_elic_state_dict(paths[q])
    if args.synthetic:
        return synthetic.elic_state_dict_with_density(q) if density else synthetic.elic_state_dict(q)
    sys.exit(missing)


def resolve_noise(args, say):
    """What the resolved policy rules out among --batch-invariant, --share-generations, --bitstream-dir and --noise, and the
    noise the sweep draws (``args.noise``)."""
    if args.batch_invariant:
        from .recovery import recovery_mode
        if args.policy == "mask":
            sys.exit("--batch-invariant applies to the psnr / lpips policy sweep (the mask policy decodes fixed batches)")
        if args.noise == "torch":
            sys.exit("--batch-invariant with --noise torch: nobody can replay torch's generators, so there is no receiver to "
                     "reproduce the frames; drop --noise or pass --noise evc")
        if recovery_mode(args.range_recovery) == "layer":
            sys.exit("--batch-invariant does not combine with --range-recovery layer: one sample's range event would demote "
                     "layers for every sample and for the rest of the run, and a receiver could not know which")
        if args.noise is None:
            say("noise: evc (specification N1) because --batch-invariant frames are meant to be reproduced")
            args.noise = "evc"
    if args.noise_trials != 1:
        if not 1 <= args.noise_trials <= 255:
            sys.exit(f"--noise-trials {args.noise_trials}: 1 .. 255 (a job stream names the trial in one byte)")
        if args.policy == "mask":
            sys.exit("--noise-trials applies to the psnr / lpips policy sweep (the mask policy judges nothing, so there is no "
                     "draw to prefer)")
        if args.noise == "torch":
            sys.exit("--noise-trials with --noise torch: the receiver regenerates the chosen draw from its trial number, which "
                     "only the keyed noise of specification N1 allows; drop --noise or pass --noise evc")
        if args.noise_trials > args.policy_batch:
            sys.exit(f"--noise-trials {args.noise_trials} > --policy-batch {args.policy_batch}: the trials of a state ride in "
                     "one launch, and --policy-batch counts samples")
        if args.noise is None:
            say("noise: evc (specification N1) because --noise-trials names its draws by their key")
            args.noise = "evc"
    if args.share_generations and args.policy == "mask":
        sys.exit("--share-generations applies to the psnr / lpips policy sweep (the mask policy has one job per clip)")
    if args.policy != "mask":
        if args.bitstream_dir and args.noise == "torch":
            sys.exit("--bitstream-dir with --noise torch: a job stream whose frames depend on torch's generators cannot be "
                     "replayed by a receiver; drop --noise or pass --noise evc")
        if args.bitstream_dir and args.noise is None:
            say("noise: evc (specification N1) because --bitstream-dir writes job streams a receiver must replay")
            args.noise = "evc"
        args.noise = args.noise or "torch"


def write_run_files(args, raw):
    """config.yml and args.yml of the run, where the reference writes them."""
    import yaml
    vf = os.path.join(args.exp, "video_samples", args.video_folder)
    os.makedirs(vf, exist_ok=True)
    with open(os.path.join(vf, "config.yml"), "w") as f:
        yaml.dump(raw, f, default_flow_style=False)
    with open(os.path.join(vf, "args.yml"), "w") as f:
        defaults = vars(build_parser().parse_args([]))      # the opt-in flags appear only when used
        yaml.dump({k: v for k, v in vars(args).items() if k not in OPT_IN_FLAGS or v != defaults[k]}, f, default_flow_style=False)


def load_models(args, cfg, rank, world, device):
    """-> (score network, {q: ElicModel}): rank 0 reads (or synthesises) the weights, one RCCL broadcast each."""
    from . import dist as D
    from .elic import ElicModel
    from .scorenet import build_score_network
    sd_d, sd_e = None, {}
    if rank == 0:
        sd_d = diffusion_weights(args, cfg)
        sd_e = {q: elic_weights(args, args.paths, q, f"missing {args.paths[q]} (pass --synthetic)", args.entropy_estimation)
                for q in args.q}
    sd_d = D.broadcast_state_dict(sd_d, 0, device, world)
    net = build_score_network(cfg, sd_d, device=device)     # model.arch: unetmore (default, + spade) | unetmorepseudo3d | unet
    return net, {q: ElicModel(D.broadcast_state_dict(sd_e.get(q), 0, device, world), device=device) for q in args.q}


def load_data(args, cfg, rank, log):
    """-> (clips indexable by video, (30, 3, H, W) uint8 each; frame rate of written .y4m files)."""
    if args.data_yuv or args.data_frames:
        data, fps = load_yuv_clips(args, cfg.data.image_size, log=log)
        if args.end_idx >= len(data):
            sys.exit(f"{'--data_yuv ' + args.data_yuv if args.data_yuv else '--data_frames ' + args.data_frames} holds {len(data)} clip(s) of 30 frames; --end_idx {args.end_idx} is beyond them")
        if args.yuv_fit == "tile" and rank == 0:
            write_tile_manifests(args, cfg.data.image_size, len(data), fps, log=log)
        return data, fps
    if os.path.exists(args.data_npy):
        return np.load(args.data_npy, mmap_mode="r"), 30
    if args.synthetic:
        from . import synthetic
        return synthetic.make_clips(args.end_idx + 1, seed=args.seed), 30
    sys.exit(f"missing {args.data_npy} (pass --synthetic)")


def report_jobs(run, jobs, more=None, trials=None):
    """jobs: [(vid, q, thr, x, gt, bits, d)] that passed ``check_numerics``, x and gt numpy (30, 3, H, W).  They are measured
    together (report.Measurer: one I3D pass for the call's clips); then, job by job, the lines are printed, city_output_npy /
    .png / .y4m written and the values handed to the collector.  more: per job, values measured elsewhere.  trials: per job of
    a --noise-trials sweep, (K, trial bits): the bits join the job's BPP and its first line says so."""
    values = run.measurer.measure_jobs([(vid, x, gt) for vid, _, _, x, gt, _, _ in jobs])
    for i, ((vid, q, thr, x, gt, bits, d), v, extra) in enumerate(zip(jobs, values, more or [{}] * len(jobs))):
        pixels = getattr(run, "pixels", None) or 128 * 128         # --yuv-fit joint: the frame's own H x W
        bpp = (sum(bits) if trials is None else sum(bits) + trials[i][1]) / pixels / 30
        lines = R.sender_lines(v, d, bpp, run.measurer.net)
        if trials is not None:
            lines[0] += f" trials {trials[i][0]} (+{trials[i][1]} bits)"
        for line in lines:
            run.log(f"video {vid} q{q} thr {thr:.2f}: {line}")
        out = os.path.join(run.args.output_path, f"output_{vid}")
        save_output(np.concatenate(list(gt.transpose(0, 2, 3, 1)), axis=1), np.concatenate(list(x.transpose(0, 2, 3, 1)), axis=1),
                    q, thr, vid, out)
        if run.args.yuv_out:
            from . import video_io as V
            V.write_clip(os.path.join(out, "city_idx%d_q%d_thr%.2f.y4m" % (vid, q, thr)), x, run.fps)
        run.collector.add(vid, bpp, {**v, **extra})


def run_mask_policy(run, net, models, cfg, data, vids, device, gen):
    """Every clip has the same transmit mask (2 key frames, then generated): decode ``--batch`` clips per launch through the
    receiver (the path bench.py measures) instead of one clip at a time."""
    from . import keystrings as KS, sampler as S
    from .decoder import ClipDecoder, all_generated_mask
    from .elic import compress_padded, estimate_padded
    args = run.args
    mask = all_generated_mask()
    for q in args.q:
        model = models[q]
        dec = ClipDecoder(net, model, cfg, S.get_sampler(args.sampler), groups=args.groups,
                          range_recovery=args.range_recovery, log=run.log)
        for b0 in range(0, len(vids), max(1, args.batch)):
            chunk = vids[b0:b0 + max(1, args.batch)]
            gt = torch.from_numpy(np.stack([np.asarray(data[v], dtype=np.float32) / 255.0 for v in chunk]))
            keys, shape, est_bits = [], None, []
            key_frames = [] if args.entropy_estimation else None
            for f in (0, 1):                                   # key frames (city_sender.py:521-524), batched
                if args.entropy_estimation:                    # no strings: the decoder is handed the frames themselves, still
                    xh, b, _ = estimate_padded(model, gt[:, f], args.patch)      # padded, as it decodes the strings' frames
                    key_frames.append(xh); est_bits.append(b)
                    continue
                enc = compress_padded(model, gt[:, f], args.patch)     # compress only: ``dec.decode`` below decompresses
                keys.append(enc["strings"]); shape = enc["shape"]
            d_rx, keys_rx, shape_rx = mask, keys, shape
            if args.bitstream_dir:                             # sender -> file -> receiver
                from . import container
                os.makedirs(args.bitstream_dir, exist_ok=True)
                path = os.path.join(args.bitstream_dir, f"clips_{chunk[0]}_{chunk[-1]}_q{q}.evc")
                with open(path, "wb") as fh:
                    fh.write(container.pack(mask, keys, shape, codec=model.codec_tag()))
                with open(path, "rb") as fh:          # refuses a stream coded under another arithmetic
                    d_rx, keys_rx, shape_rx = container.unpack(fh.read(), expect_codec=model.codec_tag())
            crop = dict(size=tuple(gt.shape[-2:])) if getattr(run, "pixels", None) else {}       # --yuv-fit joint: generate at H x W
            frames = dec.decode(d_rx, keys_rx, shape_rx, generator=gen, key_frames=key_frames, **crop)[..., :gt.shape[-2], :gt.shape[-1]]
            check_numerics(frames, f"videos {chunk[0]}..{chunk[-1]} q{q}", recovery_note(dec))
            x_all = frames.cpu().numpy()
            per_key = est_bits if args.entropy_estimation else [[KS.bits(s) for s in KS.split(k)] for k in keys]
            bits = [[b[j] for b in per_key] for j in range(len(chunk))]
            report_jobs(run, [(vid, q, 0.0, x_all[j], gt[j].numpy(), bits[j], mask) for j, vid in enumerate(chunk)])


def run_policy_sweep(run, net, models, cfg, data, vids, device):
    """city_sender.py:495-607 batched (policy.py): every (video, q, threshold) job of this rank advances in lockstep,
    ``--policy-batch`` jobs per score-network launch; key frames coded once per (video, q, frame)."""
    from . import policy as P, sampler as S
    from .decoder import ClipDecoder
    args = run.args
    if args.policy == "lpips":       # city_sender.py:508: np.arange(0.30, 0.02, -0.01) rounded to 2 decimals
        thresholds = args.thresholds or [float("%.2f" % t) for t in np.arange(0.30, 0.02, -0.01)]
    else:
        thresholds = args.thresholds or [0.0]
    metric = P.load_metric(args.policy, args.metric, device, net=args.lpips_net)
    if args.noise_trials > 1 and args.policy == "psnr":
        metric = P.PsnrDeviceMetric()        # K times the candidates: their squared error is summed where they are
    dec = ClipDecoder(net, None, cfg, S.get_sampler(args.sampler), range_recovery=args.range_recovery, log=run.log)
    clips = {vid: torch.from_numpy(np.asarray(data[vid], dtype=np.float32) / 255.0) for vid in vids}
    shared = dict(noise_streams="group", share=True, stats={}) if args.share_generations else {}
    if args.noise_trials > 1:
        shared["trials"] = args.noise_trials
    res = P.run_policy(dec, models, clips, args.q, thresholds, metric, patch=args.patch, max_batch=args.policy_batch,
                       seed=args.seed, device=device, bpp_limit=args.bpp_limit, log=run.log,
                       noise=args.noise, batch_invariant=args.batch_invariant, estimate=args.entropy_estimation, **shared)
    if args.share_generations:
        st = shared["stats"]
        run.log(f"shared generations: {sum(st['states'])} sample-rounds generated for {sum(st['jobs_served'])} "
                f"job-rounds served ({len(st['states'])} rounds)")
    if args.bitstream_dir:       # one replayable stream per reported job (receiver.py decodes them)
        from .receiver import write_job_streams
        written = write_job_streams(args.bitstream_dir, res, models, args.sampler, cfg)
        run.log(f"wrote {len(written)} job stream(s) to {args.bitstream_dir}")
    for vid in vids:
        for q in args.q:
            for r in res[(vid, q)]:
                check_numerics(r["x"], f"video {vid} q{q} thr {r['thr']:.2f}", recovery_note(dec))
            more = None
            if args.policy == "lpips":      # per-frame distances of the decoded clip (city_sender.py:570-571)
                more = [{"policy_lpips": metric.values(torch.from_numpy(r["x"]).to(device), clips[vid].to(device))}
                        for r in res[(vid, q)]]
            trials = [(r["n_trials"], r["trial_bits"]) for r in res[(vid, q)]] if args.noise_trials > 1 else None
            report_jobs(run, [(vid, q, r["thr"], r["x"], clips[vid].numpy(), r["bits"], r["d"]) for r in res[(vid, q)]], more, trials)


def main(argv=None):
    # ---- parse and refuse: everything that can be said before any GPU work ----
    args = parse_args(argv)
    if args.entropy_estimation and args.bitstream_dir:
        sys.exit("--entropy-estimation with --bitstream-dir: an estimated rate comes without coded strings, so there is nothing "
                 "to write into a bitstream; drop one of the two")
    R.check_metric_flags(args)
    from . import dist as D
    if D.needs_self_launch(args.gpus):      # parent: starts the ranks before any HIP call, relays their exit status
        script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "city_sender.py")
        sys.exit(D.self_launch(script, sys.argv[1:] if argv is None else list(argv), args.gpus))
    from types import SimpleNamespace
    from . import config as C, lib as L
    say = lambda m: print(m, flush=True)  # noqa: E731
    resolve_policy(args, log=say)
    resolve_noise(args, say)
    fvd_path = resolve_fvd(args, log=say)
    cfg, raw = C.load_config(args.config, args.config_mod)
    if args.subsample is not None:
        cfg.sampling.subsample = args.subsample
    cfg.sampling.ckpt_id = args.ckpt or cfg.sampling.ckpt_id
    rank, world, device = D.init()
    if args.gpus > 1 and world != args.gpus:
        sys.exit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    L.hip_lib()
    # ---- weights and data ----
    nets = R.load_networks(args, device, fvd_path)
    if args.fid:
        say(f"Inception-v3 weights of --fid: {args.fid} (features: {args.fid_dims})")
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    if rank == 0:
        write_run_files(args, raw)
    net, models = load_models(args, cfg, rank, world, device)
    log = lambda m: print(f"[rank {rank}] {m}", flush=True)  # noqa: E731
    data, yuv_fps = load_data(args, cfg, rank, log)
    R.check_ms_ssim_size(args, *data[0].shape[-2:])      # before anything is generated
    canvas = joint_canvas(args, cfg.data.image_size, data, yuv_fps, rank, log) if args.data_yuv or args.data_frames else None
    if canvas is not None:       # the network takes whole frames: eps blended over the tiles that cover a pixel (tiled.py)
        from .tiled import TiledScoreNet
        try:
            net = TiledScoreNet(net, cfg.data.image_size, args.yuv_tile_overlap, tile_batch=max(1, args.batch))
        except NotImplementedError as e:
            sys.exit(f"--yuv-fit joint: {e}")
    # ---- this rank's videos under one of the two policies ----
    lo, hi = D.shard_range(args.end_idx + 1 - args.start_idx, rank, world)
    vids = list(range(args.start_idx + lo, args.start_idx + hi))
    gen = torch.Generator(device=device).manual_seed(args.seed + rank)
    t_start = time.time()
    run = SimpleNamespace(args=args, log=log, fps=yuv_fps, measurer=R.Measurer(ssim=args.ssim, ms_ssim=args.ms_ssim, fid_dims=args.fid_dims, yuv=args.yuv_metrics, **nets))
    run.collector = R.Collector(net=run.measurer.net)
    run.pixels = canvas["width"] * canvas["height"] if canvas is not None else None       # of a frame, for BPP (None: 128 x 128)
    if args.policy == "mask":
        run_mask_policy(run, net, models, cfg, data, vids, device, gen)
    else:
        run_policy_sweep(run, net, models, cfg, data, vids, device)
    run.collector.save(args.output_path)
    D.barrier()
    if rank == 0:
        print(f"done in {time.time() - t_start:.1f}s")


if __name__ == "__main__":
    main()

