"""Receiver for policy-coded clips: decodes the job streams a ``city_sender.py --policy psnr|lpips --bitstream-dir DIR`` run
wrote (container format 3, or 4 for jobs generated with ``--batch-invariant``; 5 and 6 are those of a ``--noise-trials K``
sweep, whose generated segments name the one draw the receiver makes; one file per reported (video, q, threshold)
job) with nothing but the model files.  A format-4 job is decoded on the score network's batch-invariant view, whatever
``--batch`` is; the CRC-32 of its frames is compared with the sender's and ``frames: match`` / ``frames: MISMATCH`` printed
per job (any mismatch makes the exit status non-zero).

    python city_receiver.py --bitstream-dir DIR --output_path OUT [--config ... --exp ... --ckpt ... -p ... | --synthetic]

The reference has no receiver (its generator runs inside the sender, city_sender.py:521-550).  What it implies is restated in
``ClipDecoder.decode_jobs``: the stream carries the job's program -- which frames are key frames, where each generation round
was cut -- and the key of its noise (noise specification N1), so the receiver generates from the same
decoded frames, in the same chunks, with the same noise as the sender judged.  The sampler, its step count and the denoise
flag are read from the streams; only the ELIC models the streams name are loaded.  One process, one GPU.  With the original
clips present each job's line carries its PSNR (``--ssim``, ``--ms-ssim``, ``--lpips``: and those) and ``--fid`` adds a line, all from report.py.
``--yuv-fit joint`` decodes the streams of a ``city_sender.py --yuv-fit joint`` run: whole frames of the size and tile grid that
``canvas.json`` in ``--bitstream-dir`` names, generated jointly over the tiles (tiled.py); no source is needed.
"""
import argparse
import glob
import os
import sys

import numpy as np
import torch

from . import container


def write_job_streams(directory, results, models, sampler, cfg):
    """Sender side: one ``job_v<vid>_q<q>_thr<thr>.evc`` per reported job of ``policy.run_policy(..., noise="evc")``.
    results: its return value; sampler: "DDPM" | "DDIM" | "FPNDM"; cfg: the generator's config.  -> {(vid, q, thr): path}."""
    os.makedirs(directory, exist_ok=True)
    paths = {}
    for (vid, q), lst in results.items():
        for r in lst:
            extra = {}
            if r.get("invariant"):       # format 4: the plan the frames were generated under, and their checksum
                from . import lib as L
                extra = dict(plan=(container.PLAN_INVARIANT, L.invariant_plan_revision()), crc=container.frames_crc(r["x"]))
            if r.get("n_trials", 1) > 1:     # formats 5 / 6: the noise trial every generated segment was drawn with
                extra.update(trials=r["trials"], n_trials=r["n_trials"])
            blob = container.pack_job(r["segments"], r["key_strings"], r["shape"], models[q].codec_tag(), r["seed"],
                                      r["stream_id"], vid, q, r["thr"], sampler, getattr(cfg.sampling, "subsample", None) or 0,
                                      cfg.sampling.denoise, **extra)
            path = os.path.join(directory, container.job_file_name(vid, q, r["thr"]))
            with open(path, "wb") as fh:
                fh.write(blob)
            paths[(vid, q, r["thr"])] = path
    return paths


def read_job_streams(directory):
    """-> [(path, bytes)] of every job_*.evc in ``directory``, sorted by name."""
    out = []
    for path in sorted(glob.glob(os.path.join(directory, "job_*.evc"))):
        with open(path, "rb") as fh:
            out.append((path, fh.read()))
    return out


def decode_streams(blobs, net, cfg, model_for, max_batch=32, range_recovery=None, log=print, share=False, stats=None, size=None):
    """blobs: [bytes]; model_for: q -> ElicModel (called once per q the streams name); -> ([job dict], [frames tensor]) in
    the order given.  A stream coded under another entropy arithmetic raises ``container.CodecMismatch``.  ``share`` and
    ``stats`` are ``ClipDecoder.decode_jobs``': decode every distinct key frame and generate every distinct state of a round
    once, and count the samples generated.  ``size`` = (H, W) of a frame when it is not the generator's image size (``net`` is
    then a ``tiled.TiledScoreNet``); a stream made for another size is refused (``ValueError``)."""
    import copy
    from . import lib as L, sampler as S
    from .decoder import ClipDecoder
    rev = L.invariant_plan_revision()
    jobs = [container.unpack_job(b, expect_plan_revision=rev) for b in blobs]
    if recovery_is_layer(range_recovery) and any(j["plan"] is not None for j in jobs):
        raise ValueError("format-4 job streams (batch-invariant generation) do not combine with range recovery "
                         "(--range-recovery layer)")
    models = {q: model_for(q) for q in sorted({j["q"] for j in jobs})}
    jobs = [container.unpack_job(b, expect_codec=models[j["q"]].codec_tag(), expect_plan_revision=rev)
            for b, j in zip(blobs, jobs)]
    frames = [None] * len(jobs)
    decoders = []
    for setting in sorted({(j["sampler"], j["subsample"], j["denoise"]) for j in jobs}):
        c = copy.deepcopy(cfg)
        c.sampling.subsample = setting[1] or None
        c.sampling.denoise = setting[2]
        dec = ClipDecoder(net, None, c, S.get_sampler(setting[0]), range_recovery=range_recovery, log=log)
        decoders.append(dec)
        idx = [i for i, j in enumerate(jobs) if (j["sampler"], j["subsample"], j["denoise"]) == setting]
        for i, f in zip(idx, dec.decode_jobs([jobs[i] for i in idx], max_batch=max_batch, models=models, share=share,
                                                stats=stats, size=size)):
            frames[i] = f
    return jobs, frames, decoders


def recovery_is_layer(range_recovery):
    from .recovery import recovery_mode
    return recovery_mode(range_recovery) == "layer"


def frames_match(job, x):
    """None for a format-3 job (nothing to compare); else whether the decoded frames ``x`` have the sender's CRC-32."""
    if job.get("crc") is None:
        return None
    return container.frames_crc(x) == job["crc"]


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--bitstream-dir", type=str, required=True, help="directory of job_*.evc files (city_sender.py --bitstream-dir)")
    p.add_argument("--output_path", type=str, default="test_out/", help="decoded_v<vid>_q<q>_thr<thr>.npy are written here")
    # the sender's model flags
    p.add_argument("--config", type=str, default="configs/mine.yml", help="Path to the config file")
    p.add_argument("--exp", type=str, default="checkpoints/sender", help="directory of checkpoint_<ckpt>.pt")
    p.add_argument("--ckpt", type=int, default=900000, help="Model checkpoint # to load from")
    p.add_argument("--config_mod", nargs="*", type=str, default="model.ngf=192 model.n_head_channels=192")
    p.add_argument("-p", "--path", dest="paths", type=str, nargs="+", default=None, help="ELIC checkpoints (indexed by q)")
    p.add_argument("--synthetic", action="store_true", help="seeded stand-ins for missing checkpoints / data")
    p.add_argument("--seed", type=int, default=1234, help="seed of the synthetic stand-ins (the sender's --seed)")
    p.add_argument("--range-recovery", choices=["off", "layer"], default=None, help="as city_sender.py")
    p.add_argument("--batch", type=int, default=32, help="jobs stacked per score-network launch")
    p.add_argument("--share-generations", action="store_true",
                   help="decode each distinct key frame and generate each distinct state of a round once, whichever jobs need "
                        "it (streams of a city_sender.py --share-generations sweep share most of their rounds); --batch then "
                        "counts states per launch")
    p.add_argument("--data_npy", type=str, default="city_bonn.npy", help="original clips: when present, per-job PSNR is printed")
    from .cli import add_yuv_input_flags
    add_yuv_input_flags(p)       # --data_yuv / --data_frames: the original clips from a video file or image frames instead (city_sender.py's flags)
    p.add_argument("--yuv", action="store_true",
                   help="also write decoded_v<vid>_q<q>_thr<thr>.y4m (8-bit 4:2:0, full-range BT.709) beside each .npy")
    p.add_argument("--fps", type=str, default="30", help="--yuv: frame rate of the written files (30, 29.97 or 30000/1001)")
    from .report import add_metric_flags
    add_metric_flags(            # with the original clips present: parts of the job's line, and one FID / precision / recall line
        p,
        ssim_help="when the original clips are present, also print each job's SSIM (city_sender.py --ssim) after its PSNR",
        lpips_help="when the original clips are present, also print each job's LPIPS (city_sender.py --lpips: NET = alex, vgg "
                   "or squeeze; frames mapped to [-1, 1], mean of the spatial map) after its PSNR / SSIM")
    return p


def main(argv=None):
    from . import cli, config as C, lib as L, report as R
    args = cli.parse_args(argv, build_parser(), receiver=True)
    R.check_metric_flags(args)
    from .decoder import StreamSizeError
    from .elic import ElicModel
    from .scorenet import build_score_network
    paths = args.paths or cli.DEFAULT_PATHS
    streams = read_job_streams(args.bitstream_dir)
    if not streams:
        sys.exit(f"no job_*.evc under {args.bitstream_dir}")
    cfg, _ = C.load_config(args.config, args.config_mod)
    cfg.sampling.ckpt_id = args.ckpt or cfg.sampling.ckpt_id
    canvas = None
    if args.yuv_fit == "joint":      # whole frames generated jointly over tiles: the sender's canvas.json names size and grid
        from . import video_io as V
        try:
            canvas = V.read_canvas(args.bitstream_dir)
        except V.VideoFormatError as e:
            sys.exit(f"--yuv-fit joint: {e}")
        if canvas["size"] != cfg.data.image_size:
            sys.exit(f"--yuv-fit joint: {os.path.join(args.bitstream_dir, V.CANVAS_NAME)} was written for a model of size "
                     f"{canvas['size']}, config.data.image_size is {cfg.data.image_size}")
    R.check_ms_ssim_size(args, *((canvas["height"], canvas["width"]) if canvas is not None else (cfg.data.image_size,) * 2))
    device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cuda"
    L.hip_lib()
    net = build_score_network(cfg, cli.diffusion_weights(args, cfg), device=device)
    size = None
    if canvas is not None:
        from .tiled import TiledScoreNet
        try:
            net = TiledScoreNet(net, canvas["size"], canvas["overlap"], tile_batch=max(1, args.batch))
        except NotImplementedError as e:
            sys.exit(f"--yuv-fit joint: {e}")
        size = (canvas["height"], canvas["width"])
        print(V.canvas_line(canvas["width"], canvas["height"], canvas["size"], canvas["overlap"], canvas["oy"], canvas["ox"]), flush=True)
    nets = R.load_networks(args, device)
    measurer = R.Measurer(ssim=args.ssim, ms_ssim=args.ms_ssim, fid_dims=args.fid_dims, **nets)

    def model_for(q):
        return ElicModel(cli.elic_weights(args, paths, q, f"missing ELIC checkpoint for q{q} (pass --synthetic)"), device=device)

    log = lambda m: print(m, flush=True)  # noqa: E731
    stats = {}
    try:
        jobs, frames, decoders = decode_streams([b for _, b in streams], net, cfg, model_for, max_batch=max(1, args.batch),
                                                range_recovery=args.range_recovery, log=log, share=args.share_generations,
                                                stats=stats, size=size)
    except StreamSizeError as e:
        sys.exit(f"{e}" + ("" if canvas is not None else " (streams of a --yuv-fit joint sender: pass --yuv-fit joint)"))
    if args.share_generations:
        log(f"shared generations: {stats.get('samples', 0)} sample-rounds generated for {stats.get('job_rounds', 0)} job-rounds "
            f"served, {stats.get('key_frames_decoded', 0)} key frames decoded")
    if args.data_yuv or args.data_frames:
        data, _ = cli.load_yuv_clips(args, cfg.data.image_size, log=log)
    else:
        data = np.load(args.data_npy, mmap_mode="r") if os.path.exists(args.data_npy) else None
    os.makedirs(args.output_path, exist_ok=True)
    note = cli.recovery_note(decoders[0])
    mismatches = 0
    for (path, _), job, x in zip(streams, jobs, frames):
        name = "v%d_q%d_thr%.2f" % (job["vid"], job["q"], job["thr"])
        cli.check_numerics(x, f"{os.path.basename(path)}", note)
        x = x.cpu().numpy()
        np.save(os.path.join(args.output_path, f"decoded_{name}.npy"), x)
        if args.yuv:
            from . import video_io as V
            V.write_clip(os.path.join(args.output_path, f"decoded_{name}.y4m"), x, args.fps)
        values = {}
        if data is not None:
            values = measurer.measure(job["vid"], x, (np.asarray(data[job["vid"]], dtype=np.float32) / 255.0)[:len(x)])
        same = frames_match(job, x)      # format 4: the receiver's frames against the sender's checksum
        mismatches += same is False
        for line in R.receiver_lines(os.path.basename(path), job["frames"], int(job["d"].sum()), container.payload_bits(job["key_strings"]),
                                     job["sampler"], job["subsample"], values, measurer.net, same):
            log(line)
    log(f"decoded {len(jobs)} job stream(s) into {args.output_path}")
    if mismatches:
        sys.exit(f"{mismatches} job(s) decoded to other frames than the sender's (frames: MISMATCH)")


if __name__ == "__main__":
    main()
