"""Stitch the decoded tiles of a ``--yuv-fit tile`` run back into whole frames (DESIGN.md section 8c "Whole frames").

    python city_stitch.py --tiles out/tiles.json --decoded rx/ --output_path full/ [--bitstream-dir bits/]
                          [--data_yuv SRC | --data_frames PATTERN] [--yuv-geometry ...] [--yuv-upsample ...] [--ssim] [--ms-ssim] [--fps ...]

``city_sender.py --data_yuv SRC --yuv-fit tile`` codes every overlapping tile of the source as a video of its own (video index =
clip * tiles + tile) and writes the grid as ``tiles.json``; ``city_receiver.py`` decodes the job streams into
``decoded_v<vid>_q<q>_thr<thr>.npy``.  This entry groups those files by (clip, q, threshold), blends every complete group on
the GPU (``lib.tile_blend``: tent weights, fixed order, no atomics) and writes ``stitched_c<clip>_q<q>_thr<thr>.npy`` (float32
(30, 3, H, W)) and, for an even width and height, ``.y4m``.  With the source given it adds the PSNR (and ``--ssim``, ``--ms-ssim``) of the
whole frames, with ``--bitstream-dir`` the rate: the bits of the group's job streams over frames x W x H -- the overlaps are
coded twice and counted twice.  The reference has no counterpart: it only ever sees frames of the model's size.
"""
import argparse
import glob
import os
import re
import sys

import numpy as np

DECODED_NAME = re.compile(r"^decoded_v(\d+)_q(\d+)_thr(-?\d+\.\d\d)\.npy$")


def parse_decoded_name(name):
    """``decoded_v<vid>_q<q>_thr<thr>.npy`` (the receiver's name, base name or path) -> (vid, q, thr text), or None."""
    m = DECODED_NAME.match(os.path.basename(name))
    return (int(m.group(1)), int(m.group(2)), m.group(3)) if m else None


def group_decoded(names, tiles):
    """names: file names -> {(clip, q, thr text): {tile index: name}} with clip = vid // tiles, tile index = vid % tiles; names
    that are not the receiver's are left out."""
    groups = {}
    for n in sorted(names):
        key = parse_decoded_name(n)
        if key is None:
            continue
        vid, q, thr = key
        groups.setdefault((vid // tiles, q, thr), {})[vid % tiles] = n
    return groups


def missing_videos(clip, found, tiles):
    """The video indexes of clip ``clip`` that ``found`` (tile indexes) lacks."""
    return [clip * tiles + t for t in range(tiles) if t not in found]


def stitched_name(clip, q, thr):
    return f"stitched_c{clip}_q{q}_thr{thr}"


def missing_line(clip, q, thr, missing, tiles):
    return (f"{stitched_name(clip, q, thr)}: skipped, {len(missing)} of {tiles} tile(s) missing: video index(es) "
            f"{', '.join(str(v) for v in missing)}")


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--tiles", type=str, required=True, help="tiles.json of the sender's --yuv-fit tile run")
    p.add_argument("--decoded", type=str, required=True, help="directory of the receiver's decoded_v<vid>_q<q>_thr<thr>.npy")
    p.add_argument("--output_path", type=str, default="test_out/", help="stitched_c<clip>_q<q>_thr<thr>.npy / .y4m are written here")
    p.add_argument("--bitstream-dir", type=str, default=None,
                   help="directory of the job streams (city_sender.py --bitstream-dir): adds each group's bits and bits per pixel")
    p.add_argument("--data_yuv", type=str, default=None, help="the source file: adds the PSNR of the whole frames")
    p.add_argument("--data_frames", type=str, default=None, metavar="PATTERN", help="the source as RGB image files instead")
    p.add_argument("--yuv-geometry", type=str, default=None, help="raw .yuv only: WxH[@fps][:bits]")
    p.add_argument("--yuv-upsample", choices=["bicubic", "bilinear", "nearest"], default="bicubic",
                   help="chroma up-sampling of --data_yuv (as city_sender.py)")
    p.add_argument("--ssim", action="store_true", help="with the source given, also the SSIM of the whole frames")
    p.add_argument("--ms-ssim", action="store_true",
                   help="with the source given, also the MS-SSIM of the whole frames (msssim.py: five levels, the frames' shorter "
                        "side must be > 160)")
    p.add_argument("--fps", type=str, default=None, help="frame rate of the written .y4m (default: the manifest's)")
    return p


def load_source(args, m, log):
    """The source's whole frames, (clips, frames, 3, H, W) uint8, or None without --data_yuv / --data_frames."""
    from . import video_io as V
    if not (args.data_yuv or args.data_frames):
        return None
    try:
        if args.data_frames:
            data = V.read_frame_clips(args.data_frames, frames=m["frames"], log=log)
        else:
            data = V.read_clips(args.data_yuv, frames=m["frames"], geometry=args.yuv_geometry, upsample=args.yuv_upsample, log=log)
    except V.VideoFormatError as e:
        sys.exit(f"{'--data_frames' if args.data_frames else '--data_yuv'}: {e}")
    if data.shape[-2:] != (m["height"], m["width"]):
        sys.exit(f"{args.data_frames or args.data_yuv}: frames are {data.shape[-1]}x{data.shape[-2]}, the manifest {args.tiles} "
                 f"describes {m['width']}x{m['height']} frames")
    return data


def group_bits(directory, vids, q, thr):
    """Sum of ``container.payload_bits`` over the job streams of the videos ``vids`` at (q, thr text)."""
    from . import container
    total = 0
    for vid in vids:
        path = os.path.join(directory, "job_v%d_q%d_thr%s.evc" % (vid, q, thr))
        with open(path, "rb") as fh:
            total += container.payload_bits(container.unpack_job(fh.read())["key_strings"])
    return total


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.data_yuv and args.data_frames:
        sys.exit("--data_frames replaces --data_yuv: pass one of them")
    import torch
    from . import lib as L, report as R, video_io as V
    from .recovery import NumericsError
    log = lambda s: print(s, flush=True)  # noqa: E731
    try:
        m = V.read_manifest(args.tiles)
    except V.VideoFormatError as e:
        sys.exit(f"--tiles: {e}")
    H, W, S, oy, ox = m["height"], m["width"], m["size"], m["oy"], m["ox"]
    tiles = m["ny"] * m["nx"]
    groups = group_decoded(os.listdir(args.decoded) if os.path.isdir(args.decoded) else [], tiles)
    if not groups:
        sys.exit(f"no decoded_v*_q*_thr*.npy under {args.decoded}")
    R.check_ms_ssim_size(args, H, W)
    L.hip_lib()
    data = load_source(args, m, log)
    measurer = R.Measurer(ssim=args.ssim, ms_ssim=args.ms_ssim)
    os.makedirs(args.output_path, exist_ok=True)
    fps = args.fps or m["fps"]
    done = 0
    for (clip, q, thr), found in sorted(groups.items()):
        name = stitched_name(clip, q, thr)
        missing = missing_videos(clip, found, tiles)
        if missing:
            log(missing_line(clip, q, thr, missing, tiles))
            continue
        x = np.stack([np.load(os.path.join(args.decoded, found[t])) for t in range(tiles)]).astype(np.float32, copy=False)
        if x.shape[2:] != (3, S, S):
            sys.exit(f"{name}: the decoded tiles are {x.shape[1:]}, the manifest's tiles are (frames, 3, {S}, {S})")
        full = L.tile_blend(torch.from_numpy(np.ascontiguousarray(x)).cuda(), H, W, oy, ox).cpu().numpy()
        if not np.isfinite(full).all():
            log(f"{name}: refused, the stitched frames hold a NaN or an infinity (a decoded tile held one); nothing is written")
            continue
        np.save(os.path.join(args.output_path, name + ".npy"), full)
        if W % 2 == 0 and H % 2 == 0:
            try:
                V.write_clip(os.path.join(args.output_path, name + ".y4m"), full, fps)
            except NumericsError as e:
                log(f"{name}: no .y4m: {e}")
        else:
            log(f"{name}: no .y4m: 4:2:0 needs an even width and height, the frames are {W}x{H}")
        values, bits = {}, None
        if data is not None:
            if clip >= len(data):
                sys.exit(f"{name}: the source holds {len(data)} clip(s) of {m['frames']} frames")
            values = measurer.measure(clip, full, (np.asarray(data[clip], dtype=np.float32) / 255.0)[:len(full)])
        if args.bitstream_dir:
            bits = group_bits(args.bitstream_dir, [clip * tiles + t for t in range(tiles)], q, thr)
        log(R.stitcher_line(name, W, H, tiles, values, bits, len(full)))
        done += 1
    log(f"stitched {done} of {len(groups)} group(s) into {args.output_path}")
    if not done:
        sys.exit("nothing was stitched")


if __name__ == "__main__":
    main()
