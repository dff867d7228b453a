"""Time joint generation (tiled.py, DESIGN.md section 8c "Joint generation") on whole frames, default 352x288 and 1920x1080, with
the full-size score network on seeded weights, tiles of 128 overlapping by 16, one canvas (B = 1):

  step    one sampler step's network call on the canvas, split into its parts: the glue (gather of the noisy state + blend of
          eps; the conditioning tiles are gathered once per chunk and timed on their own) against the T-tile forward
          (``tile_batch`` tiles per inner launch), and the whole call
  chunk   one 5-frame chunk (``ClipDecoder.generate``, DDPM with ``--subsample`` steps + denoise) on the canvas in joint mode
          against the same T tiles generated as T independent samples (``--yuv-fit tile``), ``tile_batch`` per launch
  rate    the coded bits of one 352x288 key frame as a whole frame (padded to 64) against the same frame as 9 tiles, with the
          seeded ELIC stand-in weights (real weights will differ)

Host clock around work that ends in a device synchronise, after a warm-up of every shape; median (min - max) of ``--reps``.

    python tools/joint_time.py [--sizes 352x288 1920x1080] [--tile-batch 8] [--subsample 10] [--reps 3] [--q 3] [--small]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import evc_amd  # noqa: E402,F401
from evc_amd import lib as L, sampler as S, synthetic, video_io as V  # noqa: E402
from evc_amd.config import default_config  # noqa: E402
from evc_amd.decoder import ClipDecoder  # noqa: E402
from evc_amd.scorenet import ScoreNet  # noqa: E402
from evc_amd.tiled import TiledScoreNet  # noqa: E402

LABEL = 500


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    out.sort()
    return dict(ms_median=round(out[len(out) // 2], 3), ms_min=round(out[0], 3), ms_max=round(out[-1], 3))


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--sizes", type=str, nargs="+", default=["352x288", "1920x1080"], help="WxH of the frames")
    p.add_argument("--tile-batch", type=int, default=8)
    p.add_argument("--overlap", type=int, default=16)
    p.add_argument("--subsample", type=int, default=10)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--q", type=int, default=3)
    p.add_argument("--small", action="store_true", help="the reduced network (ngf 32) instead of the full-size one: a rehearsal")
    a = p.parse_args()
    L.hip_lib()
    size = 128
    cfg = default_config(32, 32, size, subsample=a.subsample) if a.small else default_config(192, 192, size, subsample=a.subsample)
    inner = ScoreNet(cfg, synthetic.diffusion_state_dict(cfg, 1234))
    net = TiledScoreNet(inner, size, a.overlap, tile_batch=a.tile_batch)
    dec_joint = ClipDecoder(net, None, cfg, S.get_sampler("DDPM"))
    dec_tile = ClipDecoder(inner, None, cfg, S.get_sampler("DDPM"))
    g = torch.Generator(device="cuda").manual_seed(1)
    for wh in a.sizes:
        W, H = (int(v) for v in wh.lower().split("x"))
        oy, ox = V.tile_grid(H, W, size, a.overlap)
        T = len(oy) * len(ox)
        base = dict(width=W, height=H, tiles=f"{len(oy)}x{len(ox)}", tile_batch=a.tile_batch, network="ngf32" if a.small else "ngf192")
        x = torch.randn(1, 15, H, W, device="cuda", generator=g)
        cond = torch.randn(1, 6, H, W, device="cuda", generator=g)
        xt = L.tile_gather_f32(x, size, oy, ox).view(T, 15, size, size)
        ct = L.tile_gather_f32(cond, size, oy, ox).view(T, 6, size, size)
        eps = torch.randn(T, 1, 15, size, size, device="cuda", generator=g)

        def forward():
            for lo in range(0, T, a.tile_batch):
                inner.forward_label(xt[lo:lo + a.tile_batch], LABEL, ct[lo:lo + a.tile_batch])

        parts = {
            "gather_x+blend_eps": lambda: (L.tile_gather_f32(x, size, oy, ox), L.tile_blend_planes(eps, H, W, oy, ox)),
            "gather_cond (once per chunk)": lambda: L.tile_gather_f32(cond, size, oy, ox),
            "tile_forward": forward,
            "whole_call": lambda: net.forward_label(x, LABEL, cond),
        }
        res = {name: timed(fn, max(a.reps, 5) if "gather" in name else a.reps, warm=2) for name, fn in parts.items()}
        for name, r in res.items():
            print(json.dumps(dict(base, what="step", part=name, **r)), flush=True)
        print(json.dumps(dict(base, what="step", glue_share_of_call=round(res["gather_x+blend_eps"]["ms_median"] /
                                                                         res["whole_call"]["ms_median"], 4))), flush=True)
        # one 5-frame chunk: the canvas jointly, and its T tiles as T samples of the plain network
        frames = torch.rand(1, 2, 3, H, W, device="cuda", generator=g)
        tiles = L.tile_gather_f32(frames.view(1, 6, H, W), size, oy, ox).view(T, 2, 3, size, size)

        def tile_mode():
            for lo in range(0, T, a.tile_batch):
                dec_tile.generate(tiles[lo:lo + a.tile_batch].contiguous(), groups=1)

        for name, fn in (("joint", lambda: dec_joint.generate(frames)), ("tile", tile_mode)):
            print(json.dumps(dict(base, what="chunk", mode=name, steps=a.subsample, **timed(fn, a.reps, warm=1))), flush=True)
        L.range_events(reset=True)
    # the rate of one key frame: whole against tiled
    from evc_amd.elic import ElicModel, coded_batch
    model = ElicModel(synthetic.elic_state_dict(a.q))
    H, W = 288, 352
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    blocks = np.repeat(np.repeat(rng.random((3, H // 16, W // 16), dtype=np.float32), 16, axis=1), 16, axis=2)
    frame = 0.5 * blocks + 0.25 * (yy / H)[None] + 0.25 * (xx / W)[None]                     # blocks over two ramps, in [0, 1]
    frame = torch.from_numpy(frame.astype(np.float32))[None].cuda()
    oy, ox = V.tile_grid(H, W, size, a.overlap)
    _, whole, _, shape = coded_batch(model, frame, 64)
    _, tiled, _, _ = coded_batch(model, L.tile_gather_f32(frame.contiguous(), size, oy, ox)[:, 0].contiguous(), 64)
    print(json.dumps(dict(what="rate", width=W, height=H, q=a.q, whole_bits=int(whole[0]), whole_latent_shape=list(shape),
                          tiles=len(tiled), tile_bits=int(sum(tiled)), tile_over_whole=round(sum(tiled) / whole[0], 4))), flush=True)


if __name__ == "__main__":
    main()
