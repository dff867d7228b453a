"""Joint generation of whole frames (DESIGN.md section 8c "Joint generation"): a view of a score network that takes canvases of
any size.

The samplers only ever ask the network for eps and update every pixel on its own.  ``TiledScoreNet`` makes the *network*
whole-frame: its eps at a canvas pixel is the tent-weighted mean of the eps predictions of all S x S tiles that cover the pixel
(the weights and the order of ``evc_tile_blend_f32``).  The noisy state, the noise, the conditioning frames and the key frames
then live on the H x W canvas, neighbouring tiles agree on their overlap after every step by construction, and nothing is left
to stitch.

    canvas x (B, 15, H, W), cond (B, 6, H, W)
      -> lib.tile_gather_f32 -> (T * B, C, S, S) tiles, tile-major (tile t of sample b at row t * B + b)
      -> the inner network's forward over the rows, ``tile_batch`` at a time
      -> lib.tile_blend_planes -> eps (B, 15, H, W)

At the model's own size the call goes straight to the inner network: same tensors in, same bits out.  Over the inner network's
batch-invariant view (``invariant_view``) every tile is a sample of the invariant network and gather and blend do not depend on
the batch, so a canvas's bits are independent of B, of ``tile_batch`` and of the launch it rides in.
"""
import torch

from . import lib as L
from . import video_io as V


class TiledScoreNet:
    """inner: a built concat-conditioned ``ScoreNet`` (arch unetmore, no SPADE, no noise_in_cond); S: its image size; overlap:
    samples by which neighbouring tiles overlap at least (``video_io.tile_grid``); tile_batch: tiles per inner launch.
    Everything that is not defined here (schedule buffers, ``prepare_labels``, ``device``, range-event sites ...) is the inner
    network's."""

    TILED = True

    def __init__(self, inner, S, overlap=16, tile_batch=8):
        if getattr(inner, "ARCH", None) != "unetmore" or getattr(inner, "SPADE", False) or getattr(inner, "noise_in_cond", False) \
                or not hasattr(inner, "forward_label"):
            raise NotImplementedError(f"joint generation over tiles is built for the concat-conditioned score network (arch: "
                                      f"unetmore, no SPADE, no noise_in_cond), not for {type(inner).__name__}: a SPADE network "
                                      f"keeps per-tensor conditioning maps and noise_in_cond draws per launch")
        if isinstance(inner, TiledScoreNet):
            raise NotImplementedError("a TiledScoreNet over a TiledScoreNet is not built")
        self.inner, self.S, self.overlap, self.tile_batch = inner, int(S), int(overlap), int(tile_batch)
        if self.S < 1 or self.tile_batch < 1:
            raise ValueError(f"tile size {S} and tile_batch {tile_batch} must be positive")
        V.check_overlap(self.S, self.overlap)
        self._grids = {}              # (H, W) -> (oy, ox)
        self._cond = None             # (the conditioning tensor last gathered, its version, H, W, its tiles)
        self.cond_gathers = 0         # conditioning tensors gathered so far
        self._inv = None

    def __getattr__(self, name):      # only reached for what this class does not define
        if name == "inner":
            raise AttributeError(name)
        return getattr(self.inner, name)

    def grid(self, H, W):
        key = (int(H), int(W))
        if key not in self._grids:
            self._grids[key] = V.tile_grid(key[0], key[1], self.S, self.overlap)
        return self._grids[key]

    def invariant_view(self):
        """The same view over the inner network's batch-invariant view (built once)."""
        if getattr(self.inner, "batch_invariant", False):
            return self
        if self._inv is None:
            self._inv = TiledScoreNet(self.inner.invariant_view(), self.S, self.overlap, self.tile_batch)
        return self._inv

    def _own_size(self, x):
        return tuple(x.shape[-2:]) == (self.S, self.S)

    def _cond_tiles(self, cond, oy, ox):
        """The tiles of a conditioning tensor, gathered once per tensor: the samplers pass the same one on every step."""
        if cond is None:
            return None
        c = self._cond
        if c is not None and c[0] is cond and c[1] == cond._version:
            return c[2]
        src = cond.to(self.inner.device, torch.float32).contiguous()
        tiles = L.tile_gather_f32(src, self.S, oy, ox)
        tiles = tiles.view(-1, *tiles.shape[2:])
        self._cond = (cond, cond._version, tiles)
        self.cond_gathers += 1
        return tiles

    def _tiled(self, x, cond, run):
        """run(x tiles, cond tiles or None, lo, hi) -> eps of rows lo .. hi - 1 of the tile batch."""
        x = x.to(self.inner.device, torch.float32).contiguous()
        B, C, H, W = x.shape
        if cond is not None and tuple(cond.shape[-2:]) != (H, W):
            raise ValueError(f"conditioning frames of {tuple(cond.shape[-2:])} for a canvas of {(H, W)}")
        oy, ox = self.grid(H, W)
        T = len(oy) * len(ox)
        xt = L.tile_gather_f32(x, self.S, oy, ox).view(T * B, C, self.S, self.S)
        ct = self._cond_tiles(cond, oy, ox)
        out = None
        for lo in range(0, T * B, self.tile_batch):
            hi = min(lo + self.tile_batch, T * B)
            eps = run(xt[lo:hi], None if ct is None else ct[lo:hi], lo, hi)
            if out is None:
                out = torch.empty((T * B,) + tuple(eps.shape[1:]), dtype=torch.float32, device=eps.device)
            out[lo:hi] = eps
        return L.tile_blend_planes(out.view(T, B, *out.shape[1:]), H, W, oy, ox)

    @torch.no_grad()
    def forward_label(self, x, label, cond=None):
        if self._own_size(x):
            return self.inner.forward_label(x, label, cond)
        return self._tiled(x, cond, lambda xt, ct, lo, hi: self.inner.forward_label(xt, label, ct))

    @torch.no_grad()
    def __call__(self, x, labels, cond=None, cond_mask=None):
        if self._own_size(x):
            return self.inner(x, labels, cond=cond, cond_mask=cond_mask)
        B = x.shape[0]
        rows = lambda v, lo, hi: None if v is None else [v[i % B] for i in range(lo, hi)]  # noqa: E731  (row t * B + b: sample b)
        labels = labels.detach().cpu().tolist() if torch.is_tensor(labels) else list(labels)
        if cond_mask is not None:
            cond_mask = cond_mask.detach().cpu().tolist() if torch.is_tensor(cond_mask) else list(cond_mask)
        return self._tiled(x, cond, lambda xt, ct, lo, hi: self.inner(xt, rows(labels, lo, hi), cond=ct,
                                                                      cond_mask=rows(cond_mask, lo, hi)))

    forward = __call__

    def eval(self):
        return self
