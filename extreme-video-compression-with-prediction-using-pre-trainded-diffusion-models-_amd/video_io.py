"""Video files at the codec's boundary: planar YUV 4:2:0 as Y4M or raw ``.yuv``, 8 or 10 bits.

The conventions are the reference's codec benchmark's (benchmark/transform.py, benchmark/fvd_utils/bench_uvg.py:345-402,
473-509): full-range BT.709, chroma sited at the centre of its 2x2 luma block whatever the file's tag says
(the reference treats every file so), chroma up-sampled x2 with torch's bicubic, PSNR on RGB rounded to 8 bits.

Parsing, slicing and writing bytes are host code (numpy only).  The colour transforms are the two HIP kernels of csrc/yuv.hip:
``read_clips`` / ``write_clip`` / ``yuv_round_trip_u8`` upload a piece of the file as it lies (``FRAME`` markers included) and
convert it with one launch; there is no CPU substitute for them.  ``fit="crop"`` fits frames of another size to the model
(csrc/resample.hip), ``fit="tile"`` cuts them into overlapping tiles of the model's size (csrc/tile.hip; ``tile_grid`` and the
``tiles.json`` manifest are host code).
"""
import os
import re
from fractions import Fraction

import numpy as np

Y4M_MAGIC = b"YUV4MPEG2"
FRAME_MARK = b"FRAME\n"
# chroma tags read as 4:2:0 (all treated as centre-sited) -> bit depth
Y4M_420 = {"420": 8, "420jpeg": 8, "420mpeg2": 8, "420paldv": 8, "420p10": 10}
_NAME_GEOMETRY = re.compile(r"_(\d+)x(\d+)_(\d+(?:\.\d+)?)Hz_(\d+)bit_")
_FLAG_GEOMETRY = re.compile(r"^(\d+)x(\d+)(?:@([0-9.]+(?:/[0-9]+)?))?(?::(\d+))?$")


class VideoFormatError(ValueError):
    pass


def _check_geometry(width, height, bits, what):
    if width < 2 or height < 2 or width % 2 or height % 2:
        raise VideoFormatError(f"{what}: 4:2:0 needs an even width and height of at least 2, got {width}x{height}")
    if bits not in (8, 10):
        raise VideoFormatError(f"{what}: bit depth {bits} is not supported (8 or 10)")


def frame_bytes(width, height, bits=8):
    return width * height * (2 if bits > 8 else 1) * 3 // 2


def as_fps(fps):
    """30, 29.97, "30000/1001", (30000, 1001) or a Fraction -> Fraction."""
    if isinstance(fps, (tuple, list)):
        return Fraction(int(fps[0]), int(fps[1]))
    f = Fraction(str(fps)) if not isinstance(fps, Fraction) else fps
    if f <= 0:
        raise VideoFormatError(f"frame rate must be positive, got {fps}")
    return f


# ---- geometry of raw files ------------------------------------------------------------------------------------------

def parse_geometry(text):
    """``--yuv-geometry WxH[@fps][:bits]`` -> dict(width, height, fps, bits); fps defaults to 30, bits to 8."""
    m = _FLAG_GEOMETRY.match(text.strip())
    if not m:
        raise VideoFormatError(f"geometry {text!r} is not WxH[@fps][:bits] (e.g. 128x128@30:8)")
    g = dict(width=int(m.group(1)), height=int(m.group(2)), fps=as_fps(m.group(3) or 30), bits=int(m.group(4) or 8))
    _check_geometry(g["width"], g["height"], g["bits"], f"geometry {text!r}")
    return g


def geometry_from_name(path):
    """The reference's file naming, ``city_128x128_30Hz_8bit_yuv420p8.yuv`` -> dict(width, height, fps, bits), or None."""
    m = _NAME_GEOMETRY.search(os.path.basename(path))
    if not m:
        return None
    g = dict(width=int(m.group(1)), height=int(m.group(2)), fps=as_fps(m.group(3)), bits=int(m.group(4)))
    _check_geometry(g["width"], g["height"], g["bits"], os.path.basename(path))
    return g


# ---- Y4M headers ----------------------------------------------------------------------------------------------------

def y4m_header(width, height, fps, bits=8):
    """The stream header this project writes (one line, newline included)."""
    _check_geometry(width, height, bits, "Y4M header")
    f = as_fps(fps)
    chroma = "420jpeg" if bits == 8 else "420p10"
    return (f"YUV4MPEG2 W{width} H{height} F{f.numerator}:{f.denominator} Ip A1:1 C{chroma} XCOLORRANGE=FULL\n").encode("ascii")


def parse_y4m_header(line):
    """One header line (bytes, without or with its newline) -> dict(width, height, fps, bits).  Refuses what is not progressive
    4:2:0 of 8 or 10 bits."""
    fields = line.rstrip(b"\n").split(b" ")
    if fields[0] != Y4M_MAGIC:
        raise VideoFormatError("not a Y4M stream: the file does not begin with YUV4MPEG2")
    g = dict(width=None, height=None, fps=Fraction(30), bits=8)
    for f in fields[1:]:
        if not f:
            continue
        tag, val = chr(f[0]), f[1:].decode("ascii", "replace")
        if tag == "W":
            g["width"] = int(val)
        elif tag == "H":
            g["height"] = int(val)
        elif tag == "F":
            num, _, den = val.partition(":")
            if int(num) > 0 and int(den or 1) > 0:        # 0:0 = unknown: keep the default
                g["fps"] = Fraction(int(num), int(den or 1))
        elif tag == "I":
            if val not in ("p", "?"):
                raise VideoFormatError(f"interlaced Y4M (I{val}) is not supported: only progressive frames (Ip)")
        elif tag == "C":
            if val.startswith("422") or val.startswith("444") or val.startswith("411") or val.startswith("mono"):
                raise VideoFormatError(f"Y4M chroma format C{val} is not supported: only 4:2:0 "
                                       f"({', '.join('C' + k for k in Y4M_420)})")
            if val not in Y4M_420:
                raise VideoFormatError(f"Y4M chroma format C{val} is not supported: only {', '.join('C' + k for k in Y4M_420)}")
            g["bits"] = Y4M_420[val]
    if g["width"] is None or g["height"] is None:
        raise VideoFormatError("Y4M header without W or H")
    _check_geometry(g["width"], g["height"], g["bits"], "Y4M header")
    return g


# ---- files ----------------------------------------------------------------------------------------------------------

class YuvFile:
    """A memory-mapped 4:2:0 file: ``n_frames`` frames of ``frame_bytes`` bytes, frame i at byte ``first + i * stride``."""

    def __init__(self, path, data, width, height, fps, bits, first, stride, n_frames, container):
        self.path, self.data, self.width, self.height, self.fps, self.bits = path, data, width, height, fps, bits
        self.first, self.stride, self.n_frames, self.container = first, stride, n_frames, container
        self.frame_bytes = frame_bytes(width, height, bits)

    def frame(self, i):
        """The bytes of frame i (a view of the mapping)."""
        if not 0 <= i < self.n_frames:
            raise IndexError(i)
        at = self.first + i * self.stride
        return self.data[at:at + self.frame_bytes]

    def planes(self, i):
        """Frame i -> (Y (H, W), U (H/2, W/2), V (H/2, W/2)), uint8 or little-endian uint16."""
        return split_planes(self.frame(i), self.width, self.height, self.bits)

    def chunk(self, i0, n):
        """(bytes view, first, stride) of frames i0 .. i0+n-1 as they lie in the file, markers between them included."""
        if n < 1 or i0 < 0 or i0 + n > self.n_frames:
            raise IndexError((i0, n))
        at = self.first + i0 * self.stride
        return self.data[at:at + (n - 1) * self.stride + self.frame_bytes], 0, self.stride


def split_planes(buf, width, height, bits=8):
    dt = np.dtype("<u2") if bits > 8 else np.dtype(np.uint8)
    s = np.frombuffer(bytes(buf), dtype=dt)
    if s.size != width * height * 3 // 2:
        raise VideoFormatError(f"a {width}x{height} 4:2:0 frame has {width * height * 3 // 2} samples, got {s.size}")
    n, c = width * height, width * height // 4
    return (s[:n].reshape(height, width), s[n:n + c].reshape(height // 2, width // 2),
            s[n + c:].reshape(height // 2, width // 2))


def join_planes(y, u, v, bits=8):
    """(Y, U, V) -> the frame's bytes."""
    dt = np.dtype("<u2") if bits > 8 else np.dtype(np.uint8)
    h, w = y.shape
    if u.shape != (h // 2, w // 2) or v.shape != u.shape:
        raise VideoFormatError(f"planes {y.shape}, {u.shape}, {v.shape} are not one 4:2:0 frame")
    return b"".join(np.ascontiguousarray(p, dtype=dt).tobytes() for p in (y, u, v))


def _map(path):
    if os.path.getsize(path) == 0:
        raise VideoFormatError(f"{path}: empty file")
    return np.memmap(path, dtype=np.uint8, mode="r")


def open_y4m(path):
    data = _map(path)
    end = bytes(data[:4096]).find(b"\n")
    if end < 0:
        raise VideoFormatError(f"{path}: no Y4M header line in the first 4096 bytes")
    try:
        g = parse_y4m_header(bytes(data[:end]))
    except VideoFormatError as e:
        raise VideoFormatError(f"{path}: {e}") from None
    fb = frame_bytes(g["width"], g["height"], g["bits"])
    stride = len(FRAME_MARK) + fb
    body = data.size - (end + 1)
    if body % stride:
        raise VideoFormatError(f"{path}: {body} bytes after the header are not a whole number of {g['width']}x{g['height']} "
                               f"{g['bits']}-bit frames ({stride} bytes each with the FRAME marker): truncated file, or FRAME "
                               f"parameters, which are not supported")
    n = body // stride
    for i in range(n):
        at = end + 1 + i * stride
        if bytes(data[at:at + len(FRAME_MARK)]) != FRAME_MARK:
            raise VideoFormatError(f"{path}: no plain FRAME marker at byte {at} (frame {i}); FRAME parameters are not supported")
    return YuvFile(path, data, g["width"], g["height"], g["fps"], g["bits"], end + 1 + len(FRAME_MARK), stride, n, "y4m")


def open_raw(path, geometry=None):
    g = geometry if isinstance(geometry, dict) else (parse_geometry(geometry) if geometry else geometry_from_name(path))
    if g is None:
        raise VideoFormatError(f"{path}: a raw .yuv file carries no geometry; pass --yuv-geometry WxH[@fps][:bits] or name the "
                               f"file ..._<W>x<H>_<fps>Hz_<bits>bit_...")
    data = _map(path)
    fb = frame_bytes(g["width"], g["height"], g["bits"])
    if data.size % fb:
        raise VideoFormatError(f"{path}: {data.size} bytes are not a whole number of {g['width']}x{g['height']} {g['bits']}-bit "
                               f"4:2:0 frames ({fb} bytes each): truncated file or wrong geometry")
    return YuvFile(path, data, g["width"], g["height"], g["fps"], g["bits"], 0, fb, data.size // fb, "raw")


def is_y4m(path):
    return path.lower().endswith(".y4m")


def open_video(path, geometry=None):
    """.y4m -> Y4M (the header wins; ``geometry`` is ignored), anything else -> raw planar 4:2:0."""
    if not os.path.isfile(path):
        raise VideoFormatError(f"{path}: no such file")
    return open_y4m(path) if is_y4m(path) else open_raw(path, geometry)


def write_frames(path, frames, width, height, fps=30, bits=8):
    """frames: iterable of frame byte strings (``join_planes``) or (Y, U, V) triples -> a .y4m file, or raw for any other
    extension.  -> number of frames written."""
    _check_geometry(width, height, bits, path)
    fb, n = frame_bytes(width, height, bits), 0
    with open(path, "wb") as fh:
        if is_y4m(path):
            fh.write(y4m_header(width, height, fps, bits))
        for f in frames:
            b = join_planes(*f, bits=bits) if isinstance(f, (tuple, list)) else bytes(f)
            if len(b) != fb:
                raise VideoFormatError(f"{path}: frame {n} has {len(b)} bytes, a {width}x{height} {bits}-bit frame has {fb}")
            if is_y4m(path):
                fh.write(FRAME_MARK)
            fh.write(b)
            n += 1
    return n


def clip_slices(n_frames, frames=30):
    """-> ([(first frame, frame count)] of the whole clips, frames dropped at the tail)."""
    n = n_frames // frames
    return [(i * frames, frames) for i in range(n)], n_frames - n * frames


# ---- through the GPU ------------------------------------------------------------------------------------------------

def _device(device):
    import torch
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


FIT_GROUP_BYTES = 1 << 28       # device bytes of full-size RGB held at a time while a clip is fitted


def center_box(H, W):
    """The reference's center_crop (bench_uvg.py:577-582) as (r0, c0, h, w): rows H//2 - m//2 .. H//2 + m//2 and columns
    W//2 - m//2 .. W//2 + m//2 with m = min(H, W), so an odd m gives a square of side m - 1."""
    m = min(H, W)
    return H // 2 - m // 2, W // 2 - m // 2, 2 * (m // 2), 2 * (m // 2)


# ---- whole frames as overlapping tiles (DESIGN.md section 8c "Whole frames") ---------------------------------------

def check_overlap(size, overlap):
    if overlap < 0 or overlap % 2 or 2 * overlap > size:
        raise ValueError(f"tile overlap {overlap} must be even and inside [0, {size // 2}] (half the tile size {size})")


def tile_axis(L, S, O):
    """Origins of the S-sample tiles of an axis of L samples that overlap by at least O (0 <= O <= S / 2).  L <= S: one tile at
    0 (its samples past L repeat the last one and take no part in the blend).  L > S: n = ceil((L - O) / (S - O)) tiles at
    (k (L - S)) // (n - 1): the first at 0, the last at L - S, steps of 1 .. S - O, every tile inside the axis."""
    if L < 1 or S < 1 or O < 0 or 2 * O > S:
        raise ValueError(f"tile_axis: length {L}, tile size {S}, overlap {O}: sizes must be positive and 0 <= overlap <= size / 2")
    if L <= S:
        return [0]
    P = S - O
    n = -(-(L - O) // P)
    return [(k * (L - S)) // (n - 1) for k in range(n)]


def tile_grid(H, W, S, O):
    """-> (oy, ox): the row and column origins of the ny x nx tiles of an H x W frame; tile index = ty * nx + tx."""
    return tile_axis(H, S, O), tile_axis(W, S, O)


def tile_line(what, H, W, size, overlap, oy, ox):
    return (f"{what}: {W}x{H} frames as {len(oy)}x{len(ox)} tiles of {size}x{size} overlapping by at least {overlap}, rows at "
            f"{list(oy)}, columns at {list(ox)}; video index = clip * {len(oy) * len(ox)} + row * {len(ox)} + column")


def tile_frames_u8(x, size, oy, ox):
    """x: (N, 3, H, W) uint8 on the device -> (ny * nx, N, 3, size, size): lib.tile_gather_u8."""
    from . import lib as L
    return L.tile_gather_u8(x, size, oy, ox)


MANIFEST_NAME = "tiles.json"
MANIFEST_KEYS = ("version", "width", "height", "size", "overlap", "ny", "nx", "oy", "ox", "clips", "frames", "fps", "source")


def tile_manifest(width, height, size, overlap, clips, frames, fps, source):
    """What ``city_stitch.py`` needs to put the tile-videos of a ``--yuv-fit tile`` run back together."""
    oy, ox = tile_grid(height, width, size, overlap)
    f = as_fps(fps)
    return dict(version=1, width=int(width), height=int(height), size=int(size), overlap=int(overlap), ny=len(oy), nx=len(ox),
                oy=oy, ox=ox, clips=int(clips), frames=int(frames), fps=f"{f.numerator}/{f.denominator}",
                source=os.path.basename(str(source)))


CANVAS_NAME = "canvas.json"        # --yuv-fit joint: the same fields for ONE video per clip, generated jointly over the grid (tiled.py)


def canvas_line(width, height, size, overlap, oy, ox):
    return f"{width}x{height} frames, joint generation over {len(oy)} x {len(ox)} tiles of {size}x{size} (overlap {overlap})"


def read_canvas(directory):
    """canvas.json of a ``--yuv-fit joint`` sender in ``directory`` -> its dict, checked as ``read_manifest`` checks."""
    path = os.path.join(directory, CANVAS_NAME)
    if not os.path.isfile(path):
        raise VideoFormatError(f"{path}: no such file (the sender's --yuv-fit joint writes it beside the job streams)")
    return read_manifest(path)


def write_manifest(directory, manifest, name=MANIFEST_NAME):
    import json
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, name)
    with open(path, "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
        fh.write("\n")
    return path


def read_manifest(path):
    """tiles.json -> its dict, checked: version 1, every key present, the origins those of ``tile_grid``."""
    import json
    try:
        with open(path) as fh:
            m = json.load(fh)
    except (OSError, ValueError) as e:
        raise VideoFormatError(f"{path}: not a tile manifest ({e})") from None
    if not isinstance(m, dict) or m.get("version") != 1:
        raise VideoFormatError(f"{path}: not a version-1 tile manifest")
    missing = [k for k in MANIFEST_KEYS if k not in m]
    if missing:
        raise VideoFormatError(f"{path}: tile manifest without {', '.join(missing)}")
    try:
        oy, ox = tile_grid(m["height"], m["width"], m["size"], m["overlap"])
    except (TypeError, ValueError) as e:
        raise VideoFormatError(f"{path}: {e}") from None
    if list(m["oy"]) != oy or list(m["ox"]) != ox or (m["ny"], m["nx"]) != (len(oy), len(ox)):
        raise VideoFormatError(f"{path}: the origins are not those of a {m['width']}x{m['height']} frame in {m['size']}x{m['size']} "
                               f"tiles overlapping by {m['overlap']}")
    return m


def _check_fit(fit, size, resize, overlap=None):
    from . import lib as L
    if fit not in (None, "crop", "tile"):
        raise ValueError(f"fit must be None, 'crop' or 'tile', got {fit!r}")
    if fit and (size is None or size < 1):
        raise ValueError(f"fit={fit!r} needs the size to fit to")
    if fit == "tile":
        check_overlap(size, 16 if overlap is None else overlap)
    if resize not in L.RESAMPLE_FILTERS:
        raise ValueError(f"resize filter {resize!r} is not one of {', '.join(L.RESAMPLE_FILTERS)}")


def fit_frames_u8(x, size, resize="lanczos"):
    """x: (N, 3, H, W) uint8 on the device -> (N, 3, size, size): the reference's read_video (bench_uvg.py:588-598) -- centre
    crop, then Pillow's 8-bit resize with ``resize`` (lib.resample_u8: bit for bit)."""
    from . import lib as L
    return L.resample_u8(x, size, size, resize, box=center_box(x.shape[2], x.shape[3]))


def fit_line(what, H, W, size, resize):
    r0, c0, h, w = center_box(H, W)
    return f"{what}: {W}x{H} frames, centre crop {w}x{h} at column {c0}, row {r0}, resized to {size}x{size} ({resize}, 8-bit, as Pillow)"


def read_clips(path, frames=30, geometry=None, upsample="bicubic", device=None, log=print, fit=None, size=None, resize="lanczos",
               overlap=16):
    """-> (B, frames, 3, H, W) uint8 RGB, the array ``--data_npy`` would have held: consecutive ``frames``-frame clips of the
    file are videos 0, 1, ...; a trailing partial clip is dropped (one line through ``log``).  Each clip is uploaded as it lies
    in the file and converted by one launch (evc_yuv420_to_rgb, uint8 form).

    ``fit="crop"``: frames of another size than ``size`` x ``size`` are centre-cropped and resized to it on the device
    (``fit_frames_u8``, one more line through ``log``) after the same conversion, a group of frames at a time, and only the
    result comes back: (B, frames, 3, size, size) whatever the source.  A file that already has that size is read as without
    ``fit``.

    ``fit="tile"``: every frame of another size is cut into the ny x nx overlapping ``size`` x ``size`` tiles of ``tile_grid``
    (``overlap`` samples at least; lib.tile_gather_u8 after the same conversion, a group of frames at a time, one more line
    through ``log``) and each tile's frames are a video of their own: (B * ny * nx, frames, 3, size, size), video index =
    clip * (ny * nx) + tile index."""
    import torch
    from . import lib as L
    _check_fit(fit, size, resize, overlap)
    v = path if isinstance(path, YuvFile) else open_video(path, geometry)
    slices, dropped = clip_slices(v.n_frames, frames)
    if dropped:
        log(f"{v.path}: {v.n_frames} frames = {len(slices)} clip(s) of {frames}; the last {dropped} frame(s) are dropped")
    if not slices:
        raise VideoFormatError(f"{v.path}: {v.n_frames} frame(s), fewer than one clip of {frames}")
    dev = _device(device)
    fitted = fit == "crop" and (v.height, v.width) != (size, size)
    tiled = fit == "tile" and (v.height, v.width) != (size, size)
    if fitted:
        log(fit_line(v.path, v.height, v.width, size, resize))
    tiles = 1
    if tiled:
        oy, ox = tile_grid(v.height, v.width, size, overlap)
        tiles = len(oy) * len(ox)
        log(tile_line(v.path, v.height, v.width, size, overlap, oy, ox))
    out = np.empty((len(slices) * tiles, frames, 3) + ((size, size) if fitted or tiled else (v.height, v.width)), dtype=np.uint8)
    group = max(1, FIT_GROUP_BYTES // (3 * v.height * v.width)) if fitted or tiled else frames
    for b, (i0, n) in enumerate(slices):
        piece, first, stride = v.chunk(i0, n)
        buf = torch.from_numpy(np.array(piece)).to(dev)
        for j in range(0, n, group):
            g = min(group, n - j)
            rgb = L.yuv420_to_rgb(buf, g, v.height, v.width, v.bits, upsample, first=first + j * stride, stride=stride, dtype=torch.uint8)
            if tiled:
                out[b * tiles:(b + 1) * tiles, j:j + g] = tile_frames_u8(rgb, size, oy, ox).cpu().numpy()
            else:
                out[b, j:j + g] = (fit_frames_u8(rgb, size, resize) if fitted else rgb).cpu().numpy()
    return out


def frame_path(pattern, i):
    try:
        return pattern % i
    except (TypeError, ValueError):
        raise VideoFormatError(f"{pattern!r} is not a frame pattern with one integer field, e.g. 'DIR/output_%04d.png'") from None


def read_frame_clips(pattern, frames=30, device=None, log=print, fit=None, size=None, resize="lanczos", overlap=16):
    """The reference's own entry (process_images / read_video, bench_uvg.py:588-613): ``pattern % 0``, ``pattern % 1``, ... are
    opened with Pillow until one is missing -> (B, frames, 3, H, W) uint8 as ``read_clips`` gives it.  Every file must be of
    mode RGB and of the first one's size.  ``fit="crop"``: frames of another size than ``size`` x ``size`` are uploaded as
    uint8 and take ``fit_frames_u8``, as in ``read_clips``; ``fit="tile"``: they take ``tile_frames_u8`` and come back as
    tile-videos, as in ``read_clips``."""
    import torch
    try:
        from PIL import Image
    except ImportError:
        raise VideoFormatError("reading image frames needs Pillow (PIL), which is not installed") from None
    _check_fit(fit, size, resize, overlap)
    n_files = 0
    while os.path.isfile(frame_path(pattern, n_files)):
        n_files += 1
    if not n_files:
        raise VideoFormatError(f"{frame_path(pattern, 0)}: no such file")
    slices, dropped = clip_slices(n_files, frames)
    if dropped:
        log(f"{pattern}: {n_files} frames = {len(slices)} clip(s) of {frames}; the last {dropped} frame(s) are dropped")
    if not slices:
        raise VideoFormatError(f"{pattern}: {n_files} frame(s), fewer than one clip of {frames}")

    def load(i):
        with Image.open(frame_path(pattern, i)) as im:
            if im.mode != "RGB":
                raise VideoFormatError(f"{frame_path(pattern, i)}: image mode {im.mode}, only RGB is read")
            return np.asarray(im).transpose(2, 0, 1)

    first = load(0)
    H, W = first.shape[1:]
    fitted = fit == "crop" and (H, W) != (size, size)
    tiled = fit == "tile" and (H, W) != (size, size)
    if fitted:
        log(fit_line(pattern, H, W, size, resize))
    tiles = 1
    if tiled:
        oy, ox = tile_grid(H, W, size, overlap)
        tiles = len(oy) * len(ox)
        log(tile_line(pattern, H, W, size, overlap, oy, ox))
    out = np.empty((len(slices) * tiles, frames, 3) + ((size, size) if fitted or tiled else (H, W)), dtype=np.uint8)
    group = max(1, FIT_GROUP_BYTES // (3 * H * W))
    dev = _device(device) if fitted or tiled else None
    for b, (i0, n) in enumerate(slices):
        for j in range(0, n, group):
            g = min(group, n - j)
            x = np.empty((g, 3, H, W), dtype=np.uint8)
            for t in range(g):
                f = load(i0 + j + t)
                if f.shape != (3, H, W):
                    raise VideoFormatError(f"{frame_path(pattern, i0 + j + t)}: {f.shape[2]}x{f.shape[1]}, the first frame is {W}x{H}")
                x[t] = f
            if tiled:
                out[b * tiles:(b + 1) * tiles, j:j + g] = tile_frames_u8(torch.from_numpy(x).to(dev), size, oy, ox).cpu().numpy()
            else:
                out[b, j:j + g] = fit_frames_u8(torch.from_numpy(x).to(dev), size, resize).cpu().numpy() if fitted else x
    return out


def encode_frames(x, bits=8, marker=b"", device=None):
    """x: (T, 3, H, W) float array or tensor in [0, 1] -> 1-D uint8 device tensor: T planar 4:2:0 frames, each preceded by
    ``marker`` (evc_rgb_to_yuv420 writes the samples in place between the markers).  A NaN / inf pixel raises
    ``NumericsError``: no samples are returned for it."""
    import torch
    from . import lib as L
    from .recovery import NumericsError
    dev = _device(device if device is not None else (x.device if torch.is_tensor(x) and x.is_cuda else None))
    x = (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(dev, torch.float32)
    T, _, H, W = x.shape
    stride = len(marker) + frame_bytes(W, H, bits)
    buf = torch.empty((T, stride), dtype=torch.uint8, device=dev)
    if marker:
        buf[:, :len(marker)] = torch.from_numpy(np.frombuffer(marker, dtype=np.uint8).copy()).to(dev)
    events = torch.zeros(1, dtype=torch.int32, device=dev)
    L.rgb_to_yuv420(x, events, bits, buf=buf.view(-1), first=len(marker), stride=stride)
    word = int(events.item())
    if word & L.RANGE_NONFINITE:
        raise NumericsError(f"RGB -> YUV 4:2:0: the frames hold a NaN or an infinity (range-event word {word:#x}); nothing is "
                            f"written for them")
    return buf.view(-1)


def write_clip(path, x, fps=30, bits=8):
    """x: (T, 3, H, W) float array or tensor in [0, 1] -> ``path`` (.y4m, or raw planar 4:2:0 for any other extension).
    Refuses (``NumericsError``, no file) frames with a NaN / inf."""
    T, _, H, W = x.shape
    _check_geometry(W, H, bits, path)
    body = encode_frames(x, bits, FRAME_MARK if is_y4m(path) else b"").cpu().numpy().tobytes()
    with open(path, "wb") as fh:
        if is_y4m(path):
            fh.write(y4m_header(W, H, fps, bits))
        fh.write(body)
    return path


def yuv_round_trip_u8(x, upsample="bicubic"):
    """x: (T, 3, H, W) float in [0, 1] -> uint8 (T, 3, H, W) numpy: RGB -> 8-bit 4:2:0 -> RGB -> rounded to 8 bits, what the
    reference's codec benchmark compares (bench_uvg.py:479-488)."""
    import torch
    from . import lib as L
    T, _, H, W = x.shape
    return L.yuv420_to_rgb(encode_frames(x, 8), T, H, W, 8, upsample, dtype=torch.uint8).cpu().numpy()


def psnr_u8(a, b):
    """Per-frame PSNR of two uint8 clips (T, ...): 10 log10(255^2 / mse), bench_uvg.py:508-509."""
    d = a.astype(np.float64) - b.astype(np.float64)
    mse = (d * d).reshape(len(a), -1).mean(1)
    with np.errstate(divide="ignore"):
        return 10 * np.log10(255.0 ** 2 / mse)


def yuv_metric_clips(x, gt):
    """The two clips the reference's codec benchmark compares for a decoded clip x against its original gt (both (T, 3, H, W)
    in [0, 1]): (original, decoded), each through ``yuv_round_trip_u8``."""
    return yuv_round_trip_u8(gt), yuv_round_trip_u8(x)


def psnr_yuv(x, gt, clips=None):
    """The PSNR of the reference's codec benchmark for a decoded clip x against its original gt (both (T, 3, H, W) in [0, 1]).
    ``clips``: ``yuv_metric_clips(x, gt)`` when the caller already holds them."""
    return psnr_u8(*(clips if clips is not None else yuv_metric_clips(x, gt)))


def ssim_yuv(x, gt, clips=None):
    """Per-frame SSIM (ssim.py) on the same two 8-bit-rounded RGB clips ``psnr_yuv`` compares, scaled to [0, 1]."""
    from .ssim import ssim_frames
    a, b = clips if clips is not None else yuv_metric_clips(x, gt)
    return ssim_frames(b.astype(np.float32) / np.float32(255.0), a.astype(np.float32) / np.float32(255.0))


def ms_ssim_yuv(x, gt, clips=None):
    """Per-frame MS-SSIM (msssim.py) on the same two 8-bit-rounded RGB clips ``psnr_yuv`` and ``ssim_yuv`` compare."""
    from .msssim import ms_ssim_frames
    a, b = clips if clips is not None else yuv_metric_clips(x, gt)
    return ms_ssim_frames(b.astype(np.float32) / np.float32(255.0), a.astype(np.float32) / np.float32(255.0))
