"""On-disk container for one batch of compressed clips.

The reference never serialises anything: key-frame ``strings`` live in RAM and only their bit count is used
(Inference.py:51-67, city_sender.py:556-558).  A receiver needs exactly two things per clip: the transmit mask
``d`` (which frames are key frames) and, per key frame, the ELIC strings ``[y_strings[5][2], z_string]`` plus the
hyper-latent shape.  Layout (little endian):

    magic "EVC1" | u8 format (2) | u8 arith | u16 codec_rev
                 | u16 frames | u16 n_clips | u16 n_key | u16 shape_h | u16 shape_w | u8 d[frames]
    then for every key frame k, clip b:  u32 len(z) | z | for slice 0..4, pass 0..1:  u32 len | bytes

``arith`` / ``codec_rev`` name the arithmetic the ENCODER's entropy-parameter networks ran with
(``ElicModel.codec_tag()``: the convolution arithmetic EVC_ARITH_* and a revision number bumped whenever a kernel's
summation order changes).  A learned codec's range decoder desynchronises if a predicted scale differs by one ulp, so
a receiver whose networks run another arithmetic must REFUSE the stream (``CodecMismatch``) rather than decode garbage.

The payload bytes are exactly the strings the codec produced, so ``8 * payload`` equals the reference's bit count.

Format 3 (``pack_job`` / ``unpack_job``, further down) is the stream of ONE policy job: its program of key / generated
segments and the key of its noise, so that a receiver replays exactly what the sender judged.  Format 4 is format 3 for a
job generated in batch-invariant mode: it adds the generation plan (id, revision) and a CRC-32 of the sender's frames.
Formats 5 and 6 are formats 3 and 4 of a sweep with noise trials: every generated segment names the draw the sender kept.
"""
import struct
import zlib

import numpy as np

from . import keystrings as KS

MAGIC = b"EVC1"
FORMAT = 2
HEADER_BYTES = 4 + 4 + 10          # magic + (format, arith, codec_rev) + 5 x u16
ARITH_NAMES = {0: "f32", 1: "bf16x6", 2: "f16x3"}


class CodecMismatch(ValueError):
    """The stream was produced by entropy-parameter networks running a different arithmetic / kernel revision."""


def pack(d, key_strings, shape, codec=(1, 1)):
    """d: (frames,) 0/1; key_strings: list over key frames of [y_strings[5][2][B], z_strings[B]];
    codec: ``ElicModel.codec_tag()`` of the encoder = (arith, codec_rev)."""
    d = np.asarray(d, dtype=np.uint8).reshape(-1)
    n_key = len(key_strings)
    n_clips = len(key_strings[0][1]) if n_key else 0
    assert int(d.sum()) == n_key, "mask and key-frame count disagree"
    out = [MAGIC, struct.pack("<BBH", FORMAT, int(codec[0]), int(codec[1])),
           struct.pack("<5H", len(d), n_clips, n_key, int(shape[0]), int(shape[1])), d.tobytes()]
    for strings in key_strings:
        for b in range(n_clips):
            KS.write(out, strings, b)
    return b"".join(out)


def read_codec(blob):
    """-> (arith, codec_rev) recorded by the encoder."""
    if blob[:4] != MAGIC or len(blob) < HEADER_BYTES:
        raise ValueError("not an EVC1 container")
    fmt, arith, rev = struct.unpack_from("<BBH", blob, 4)
    if fmt != FORMAT:
        raise ValueError(f"unsupported EVC1 container format {fmt} (this build reads format {FORMAT})")
    return arith, rev


def unpack(blob, expect_codec=None):
    """-> (d, key_strings, shape) in the structure ``ClipDecoder.decode`` takes.  ``expect_codec`` = the receiver's
    ``ElicModel.codec_tag()``: a stream coded under another arithmetic / kernel revision raises ``CodecMismatch``."""
    codec = read_codec(blob)
    if expect_codec is not None and tuple(codec) != tuple(int(v) for v in expect_codec):
        raise CodecMismatch(f"stream was coded with convolution arithmetic {ARITH_NAMES.get(codec[0], codec[0])} rev {codec[1]}, "
                            f"this receiver runs {ARITH_NAMES.get(int(expect_codec[0]), expect_codec[0])} rev {int(expect_codec[1])}: "
                            "the entropy parameters would differ in the last bit and the range decoder would "
                            "desynchronise (set EVC_CONV_ARITH to match the sender)")
    frames, n_clips, n_key, sh, sw = struct.unpack_from("<5H", blob, 8)
    d = np.frombuffer(blob, dtype=np.uint8, count=frames, offset=HEADER_BYTES).astype(np.int64)
    if int(d.sum()) != n_key:
        raise ValueError("corrupt container: mask and key-frame count disagree")
    reader = KS.Reader(blob, HEADER_BYTES + frames, "container")
    key_strings = [KS.read(reader, n_clips) for _ in range(n_key)]
    reader.end()
    return d, key_strings, (sh, sw)


# ---- format 3: one policy job ----------------------------------------------------------------------------------
# A policy job (policy.run_policy: one (video, q, threshold)) has its own mask, and the mask alone does not describe it:
# the sender cuts a run of generated frames where its metric stopped accepting, and every generation round draws the noise
# of its own key.  The job stream therefore carries the job's PROGRAM -- the segment list -- and what names its noise:
#
#     magic "EVC1" | u8 format (3) | u8 arith | u16 codec_rev
#                  | u8 noise spec (1 = N1) | u64 seed | u32 stream id
#                  | u32 video index | u8 q | f32 threshold                      (the job's identity)
#                  | u8 sampler id | u16 subsample steps | u8 denoise            (what the generator needs beyond the checkpoint)
#                  | u16 frames | u16 shape_h | u16 shape_w | u16 n_key | u16 n_segments
#                  | n_segments x (u8 kind: 0 = key, 1 = gen | u8 n)
#     then for every key frame in order:  u32 len(z) | z | for slice 0..4, pass 0..1:  u32 len | bytes
#
# ("key", n): n key frames decoded in one ELIC call; ("gen", n): one generation round from the last two decoded frames of
# which the first n frames are kept, its noise keyed by (seed, stream id, start frame = frames decoded so far, step).
#
# Format 4 = format 3 for a job whose frames were generated in BATCH-INVARIANT mode: a receiver then
# reproduces the sender's frames bit for bit at any batch size, so the stream also names the arithmetic that promise holds
# for and carries a checksum to verify it.  Between the head above (through n_segments) and the segment list it inserts
#
#                  | u8 generation plan id (1 = PLAN_INVARIANT) | u16 plan revision | u32 CRC-32 of the sender's frames
#
# plan revision = ``lib.invariant_plan_revision()`` of the sender's library (bumped whenever a kernel change alters the bits
# of invariant mode); the CRC is ``zlib.crc32`` of the job's decoded frames (frames, 3, H, W) as C-contiguous float32 bytes.
# A receiver refuses an unknown plan id, or another revision (``PlanMismatch``), as it refuses a foreign codec tag.  Jobs
# generated in the default mode keep writing format 3, byte for byte.
#
# Formats 5 and 6 = formats 3 and 4 for a job of a sweep with NOISE TRIALS (policy.run_policy(trials=K), K > 1): the sender drew
# every round K times and kept the draw that served it best, so each generated segment names its trial.  Two changes:
#
#                  | u8 n_trials (K, >= 2)           directly after the head (format 6: after the plan head)
#                  | n_segments x (u8 kind | u8 n | u8 trial)
#
# A ("gen", n) segment of trial t draws the key (seed, stream id, start frame + 65536 t, step): trial 0 is the key of formats
# 3 / 4, and the noise specification id stays 1.  A key segment's trial is 0 and a trial is < n_trials; anything else is a
# corrupt stream.  Jobs of a sweep without trials keep writing formats 3 / 4, byte for byte.
FORMAT_JOB = 3
FORMAT_JOB_INVARIANT = 4
FORMAT_JOB_TRIALS = 5
FORMAT_JOB_INVARIANT_TRIALS = 6
JOB_FORMATS = (FORMAT_JOB, FORMAT_JOB_INVARIANT, FORMAT_JOB_TRIALS, FORMAT_JOB_INVARIANT_TRIALS)
PLAN_INVARIANT = 1
PLANS = {PLAN_INVARIANT: "batch-invariant"}
_PLAN_HEAD = "<BHI"                # plan id, plan revision, frames CRC-32
NOISE_N1 = 1
NOISE_SPECS = {NOISE_N1: "N1"}
SAMPLER_IDS = {"DDPM": 0, "DDIM": 1, "FPNDM": 2}
SAMPLER_NAMES = {v: k for k, v in SAMPLER_IDS.items()}
SEGMENT_KINDS = ("key", "gen")
CHUNK = 5                          # frames of one generation round
_JOB_HEAD = "<BQIIBfBHBHHHHH"      # noise spec ... n_segments


class PlanMismatch(ValueError):
    """The stream's frames were generated under a generation plan (or a revision of it) this build does not reproduce."""


def frames_crc(x):
    """CRC-32 of decoded frames (frames, 3, H, W) as C-contiguous float32 bytes: what a format-4 stream carries."""
    return zlib.crc32(np.ascontiguousarray(np.asarray(x), dtype=np.float32).tobytes()) & 0xFFFFFFFF


def check_segments(segments, frames, n_key=None):
    """The consistency rules of a job's program; raises ValueError.  -> the transmit mask d."""
    d, t = [], 0
    for kind, n in segments:
        if kind not in SEGMENT_KINDS:
            raise ValueError(f"corrupt job stream: unknown segment kind {kind!r}")
        if kind == "key":
            if n < 1:
                raise ValueError("corrupt job stream: empty key segment")
        else:
            if not 1 <= n <= CHUNK:
                raise ValueError(f"corrupt job stream: a generation round keeps 1..{CHUNK} frames, not {n}")
            if t < 2:
                raise ValueError("corrupt job stream: a generated segment needs two decoded frames before it")
        d += [1 if kind == "key" else 0] * n
        t += n
    if t != frames:
        raise ValueError(f"corrupt job stream: segments add up to {t} frames, header says {frames}")
    if n_key is not None and sum(d) != n_key:
        raise ValueError(f"corrupt job stream: segments name {sum(d)} key frames, the stream holds {n_key}")
    return np.asarray(d, dtype=np.int64)


def check_trials(segments, trials, n_trials):
    """The rules of the trial numbers of a format-5 / format-6 program; raises ValueError."""
    if not 2 <= n_trials <= 255:
        raise ValueError(f"corrupt job stream: a stream with noise trials names 2..255 of them, not {n_trials}")
    if len(trials) != len(segments):
        raise ValueError(f"corrupt job stream: {len(trials)} trial numbers for {len(segments)} segments")
    for (kind, _), t in zip(segments, trials):
        if kind == "key" and t != 0:
            raise ValueError(f"corrupt job stream: a key segment with noise trial {t}")
        if not 0 <= t < n_trials:
            raise ValueError(f"corrupt job stream: noise trial {t} of {n_trials}")


def pack_job(segments, key_strings, shape, codec, seed, stream_id, vid, q, thr, sampler, subsample, denoise,
             noise_spec=NOISE_N1, plan=None, crc=None, trials=None, n_trials=1):
    """One policy job -> bytes.  ``plan`` = (plan id, plan revision) and ``crc`` = ``frames_crc`` of the sender's frames make it
    a format-4 stream (a job generated in batch-invariant mode); without them it is format 3.  segments: [("key" | "gen", n)]; key_strings: per key frame, in order, ``[y_strings[5][2][1],
    z_strings[1]]`` (one clip); codec: ``ElicModel.codec_tag()`` of the encoder; sampler: "DDPM" | "DDIM" | "FPNDM".
    ``n_trials`` > 1 with ``trials`` (per segment: 0 for key, the chosen noise trial for gen) makes it format 5 (6 with a plan);
    ``n_trials`` = 1 writes formats 3 / 4 and takes no trial but 0."""
    segments = [(str(k), int(n)) for k, n in segments]
    frames = sum(n for _, n in segments)
    check_segments(segments, frames, len(key_strings))
    if (plan is None) != (crc is None):
        raise ValueError("a format-4 job stream needs both its generation plan and the CRC of the sender's frames")
    if plan is not None and int(plan[0]) not in PLANS:
        raise ValueError(f"unknown generation plan id {plan[0]}")
    n_trials = int(n_trials)
    trials = [0] * len(segments) if trials is None else [int(t) for t in trials]
    if n_trials > 1:
        check_trials(segments, trials, n_trials)
    elif n_trials != 1 or any(trials):
        raise ValueError(f"a job stream without noise trials (n_trials = {n_trials}) names no trial but 0")
    fmt = (FORMAT_JOB, FORMAT_JOB_INVARIANT, FORMAT_JOB_TRIALS, FORMAT_JOB_INVARIANT_TRIALS)[2 * (n_trials > 1) + (plan is not None)]
    out = [MAGIC, struct.pack("<BBH", fmt, int(codec[0]), int(codec[1])),
           struct.pack(_JOB_HEAD, int(noise_spec), int(seed) & (2 ** 64 - 1), int(stream_id), int(vid), int(q), float(thr),
                       SAMPLER_IDS[sampler], int(subsample), int(bool(denoise)), frames, int(shape[0]), int(shape[1]),
                       len(key_strings), len(segments))]
    if plan is not None:
        out.append(struct.pack(_PLAN_HEAD, int(plan[0]), int(plan[1]), int(crc) & 0xFFFFFFFF))
    if n_trials > 1:
        out.append(struct.pack("<B", n_trials))
        out += [struct.pack("<BBB", SEGMENT_KINDS.index(k), n, t) for (k, n), t in zip(segments, trials)]
    else:
        out += [struct.pack("<BB", SEGMENT_KINDS.index(k), n) for k, n in segments]
    for strings in key_strings:
        assert len(strings[1]) == 1, "a job stream holds one clip"
        KS.write(out, strings)
    return b"".join(out)


def unpack_job(blob, expect_codec=None, expect_plan_revision=None):
    """bytes of ``pack_job`` -> dict(format, codec, noise_spec, seed, stream_id, vid, q, thr, sampler, subsample, denoise,
    frames, shape, segments, d, key_strings, plan, crc, trials, n_trials); ``plan`` = (id, revision) and ``crc`` of a format-4 /
    format-6 stream, None for formats 3 / 5; ``segments`` are (kind, n) pairs in every format, ``trials`` the noise trial per
    segment and ``n_trials`` the sender's K (all 0 and 1 for formats 3 / 4).  Raises ValueError for anything but a complete,
    consistent job stream (formats 3 .. 6) of a known noise
    specification and generation plan, ``CodecMismatch`` for a stream coded under another arithmetic / kernel revision,
    ``PlanMismatch`` for a format-4 stream of another plan revision than ``expect_plan_revision`` (the receiver's
    ``lib.invariant_plan_revision()``; None = not checked)."""
    if blob[:4] != MAGIC or len(blob) < 8:
        raise ValueError("not an EVC1 container")
    fmt, arith, rev = struct.unpack_from("<BBH", blob, 4)
    if fmt not in JOB_FORMATS:
        raise ValueError(f"not a job stream: EVC1 container format {fmt} (job streams are formats "
                         f"{', '.join(str(f) for f in JOB_FORMATS)})")
    invariant = fmt in (FORMAT_JOB_INVARIANT, FORMAT_JOB_INVARIANT_TRIALS)
    with_trials = fmt in (FORMAT_JOB_TRIALS, FORMAT_JOB_INVARIANT_TRIALS)
    if expect_codec is not None and (arith, rev) != tuple(int(v) for v in expect_codec):
        raise CodecMismatch(f"stream was coded with convolution arithmetic {ARITH_NAMES.get(arith, arith)} rev {rev}, this "
                            f"receiver runs {ARITH_NAMES.get(int(expect_codec[0]), expect_codec[0])} rev {int(expect_codec[1])}: "
                            "the entropy parameters would differ in the last bit and the range decoder would desynchronise")
    reader = KS.Reader(blob, 8, "job stream")
    spec, seed, stream_id, vid, q, thr, sampler, subsample, denoise, frames, sh, sw, n_key, n_seg = reader.unpack(_JOB_HEAD)
    if spec not in NOISE_SPECS:
        raise ValueError(f"unknown noise specification id {spec} (this build replays {sorted(NOISE_SPECS)} = "
                         f"{', '.join(NOISE_SPECS.values())})")
    if sampler not in SAMPLER_NAMES:
        raise ValueError(f"corrupt job stream: unknown sampler id {sampler}")
    plan = crc = None
    if invariant:
        plan_id, plan_rev, crc = reader.unpack(_PLAN_HEAD)
        if plan_id not in PLANS:
            raise PlanMismatch(f"unknown generation plan id {plan_id} (this build reproduces {sorted(PLANS)} = "
                               f"{', '.join(PLANS.values())})")
        if expect_plan_revision is not None and plan_rev != int(expect_plan_revision):
            raise PlanMismatch(f"stream was generated under revision {plan_rev} of the {PLANS[plan_id]} plan, this receiver's "
                               f"kernels are revision {int(expect_plan_revision)}: its frames would not be the sender's")
        plan = (plan_id, plan_rev)
    n_trials = reader.unpack("<B")[0] if with_trials else 1
    reader.need((3 if with_trials else 2) * n_seg)
    segments, trials = [], []
    for _ in range(n_seg):
        kind, n, trial = reader.unpack("<BBB") if with_trials else reader.unpack("<BB") + (0,)
        if kind >= len(SEGMENT_KINDS):
            raise ValueError(f"corrupt job stream: unknown segment kind {kind}")
        segments.append((SEGMENT_KINDS[kind], n))
        trials.append(trial)
    d = check_segments(segments, frames, n_key)
    if with_trials:
        check_trials(segments, trials, n_trials)
    key_strings = [KS.read(reader) for _ in range(n_key)]
    reader.end()
    return dict(format=fmt, plan=plan, crc=crc, codec=(arith, rev), noise_spec=spec, seed=seed, stream_id=stream_id, vid=vid, q=q, thr=thr,
                sampler=SAMPLER_NAMES[sampler], subsample=subsample, denoise=bool(denoise), frames=frames, shape=(sh, sw),
                segments=segments, d=d, key_strings=key_strings, trials=trials, n_trials=n_trials)


def job_file_name(vid, q, thr):
    return "job_v%d_q%d_thr%.2f.evc" % (vid, q, thr)


def payload_bits(key_strings):
    return KS.bits(key_strings)
