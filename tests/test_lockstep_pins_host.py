"""Pins that hold the sender / receiver core in place: the bytes ``container.pack`` and ``container.pack_job`` write for a fixed
input, the message of every truncation of a small stream, and the sequence of ``compress`` / ``decompress`` / ``generate`` calls
that ``policy.run_policy`` and ``ClipDecoder.decode_jobs`` make on the fakes of tests/test_shared_sweep_host.py.

Every digest and message below was computed on the commit before the key-frame string helpers (``keystrings.py``) and the named
steps of ``decode_jobs`` existed, where this file passes unchanged: a frame that changes its launch, a launch that changes its
order or a byte that moves in a stream changes a digest.  Everything that is hashed is integer arithmetic or single IEEE
operations on float32 (the clips, the stand-in noise, the fake codec and generator), so the digests do not depend on the CPU."""
import hashlib
import types

import numpy as np
import pytest
import torch

from test_gpu_job_stream import kinds_of
from test_shared_sweep_host import H, W, FakeElic, FakeReceiver, packed

sha = lambda b: hashlib.sha256(b).hexdigest()      # noqa: E731


# ---- bytes ------------------------------------------------------------------------------------------------------

def seeded_strings(rng, n_clips):
    """[y_strings[5][2][n_clips], z_strings[n_clips]] of 0..8 random bytes each (about one string in nine is empty)."""
    mk = lambda: bytes(rng.integers(0, 256, int(rng.integers(0, 9)), dtype=np.uint8))      # noqa: E731
    return [[[[mk() for _ in range(n_clips)] for _ in range(2)] for _ in range(5)], [mk() for _ in range(n_clips)]]


JOB_SEGMENTS = [("key", 2), ("gen", 3), ("key", 2), ("gen", 5), ("key", 1)]
JOB_ARGS = dict(shape=(2, 3), codec=(0, 4), seed=(9 << 32) | 1234, stream_id=41, vid=17, q=4, thr=0.29, sampler="DDIM",
                subsample=50, denoise=True)


def container_input():
    rng = np.random.default_rng(2024)
    d = np.zeros(9, dtype=np.int64)
    d[[0, 1, 6]] = 1
    return d, [seeded_strings(rng, 2) for _ in range(3)], (2, 3)


def job_input(fmt):
    rng = np.random.default_rng(2025)
    keys = [seeded_strings(rng, 1) for _ in range(5)]
    return keys, dict(JOB_ARGS, **(dict(plan=(1, 7), crc=0xDEADBEEF) if fmt == 4 else {}))


def test_pack_writes_the_pinned_bytes_and_unpack_returns_the_input():
    from evc_amd import container
    d, keys, shape = container_input()
    assert any(s == b"" for k in keys for sl in k[0] for p in sl for s in p)
    blob = container.pack(d, keys, shape, codec=(1, 4))
    print("pack:", len(blob), sha(blob))
    assert (len(blob), sha(blob)) == (507, "f6861bbdf26797d5b6d0657fde843f1d6db48391d92c1d72044efffc1c64e81c")
    d2, keys2, shape2 = container.unpack(blob, expect_codec=(1, 4))
    assert d2.tolist() == d.tolist() and keys2 == keys and shape2 == shape


@pytest.mark.parametrize("fmt, size, digest", [(3, 497, "9dd097b4dcf748bae8c08a50c366a38e54dcea15dc75486158649b9d5fc075be"),
                                               (4, 504, "7b4b815a974633b5a9bb2a0f2d52408f5da45f50b0105f2072c83ce2a698a157")])
def test_pack_job_writes_the_pinned_bytes_and_unpack_job_returns_the_input(fmt, size, digest):
    from evc_amd import container
    keys, args = job_input(fmt)
    blob = container.pack_job(JOB_SEGMENTS, keys, **args)
    print(f"pack_job format {fmt}:", len(blob), sha(blob))
    assert (blob[4], len(blob), sha(blob)) == (fmt, size, digest)
    job = container.unpack_job(blob, expect_codec=args["codec"], expect_plan_revision=7)
    assert job["key_strings"] == keys and job["segments"] == JOB_SEGMENTS and job["shape"] == args["shape"]
    assert job["d"].tolist() == [1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 1] and job["frames"] == 13 and job["format"] == fmt
    assert (job["plan"], job["crc"]) == (((1, 7), 0xDEADBEEF) if fmt == 4 else (None, None))
    assert (job["seed"], job["stream_id"], job["vid"], job["q"], job["thr"]) == ((9 << 32) | 1234, 41, 17, 4, np.float32(0.29))
    assert (job["sampler"], job["subsample"], job["denoise"], job["codec"]) == ("DDIM", 50, True, (0, 4))


def small_streams():
    """One stream of each kind, as small as the formats allow: one key frame of one clip in a mask of two frames; one job of two
    key frames and one generated frame in format 3 and in format 4."""
    from evc_amd import container
    rng = np.random.default_rng(7)
    one = container.pack([1, 0], [seeded_strings(rng, 1)], (1, 1))
    keys = [seeded_strings(rng, 1) for _ in range(2)]
    job3 = container.pack_job([("key", 2), ("gen", 1)], keys, **JOB_ARGS)
    job4 = container.pack_job([("key", 2), ("gen", 1)], keys, **dict(JOB_ARGS, plan=(1, 7), crc=5))
    return dict(container=(container.unpack, one), job3=(container.unpack_job, job3), job4=(container.unpack_job, job4))


# what reading the first ``cut`` bytes raises, for every cut from ``first`` up to the next entry's: [first cut, type, message]
TRUNCATIONS = dict(
    container=[[0, ValueError, "not an EVC1 container"], [18, ValueError, "buffer is smaller than requested size"],
               [20, ValueError, "truncated container"]],
    job3=[[0, ValueError, "not an EVC1 container"], [8, ValueError, "truncated job stream"]],
    job4=[[0, ValueError, "not an EVC1 container"], [8, ValueError, "truncated job stream"]])


def truncation_runs(read, blob):
    runs = []
    for cut in range(len(blob)):
        try:
            read(blob[:cut])
            got = [cut, None, ""]
        except Exception as e:       # the type and the words are what is pinned
            got = [cut, type(e), str(e)]
        if not runs or runs[-1][1:] != got[1:]:
            runs.append(got)
    return runs


@pytest.mark.parametrize("kind", ["container", "job3", "job4"])
def test_every_truncation_raises_the_pinned_message(kind):
    read, blob = small_streams()[kind]
    read(blob)
    runs = truncation_runs(read, blob)
    print(kind, len(blob), [[c, t.__name__ if t else None, m] for c, t, m in runs])
    assert runs == TRUNCATIONS[kind]
    with pytest.raises(ValueError, match="^trailing bytes in " + ("container" if kind == "container" else "job stream") + "$"):
        read(blob + b"\0")


# ---- launches ---------------------------------------------------------------------------------------------------

FRAMES = 17
SEED = 5
QS = [3, 4]
THRESHOLDS = [-100.0, 200.0, 16.0, 19.0, 22.0]


def integer_clips():
    """One clip of smooth motion with a turn in the middle (as tests/test_shared_sweep_host.py makes them), from integers: grey
    levels / 255."""
    rng = np.random.default_rng(11)
    clips = {}
    for vid in (0,):
        base = rng.integers(80, 176, (3, H, W))
        drift = rng.integers(-2, 3, (3, H, W))
        turn = 8
        steps = np.asarray([f if f < turn else 2 * turn - f for f in range(FRAMES)])
        wobble = rng.integers(-1, 2, (FRAMES, 3, H, W))
        levels = np.clip(base[None] + steps[:, None, None, None] * drift[None] + wobble, 0, 255)
        clips[vid] = torch.from_numpy(levels.astype(np.float32) / np.float32(255))
    return clips


def integer_noise(keys, shape, seed, step, raw=False, out=None):
    """Stand-in for ``lib.noise_normal`` keyed like N1: uniform multiples of 2^-13 in [-4, 4), exact in float32 on any CPU."""
    rows = [np.random.default_rng([int(seed), int(sid), int(start), int(step)]).integers(-2 ** 15, 2 ** 15, tuple(shape[1:]))
            for sid, start in keys.tolist()]
    return torch.from_numpy((np.stack(rows) / 2 ** 13).astype(np.float32))


class Tape:
    """Everything a run did, in order, as one SHA-256."""

    def __init__(self):
        self.h, self.calls = hashlib.sha256(), {}

    def add(self, kind, *parts):
        self.calls[kind] = self.calls.get(kind, 0) + 1
        for p in (kind,) + parts:
            self.h.update(p if isinstance(p, bytes) else repr(p).encode())
            self.h.update(b"|")

    def digest(self):
        return self.h.hexdigest()


class TapedElic(FakeElic):
    def __init__(self, q, levels, tape):
        super().__init__(levels)
        self.q, self.tape = q, tape

    def compress(self, x):
        self.tape.add("compress", self.q, tuple(x.shape), x.contiguous().numpy().tobytes())
        return super().compress(x)

    def decompress(self, strings, shape):
        ys, zs = strings
        self.tape.add("decompress", self.q, tuple(shape), tuple(sha(s) for sl in ys for p in sl for s in p), tuple(sha(z) for z in zs))
        return super().decompress(strings, shape)


def taped_generator(monkeypatch, tape):
    """The fake receiver of tests/test_shared_sweep_host.py (it serves as the sender's generator too) on the integer noise, every
    ``generate`` on the tape: the rows, the flag and the "init" noise."""
    from evc_amd import lib
    rx = FakeReceiver(monkeypatch)
    monkeypatch.setattr(lib, "noise_normal", integer_noise)
    inner = rx.generate

    def generate(cond, noise_fn=None, generator=None, groups=None, invariant=None):
        z = noise_fn("init", (cond.shape[0], 15, H, W))
        tape.add("generate", tuple(cond.shape), cond.numpy().tobytes(), invariant, groups, z.numpy().tobytes())
        return inner(cond, noise_fn=noise_fn, generator=generator, groups=groups, invariant=invariant)
    rx.generate = generate
    return rx


def taped_results(tape, jobs):
    for vid, q, r in jobs:
        tape.add("result", vid, q, r["thr"], r["x"].tobytes(), r["d"].tolist(), r["bits"], r["bpp"], r["segments"], r["stream_id"],
                 r["seed"], r["key_strings"], tuple(r["shape"]), r["invariant"])


def flat_stats(stats):
    return sorted((k, sorted(v.items()) if isinstance(v, dict) else v) for k, v in stats.items())


def send(share):
    from evc_amd import policy as P
    tape = Tape()
    models = {3: TapedElic(3, 63, tape), 4: TapedElic(4, 255, tape)}
    stats = {}
    with pytest.MonkeyPatch.context() as mp:
        res = P.run_policy(taped_generator(mp, tape), models, integer_clips(), QS, THRESHOLDS, P.PsnrMetric(), patch=64,
                           frames=FRAMES, max_batch=7, seed=SEED, bpp_limit=1e9, device="cpu", noise="evc", stats=stats,
                           noise_streams="group", share=share, log=lambda line: tape.add("log", line))
    jobs = [(vid, q, r) for (vid, q), lst in res.items() for r in lst]
    taped_results(tape, jobs)
    assert stats.pop("noise_host_seconds") > 0
    tape.add("stats", flat_stats(stats))
    return types.SimpleNamespace(jobs=jobs, tape=tape, stats=stats)


@pytest.fixture(scope="module")
def sent():
    cache = {}
    return lambda share: cache[share] if share in cache else cache.setdefault(share, send(share))


SENDER = {False: "6a1121253e560e60822cbc2dc25e3e52b5b46562d44278965e421e19a8f144c7",
          True: "fd18780c1b863fde6385a203e56073603ac6419f7fdf8f8f6ba70b520de0feb5"}


@pytest.mark.parametrize("share", [False, True])
def test_run_policy_makes_the_pinned_calls(sent, share):
    s = sent(share)
    seen = set()
    for _, _, r in s.jobs:
        seen |= kinds_of(r["segments"], FRAMES)
    assert seen == {"partial", "fallback", "clip-end"}, seen          # the sweep holds every kind of program
    assert len(s.jobs) == len(QS) * len(THRESHOLDS) and max(s.stats["launch_sizes"]) == 7 and len(s.stats["launch_sizes"]) > 1
    print(f"run_policy share={share}:", s.tape.calls, s.tape.digest())
    assert s.tape.digest() == SENDER[share]


RECEIVER = {          # (share, max_batch, formats)
    (False, 1, 3): "d5eb5473668e8cc812dd53dad1ce3a29edaf46602434fadf56f6bea686d82616",
    (False, 1, 4): "6cab957009dbe412280eb6e950f049f4184be06d8f80c581a4e60dcb123063c0",
    (False, 1, "3 and 4"): "07b8e0bda15ed0517500a86ae669b415c188af2b696a5aa4a73e19cbcf28f4bb",
    (False, 7, 3): "a104d040f508cb39fd80487a565b70ffd7ada3c1e643aff98915e13f8ea311f3",
    (False, 7, 4): "36dcbffaae9a68e3162a837e0764c3cfb100ffff96647e9fe793751fe9f85c44",
    (False, 7, "3 and 4"): "42535df416f63a3035b56e3c982eec1ec790489034a78d20cf370c56bb9cc86b",
    (True, 1, 3): "8485a50c938f9b4dc634fe5f6f6a1488706f410732b53f3bef49363ae41cde4e",
    (True, 1, 4): "c30090598897a5b2ebfe6016c8df0aa74dd7cde7017242401c8431b7c26e9b55",
    (True, 1, "3 and 4"): "0a9381684801bbd172666f4f5ca5606e725f248370fc6ac304451f28bd9c0720",
    (True, 7, 3): "482ab75611a650a5f3379a747d559b95040f9f8d93984be19c1c5506ee722599",
    (True, 7, 4): "2cfde649b90c3daf621a6d850ad9bf0cf0c247f9cbe89986796df4ace2b15d8e",
    (True, 7, "3 and 4"): "9bbc5dc9b06ac5885cd06ec2f2d9e9965181d63694ee390b9a3cbdfdf6abf6a7"}


@pytest.mark.parametrize("fmt", [3, 4, "3 and 4"])
@pytest.mark.parametrize("max_batch", [1, 7])
@pytest.mark.parametrize("share", [False, True])
def test_decode_jobs_makes_the_pinned_calls(sent, monkeypatch, share, max_batch, fmt):
    """The streams of the shared sender (group streams: the receiver has states to share).  "3 and 4": every other job is a
    format-4 stream, so a round has launches of both kinds."""
    tape = Tape()
    models = {3: TapedElic(3, 63, tape), 4: TapedElic(4, 255, tape)}
    world = types.SimpleNamespace(models=models)
    jobs = [packed(world, r, vid, q, invariant=(fmt == 4 or (fmt != 3 and i % 2 == 1))) for i, (vid, q, r) in enumerate(sent(True).jobs)]
    stats = {}
    out = taped_generator(monkeypatch, tape).decode_jobs(jobs, max_batch=max_batch, models=models, size=(H, W), share=share,
                                                         stats=stats)
    for (vid, q, r), x in zip(sent(True).jobs, out):
        assert np.array_equal(x.numpy(), r["x"]), (vid, q, r["thr"])       # the fakes are elementwise: the sender's frames
        tape.add("frames", x.numpy().tobytes())
    tape.add("stats", flat_stats(stats))
    print(f"decode_jobs {(share, max_batch, fmt)}:", tape.calls, tape.digest())
    assert tape.digest() == RECEIVER[(share, max_batch, fmt)]
