"""Host tests of noise trials (``policy.run_policy(trials=K)``): container formats 5 / 6, ``choose_trial``, the sweep on the fake
generator and codec of tests/test_shared_sweep_host.py with noise specification N1 restated on the CPU (tests/noise_ref.py), and
the receiver on the same fakes.  No GPU; the GPU side is tests/test_gpu_trials.py."""
import struct
import types

import numpy as np
import pytest
import torch

import noise_ref as NR
from test_job_stream_host import N_KEY, SEGMENTS, key_frame, packed
from test_shared_sweep_host import (FRAMES, H, SEED, W, FakeDecoder, FakeElic, FakeReceiver, assert_same_results, jobs_of,
                                    make_clips)

TRIALS = [0, 2, 1, 0, 0, 1, 2, 0, 0]                   # one per segment of SEGMENTS: 0 for key, any of 0..2 for gen
QS = [3]
THRESHOLDS = [-100.0, 200.0, 24.5, 27.0, 29.0, 31.5]   # accept all, reject all, four inside what the fake generator reaches
K = 3


# ---- container formats 5 and 6 ---------------------------------------------------------------------------------

def heads():
    from evc_amd import container
    head = 8 + struct.calcsize(container._JOB_HEAD)
    return head, head + struct.calcsize(container._PLAN_HEAD)


def test_formats_5_and_6_round_trip():
    from evc_amd import container
    plain = container.unpack_job(packed())
    for extra, fmt in ((dict(), 5), (dict(plan=(1, 7), crc=0xDEADBEEF), 6)):
        blob = packed(trials=TRIALS, n_trials=3, **extra)
        assert blob[4] == fmt
        job = container.unpack_job(blob, expect_codec=(0, 3), expect_plan_revision=7)
        assert job["format"] == fmt and job["segments"] == SEGMENTS and job["trials"] == TRIALS and job["n_trials"] == 3
        assert all(len(s) == 2 for s in job["segments"])
        assert job["key_strings"] == [key_frame(k) for k in range(N_KEY)] and job["noise_spec"] == container.NOISE_N1
        assert job["d"].tolist() == plain["d"].tolist()
        assert (job["plan"], job["crc"]) == (((1, 7), 0xDEADBEEF) if extra else (None, None))
        assert len(blob) == len(packed(**extra)) + 1 + len(SEGMENTS)             # u8 n_trials + one byte per segment
    # all trials 0 is a legal choice of a K = 255 sweep
    assert container.unpack_job(packed(trials=[0] * len(SEGMENTS), n_trials=255))["n_trials"] == 255


def test_one_trial_writes_todays_bytes_and_formats_3_and_4_read_as_before():
    from evc_amd import container
    for extra, fmt in ((dict(), 3), (dict(plan=(1, 7), crc=5), 4)):
        blob = packed(**extra)
        assert packed(n_trials=1, **extra) == blob
        assert packed(trials=None, n_trials=1, **extra) == blob
        assert packed(trials=[0] * len(SEGMENTS), n_trials=1, **extra) == blob
        job = container.unpack_job(blob)
        assert job["format"] == fmt and job["trials"] == [0] * len(SEGMENTS) and job["n_trials"] == 1
        assert job["segments"] == SEGMENTS


def test_corrupt_trials_are_refused_when_writing():
    for trials, n in ((TRIALS, 1),                                  # a trial without trials
                      (TRIALS, 0), ([0] * len(SEGMENTS), 0),        # n_trials < 1
                      ([1] + TRIALS[1:], 3),                        # a key segment with a trial
                      (TRIALS[:1] + [3] + TRIALS[2:], 3),           # trial >= n_trials
                      (TRIALS[:1] + [-1] + TRIALS[2:], 3),
                      (TRIALS[:-1], 3),                             # one number short
                      (TRIALS, 256)):                               # more than a byte names
        with pytest.raises(ValueError):
            packed(trials=trials, n_trials=n)


def test_corrupt_trials_are_refused_when_reading():
    from evc_amd import container
    for extra, head in zip((dict(), dict(plan=(1, 7), crc=5)), heads()):
        blob = packed(trials=TRIALS, n_trials=3, **extra)
        seg = head + 1                                             # u8 n_trials, then 3 bytes per segment
        assert blob[head] == 3 and blob[seg:seg + 6] == bytes([0, 2, 0, 1, 3, 2])
        container.unpack_job(blob)
        bad = bytearray(blob); bad[seg + 2] = 1                    # noqa: E702  the first key segment names trial 1
        with pytest.raises(ValueError, match="key segment"):
            container.unpack_job(bytes(bad))
        bad = bytearray(blob); bad[seg + 5] = 3                    # noqa: E702  gen segment: trial 3 of 3
        with pytest.raises(ValueError, match="trial 3 of 3"):
            container.unpack_job(bytes(bad))
        bad = bytearray(blob); bad[head] = 2                       # noqa: E702  n_trials 2 below the trials named
        with pytest.raises(ValueError, match="trial 2 of 2"):
            container.unpack_job(bytes(bad))
        zero = packed(trials=[0] * len(SEGMENTS), n_trials=3, **extra)
        for n in (0, 1):                                           # n_trials < 2, every trial 0
            bad = bytearray(zero); bad[head] = n                   # noqa: E702
            with pytest.raises(ValueError, match="2..255"):
                container.unpack_job(bytes(bad))
        # the rules of formats 3 / 4 hold as they did
        bad = bytearray(blob); bad[seg + 4] = 4                    # noqa: E702  gen 3 -> gen 4
        with pytest.raises(ValueError, match="add up"):
            container.unpack_job(bytes(bad))
        bad = bytearray(blob); bad[seg] = 7                        # noqa: E702
        with pytest.raises(ValueError, match="segment kind"):
            container.unpack_job(bytes(bad))
        with pytest.raises(ValueError, match="trailing"):
            container.unpack_job(blob + b"\0")
        with pytest.raises(ValueError, match="noise specification id 2"):
            container.unpack_job(packed(trials=TRIALS, n_trials=3, noise_spec=2, **extra))


def test_truncated_streams_are_refused():
    from evc_amd import container
    for extra in (dict(), dict(plan=(1, 7), crc=5)):
        blob = packed(trials=TRIALS, n_trials=3, **extra)
        for cut in range(len(blob)):
            with pytest.raises(ValueError):
                container.unpack_job(blob[:cut])
    with pytest.raises(ValueError, match="not a job stream"):
        container.unpack_job(packed()[:4] + b"\x07" + packed()[5:])


# ---- choose_trial ----------------------------------------------------------------------------------------------

def test_choose_trial_rules():
    from evc_amd import policy as P
    psnr = P.PsnrMetric()
    dist = P.CallableMetric(lambda a, b: None)
    assert psnr.better(2.0, 1.0) and not psnr.better(1.0, 1.0) and not psnr.better(1.0, 2.0)
    assert dist.better(1.0, 2.0) and not dist.better(1.0, 1.0) and not dist.better(2.0, 1.0)
    assert P.PsnrDeviceMetric().better(2.0, 1.0) and P.PsnrDeviceMetric.name == "psnr"
    # the longest prefix wins over a better mean
    assert P.choose_trial([[40, 40, 9, 40, 40], [31, 31, 31, 9, 9], [50, 9, 9, 9, 9]], 30.0, psnr) == (1, 3)
    assert P.choose_trial([[.01, .01, .9, 0, 0], [.2, .2, .2, .9, 0]], 0.3, dist) == (1, 3)
    # a frame after the first rejected one does not count
    assert P.choose_trial([[31, 9, 31, 31, 31], [31, 31, 9, 9, 9]], 30.0, psnr) == (1, 2)
    # equal prefixes: the better mean over the accepted frames, in the metric's direction
    assert P.choose_trial([[31, 31, 9], [31, 33, 9], [32, 31, 1]], 30.0, psnr) == (1, 2)
    assert P.choose_trial([[.2, .2, .9], [.2, .1, .9], [.1, .25, .9]], 0.3, dist) == (1, 2)
    assert P.choose_trial([[.2, .1, .9], [.2, .2, .9]], 0.3, dist) == (0, 2)
    # a full tie: the lowest trial
    assert P.choose_trial([[9, 9], [31, 32], [32, 31], [31, 32]], 30.0, psnr) == (1, 2)
    assert P.choose_trial([[np.inf, np.inf], [np.inf, np.inf]], 30.0, psnr) == (0, 2)
    # nobody accepts the first frame; NaN is never accepted
    assert P.choose_trial([[9, 40, 40], [29.99, 40, 40]], 30.0, psnr) == (None, 0)
    assert P.choose_trial([[np.nan, 40], [np.nan, 40]], 30.0, psnr) == (None, 0)
    assert P.choose_trial([[np.nan, 40], [31, np.nan]], 30.0, psnr) == (1, 1)
    assert P.choose_trial([[31, 31, 31]], 30.0, psnr) == (0, 3) and P.choose_trial([[9]], 30.0, psnr) == (None, 0)
    assert P.accepted_prefixes([[31, 9, 31], [31, 31, 31], [9, 31, 31]], 30.0, psnr) == [1, 3, 0]
    assert P.trial_bits(SEGMENTS, 1) == 0 and [P.trial_bits(SEGMENTS, k) for k in (2, 3, 4, 5, 255)] == [5, 10, 10, 15, 40]
    assert P.trial_start(7, 0) == 7 and P.trial_start(7, 2) == 7 + 2 * 65536


# ---- the sweep on the fakes ------------------------------------------------------------------------------------

@pytest.fixture
def n1_on_cpu(monkeypatch):
    """``lib.noise_keys`` / ``lib.noise_normal`` restated on the CPU from the specification (tests/noise_ref.py)."""
    from evc_amd import lib
    cache = {}

    def noise_keys(pairs, device):
        return torch.tensor([[int(a), int(b)] for a, b in pairs], dtype=torch.int64)

    def noise_normal(keys, shape, seed, step, raw=False, out=None):
        n = int(np.prod(shape[1:]))
        rows = []
        for sid, start in keys.tolist():
            k = (int(seed), sid, start, int(step), n)
            if k not in cache:
                cache[k] = torch.from_numpy(NR.normals(*k).astype(np.float32)).reshape(tuple(shape[1:]))
            rows.append(cache[k])
        return torch.stack(rows)
    monkeypatch.setattr(lib, "noise_keys", noise_keys)
    monkeypatch.setattr(lib, "noise_normal", noise_normal)
    return cache


class Dec(FakeDecoder):
    """The fake generator with what ``noise="evc"`` reads off a decoder, recording every launch's keys-in-order output."""

    def __init__(self):
        from evc_amd.config import default_config
        super().__init__()
        self.config = default_config(32, 32, 64, subsample=2)
        self.launches = []

    def generate(self, cond, noise_fn=None, groups=None, invariant=None):
        out = super().generate(cond, noise_fn, groups, invariant)
        self.launches.append(out)
        return out


@pytest.fixture
def sweep(n1_on_cpu):
    from evc_amd import policy as P
    clips, models = make_clips(), {3: FakeElic(63)}

    def run(**kw):
        dec, stats = Dec(), {}
        kw.setdefault("max_batch", 9)
        res = P.run_policy(dec, models, clips, QS, THRESHOLDS, P.PsnrMetric(), patch=64, frames=FRAMES, seed=SEED,
                           bpp_limit=kw.pop("bpp_limit", 1e9), device="cpu", noise="evc", stats=stats, **kw)
        return types.SimpleNamespace(res=res, stats=stats, dec=dec)
    return types.SimpleNamespace(P=P, run=run, clips=clips, models=models)


def gen_segments(r):
    return sum(1 for k, _ in r["segments"] if k == "gen")


def consistent_choice(P, prefixes, chosen):
    """``chosen`` is what ``choose_trial`` can return for these accepted prefixes: None when there is none, else a trial of the
    longest one -- which of those, the mean decides; with all means equal, ``choose_trial`` on the prefixes says the lowest."""
    flat = types.SimpleNamespace(accept=lambda v, thr: v >= thr, better=lambda a, b: a > b)
    lowest, longest = P.choose_trial([[1.0] * a + [-1.0] for a in prefixes], 0.0, flat)
    assert longest == max(prefixes)
    if longest == 0:
        assert chosen is None and lowest is None
    else:
        assert chosen is not None and prefixes[chosen] == longest and chosen >= lowest


def test_one_trial_is_the_call_without_the_argument(sweep):
    for kw in (dict(), dict(noise_streams="group", share=True)):
        a, b = sweep.run(**kw), sweep.run(trials=1, **kw)
        assert_same_results(a.res, b.res)
        assert a.stats["launch_sizes"] == b.stats["launch_sizes"] and "trial_prefixes" not in b.stats
        for _, _, r in jobs_of(b.res):
            assert r["n_trials"] == 1 and r["trials"] == [0] * len(r["segments"]) and r["trial_bits"] == 0
            assert r["bpp"] == sum(r["bits"]) / H / W / FRAMES


def test_refusals(sweep):
    P = sweep.P
    one = dict(patch=64, frames=7, device="cpu", bpp_limit=1e9, seed=SEED)
    args = (sweep.models, {0: sweep.clips[0]}, [3], [-100.0], P.PsnrMetric())
    with pytest.raises(ValueError, match="noise='evc'"):
        P.run_policy(Dec(), *args, trials=2, **one)                                # noise="torch"
    with pytest.raises(ValueError, match="noise_source"):
        P.run_policy(Dec(), *args, trials=2, noise="evc", noise_source=lambda job, rnd, step, shape: torch.zeros(shape), **one)
    with pytest.raises(ValueError, match="max_batch"):
        P.run_policy(Dec(), *args, trials=5, noise="evc", max_batch=4, **one)
    with pytest.raises(ValueError, match="255"):
        P.run_policy(Dec(), *args, trials=256, noise="evc", max_batch=512, **one)
    with pytest.raises(ValueError, match="trials"):
        P.run_policy(Dec(), *args, trials=0, noise="evc", **one)


def test_three_trials(sweep):
    P = sweep.P
    base = sweep.run(noise_streams="group")
    ctl = sweep.run(noise_streams="group", trials=K)
    sh = sweep.run(noise_streams="group", share=True, trials=K)
    # every recorded choice is the longest recorded prefix (None when there is none); every launch holds whole states
    assert ctl.stats["trial_prefixes"] and all(n % K == 0 and n <= 9 for n in ctl.stats["launch_sizes"])
    for prefixes, chosen in ctl.stats["trial_prefixes"]:
        assert len(prefixes) == K
        consistent_choice(P, prefixes, chosen)
    executed = sum(gen_segments(r) for _, _, r in jobs_of(ctl.res))
    assert sum(1 for _, c in ctl.stats["trial_prefixes"] if c is not None) == executed
    # trial 0 draws today's key: in the first launch state k's trial 0 is sample k of the K = 1 run's first launch
    first1, first3 = base.dec.launches[0], ctl.dec.launches[0]
    assert first1.shape[0] == 9 and first3.shape[0] == 9
    for k in range(3):
        assert torch.equal(first3[K * k], first1[k])
        assert not torch.equal(first3[K * k + 1], first1[k]) and not torch.equal(first3[K * k + 2], first3[K * k + 1])
    # the first round never accepts less than one draw did; some job took another draw than the first
    for (_, _, r1), (_, _, r3) in zip(jobs_of(base.res), jobs_of(ctl.res)):
        n1 = r1["segments"][1][1] if r1["segments"][1][0] == "gen" else 0
        n3 = r3["segments"][1][1] if r3["segments"][1][0] == "gen" else 0
        assert n3 >= n1
    assert any(t for _, _, r in jobs_of(ctl.res) for t in r["trials"])
    # results: K, one trial per segment, 2 bits per generated segment, counted in bpp
    for _, _, r in jobs_of(ctl.res):
        assert r["n_trials"] == K and len(r["trials"]) == len(r["segments"])
        assert all(t == 0 for (k, _), t in zip(r["segments"], r["trials"]) if k == "key")
        assert all(0 <= t < K for t in r["trials"])
        assert r["trial_bits"] == 2 * gen_segments(r)
        assert r["bpp"] == (sum(r["bits"]) + r["trial_bits"]) / H / W / FRAMES
    assert any(r["trial_bits"] for _, _, r in jobs_of(ctl.res))
    # shared rounds: the same jobs from fewer samples
    assert_same_results(ctl.res, sh.res)
    for (_, _, a), (_, _, b) in zip(jobs_of(ctl.res), jobs_of(sh.res)):
        assert a["trials"] == b["trials"] and a["trial_bits"] == b["trial_bits"]
    samples = lambda st: sum(n * c for n, c in st["launch_sizes"].items())      # noqa: E731
    assert samples(sh.stats) < samples(ctl.stats) and samples(sh.stats) == K * sum(sh.stats["states"])
    assert samples(ctl.stats) == K * sum(ctl.stats["jobs_served"])
    # the bpp cut sees the trial bits: a limit between a job's rate without and with them drops that job
    vid, q, r = next(j for j in jobs_of(ctl.res) if j[2]["trial_bits"])
    limit = (sum(r["bits"]) + r["trial_bits"] / 2) / H / W / FRAMES
    cut = sweep.run(noise_streams="group", trials=K, bpp_limit=limit)
    assert r["thr"] not in [c["thr"] for c in cut.res[(vid, q)]]


def test_the_receiver_generates_the_chosen_draw_only(sweep, monkeypatch):
    from evc_amd import container, lib
    mine = lib.noise_normal                                                      # n1_on_cpu's; FakeReceiver installs its own
    sent = jobs_of(sweep.run(noise_streams="group", share=True, trials=K).res)
    assert any(t for _, _, r in sent for t in r["trials"])
    for fmt6 in (False, True):
        jobs = []
        for vid, q, r in sent:
            extra = dict(plan=(container.PLAN_INVARIANT, 1), crc=container.frames_crc(r["x"])) if fmt6 else {}
            blob = container.pack_job(r["segments"], r["key_strings"], r["shape"], (1, 1), r["seed"], r["stream_id"], vid, q,
                                      r["thr"], "DDPM", 2, True, trials=r["trials"], n_trials=r["n_trials"], **extra)
            assert blob[4] == (6 if fmt6 else 5)
            jobs.append(container.unpack_job(blob, expect_codec=(1, 1)))
        counts = {}
        for share in (False, True):
            for mb in (1, 7):
                rx = FakeReceiver(monkeypatch)
                monkeypatch.setattr(lib, "noise_normal", mine)
                stats = {}
                out = rx.decode_jobs(jobs, max_batch=mb, models=sweep.models, size=(H, W), share=share, stats=stats)
                for (vid, q, r), x in zip(sent, out):
                    assert np.array_equal(x.numpy(), r["x"]), (fmt6, share, mb, vid, q, r["thr"])
                assert stats["samples"] == rx.rows and all(inv == fmt6 for _, inv in rx.launches)
                counts[(share, mb)] = stats["samples"]
        gens = sum(gen_segments(r) for _, _, r in sent)
        assert counts[(False, 1)] == counts[(False, 7)] == gens                  # one sample per gen segment: K never multiplies
        assert counts[(True, 1)] == counts[(True, 7)] < gens
    # a stream whose trial numbers were damaged after unpacking is refused before any generation
    bad = dict(jobs[0], trials=[1] + jobs[0]["trials"][1:])
    with pytest.raises(ValueError, match="key segment"):
        FakeReceiver(monkeypatch).decode_jobs([bad], models=sweep.models, size=(H, W))
