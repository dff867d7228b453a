"""Pins of the call sequences that tests/test_lockstep_pins_host.py predates: the sender's sweep with noise trials, the sweep
on a ``noise_source``, and the receiver on format-5 / format-6 streams.  The tape, the fakes, the clips and the integer noise are
that file's; every digest covers each ``compress``, ``decompress`` and ``generate`` call with its bytes, the log lines, the results
and the statistics.

Every digest below was computed on the commit before ``policy.run_policy`` became named steps and both sides launched through
``policy.generation_launch``, where this file passes unchanged (but for the one test of ``policy.torch_noise_seed``, a name that
commit does not have)."""
import types

import numpy as np
import pytest
import torch

import test_shared_sweep_host as SS
from test_gpu_job_stream import kinds_of
from test_lockstep_pins_host import (FRAMES, QS, SEED, THRESHOLDS, Tape, TapedElic, flat_stats, integer_clips, taped_generator,
                                     taped_results)
from test_shared_sweep_host import H, W

K = 3


def taped_trials(tape, jobs):
    for vid, q, r in jobs:
        tape.add("trials", vid, q, r["thr"], r["n_trials"], r["trials"], r["trial_bits"])


def send(max_batch, source=None, **kw):
    """``source``: a ``noise_source`` that takes the tape first."""
    from evc_amd import policy as P
    tape = Tape()
    if source is not None:
        kw["noise_source"] = lambda *args: source(tape, *args)
    models = {3: TapedElic(3, 63, tape), 4: TapedElic(4, 255, tape)}
    stats = {}
    with pytest.MonkeyPatch.context() as mp:
        res = P.run_policy(taped_generator(mp, tape), models, integer_clips(), QS, THRESHOLDS, P.PsnrMetric(), patch=64,
                           frames=FRAMES, max_batch=max_batch, seed=SEED, bpp_limit=1e9, device="cpu", noise="evc", stats=stats,
                           log=lambda line: tape.add("log", line), **kw)
    jobs = [(vid, q, r) for (vid, q), lst in res.items() for r in lst]
    taped_results(tape, jobs)
    taped_trials(tape, jobs)
    assert stats.pop("noise_host_seconds") > 0
    tape.add("stats", flat_stats(stats))
    return types.SimpleNamespace(jobs=jobs, tape=tape, stats=stats)


@pytest.fixture(scope="module")
def sent():
    cache = {}
    return lambda share: cache[share] if share in cache else cache.setdefault(
        share, send(10, noise_streams="group", trials=K, share=share))


# ---- the sender with trials -------------------------------------------------------------------------------------

SENDER = {False: ("b4d37e11f216a06195de7033c0c87aa64fc6d6a9f97700eced18a927a2e049d5", 24),
          True: ("abab19a75c4619cb3f2ca5a18eae92f8dc76fab336774f9907ad7c41e9f16234", 17)}


@pytest.mark.parametrize("share", [False, True])
def test_run_policy_with_trials_makes_the_pinned_calls(sent, share):
    """max_batch = 10: a launch holds up to three states of K = 3 samples, and partial launches occur."""
    s = sent(share)
    seen, chosen = set(), set()
    for _, _, r in s.jobs:
        seen |= kinds_of(r["segments"], FRAMES)
        chosen |= {t for (kind, _), t in zip(r["segments"], r["trials"]) if kind == "gen"}
        assert r["n_trials"] == K
    sizes = s.stats["launch_sizes"]
    assert seen == {"partial", "fallback", "clip-end"}, seen          # the sweep holds every kind of program
    assert chosen == {0, 1, 2}, chosen                                # ... and every trial is some job's choice
    assert len(sizes) > 1 and all(n % K == 0 for n in sizes), sizes
    assert len(s.jobs) == len(QS) * len(THRESHOLDS) and s.stats["trial_prefixes"]
    print(f"run_policy trials={K} share={share}:", s.tape.calls, sorted(sizes.items()), s.tape.digest())
    digest, launches = SENDER[share]
    assert sorted(sizes) == [3, 6, 9] and sum(sizes.values()) == launches == s.tape.calls["generate"]
    assert s.tape.digest() == digest


# ---- the sender on a noise source -------------------------------------------------------------------------------

SOURCE = "d23afbc2fca7c9cc44e8a69b9162fb502ed2cb03a9f414b51f95b526ef583cb5"


def integer_source(tape, job, rnd, step, shape):
    """Integers as ``integer_noise`` makes them, keyed by the source's own (job, round, step); every call goes on the tape."""
    vid, q, thr = job
    tape.add("noise_source", vid, q, thr, rnd, step, tuple(shape))
    rng = np.random.default_rng([SEED, int(vid), int(q), THRESHOLDS.index(thr), int(rnd), int(step)])
    return torch.from_numpy((rng.integers(-2 ** 15, 2 ** 15, tuple(shape)) / 2 ** 13).astype(np.float32))


def test_run_policy_on_a_noise_source_makes_the_pinned_calls():
    """One stream per job, one trial, the noise injected."""
    s = send(7, source=integer_source, noise_streams="job", trials=1)
    assert [r["stream_id"] for _, _, r in s.jobs] == list(range(len(QS) * len(THRESHOLDS)))
    assert all(r["n_trials"] == 1 and r["trial_bits"] == 0 for _, _, r in s.jobs) and "trial_prefixes" not in s.stats
    print("run_policy noise_source:", s.tape.calls, sorted(s.stats["launch_sizes"].items()), s.tape.digest())
    assert (s.tape.calls["noise_source"], s.tape.calls["generate"]) == (120, 13)
    assert s.tape.digest() == SOURCE


# ---- the receiver on trial streams ------------------------------------------------------------------------------

def packed_trials(r, vid, q, invariant):
    """As tests/test_trials_host.py packs them: format 5, or format 6 with the batch-invariant plan."""
    from evc_amd import container
    extra = dict(plan=(container.PLAN_INVARIANT, 1), crc=container.frames_crc(r["x"])) if invariant else {}
    blob = container.pack_job(r["segments"], r["key_strings"], r["shape"], (1, 1), r["seed"], r["stream_id"], vid, q, r["thr"],
                              "DDPM", 2, True, trials=r["trials"], n_trials=r["n_trials"], **extra)
    assert blob[4] == (6 if invariant else 5)
    return container.unpack_job(blob, expect_codec=(1, 1))


RECEIVER = {          # (share, max_batch, formats)
    (False, 1, 5): "6d7e8c768785ec274ebc15c25d3e2385f460f6068d7fa5885769b9b24f8c3f6d",
    (False, 1, 6): "a5686bdf7c17e690fb8c06b8d55299bdca969f8a7cafabee210aff790a1cd5e0",
    (False, 1, "5 and 6"): "efd4e1e9b2078a038bc5089421bafd8ccef04e3b9770c18de412a7cac9d91388",
    (False, 7, 5): "b2be460f61bd80178fc013c6937062de9fb26cbdd0086845cda78fe7f53d90a4",
    (False, 7, 6): "c416470cc72aa93ca98a1323e59852292cbb81e6802ccd7334f80c7b4b6cfe24",
    (False, 7, "5 and 6"): "34a1c31222db209bbb8c506bff24e123b933f98e9290454cc4935127247155ff",
    (True, 1, 5): "a49f14cdf01e05a1521afd15bdf59cc0a6f70224ba15726b666465ad79030988",
    (True, 1, 6): "2dda973cc3173fb4000809897de469795cd4ee65362ff640b5ece485bab0c615",
    (True, 1, "5 and 6"): "443e42140b71fe7d08db1d4ea89e44aa2a8e42802b2e49c4ce6db673338ef994",
    (True, 7, 5): "5b75a6427ebf88e9d627203f56d37286594593b47ba9987fabdbac46ca114689",
    (True, 7, 6): "50b8aa63ee77010c49bc093a3b7f4d05ffee58b3e71619934b4cc020b48a5920",
    (True, 7, "5 and 6"): "3b8092fc1b56ed336b31bab88534a77bd698b6197bb536e3d21a69a0060caeab"}


@pytest.mark.parametrize("fmt", [5, 6, "5 and 6"])
@pytest.mark.parametrize("max_batch", [1, 7])
@pytest.mark.parametrize("share", [False, True])
def test_decode_jobs_on_trial_streams_makes_the_pinned_calls(sent, monkeypatch, share, max_batch, fmt):
    """The streams of the shared sender with trials.  "5 and 6": every other job is a format-6 stream, so a round has launches of
    both kinds."""
    tape = Tape()
    models = {3: TapedElic(3, 63, tape), 4: TapedElic(4, 255, tape)}
    jobs = [packed_trials(r, vid, q, invariant=(fmt == 6 or (fmt != 5 and i % 2 == 1))) for i, (vid, q, r) in enumerate(sent(True).jobs)]
    stats = {}
    out = taped_generator(monkeypatch, tape).decode_jobs(jobs, max_batch=max_batch, models=models, size=(H, W), share=share,
                                                         stats=stats)
    for (vid, q, r), x in zip(sent(True).jobs, out):
        assert np.array_equal(x.numpy(), r["x"]), (vid, q, r["thr"])       # the fakes are elementwise: the sender's frames
        tape.add("frames", x.numpy().tobytes())
    tape.add("stats", flat_stats(stats))
    print(f"decode_jobs {(share, max_batch, fmt)}:", tape.calls, tape.digest())
    assert tape.digest() == RECEIVER[(share, max_batch, fmt)]


# ---- the seed of noise="torch" ----------------------------------------------------------------------------------

def test_torch_noise_seed_is_the_restatement():
    """``policy.torch_noise_seed`` against the restatement of tests/test_shared_sweep_host.py, fields that overflow included:
    a stream id past 20 bits and a start frame past 6 bits spill into the fields above them, in both alike."""
    from evc_amd import policy as P
    for seed, sid, at, step in [(0, 0, 0, 0), (SEED, 3, 2, 0), (SEED, 119, 29, 1000), (2 ** 40 + 77, 5, 7, 9), (5, 2 ** 20, 3, 1),
                                (5, 2 ** 20 + 9, 63, 1023), (5, 1, 64, 0), (5, 7, 2 + 2 * 65536, 3), (2 ** 63 - 1, 2 ** 31, 200, 1023)]:
        assert P.torch_noise_seed(seed, sid, at, step) == SS.torch_noise_seed(seed, sid, at, step), (seed, sid, at, step)
