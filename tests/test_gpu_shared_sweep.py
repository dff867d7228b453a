"""GPU tests of shared generation rounds: ``policy.run_policy(noise_streams="group", share=True)`` generates
once per distinct state of a round, ``ClipDecoder.decode_jobs(share=True)`` does the same on the receiving side.  In
batch-invariant mode sharing changes no bit (``np.array_equal`` throughout); in the default mode the shared sender's frames go
through the receiver at the project's existing 60 dB bar.  The reduced generator, clips and threshold grid
are those of tests/test_gpu_job_stream.py and tests/test_gpu_batch_invariant.py; the host side is tests/test_shared_sweep_host.py."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from test_gpu_batch_invariant import L, no_range_events, psnr, stream_of as stream4_of, world  # noqa: F401
from test_gpu_job_stream import kinds_of, stream_of as stream3_of, threshold_grid

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sweep(world, thr, **kw):
    from evc_amd import policy as P
    stats = {}
    res = P.run_policy(world.dec, world.models, world.clips, [3, 4], thr, P.PsnrMetric(), max_batch=32, seed=5, bpp_limit=1e9,
                       noise="evc", noise_streams="group", stats=stats, **kw)
    sent = [(vid, q, r) for vid in (0, 1) for q in (3, 4) for r in res[(vid, q)]]
    assert len(sent) == 2 * 2 * len(thr)
    return types.SimpleNamespace(sent=sent, stats=stats, samples=sum(k * n for k, n in stats["launch_sizes"].items()))


@pytest.fixture(scope="module")
def grid(world):
    return [-100.0, 200.0] + threshold_grid(world)


@pytest.fixture(scope="module")
def invariant_pair(world, grid):
    """The 56-job sweep in invariant mode under group streams, generated per job and generated per state."""
    return sweep(world, grid, batch_invariant=True, share=False), sweep(world, grid, batch_invariant=True, share=True)


def assert_same_jobs(a, b):
    for (vid, q, ra), (_, _, rb) in zip(a, b):
        assert ra["thr"] == rb["thr"] and ra["segments"] == rb["segments"], (vid, q, ra["thr"])
        assert np.array_equal(ra["d"], rb["d"]) and ra["bits"] == rb["bits"], (vid, q, ra["thr"])
        assert ra["stream_id"] == rb["stream_id"] == (0, 1).index(vid) * 2 + (3, 4).index(q)
        assert np.array_equal(ra["x"], rb["x"]), (vid, q, ra["thr"])


def test_invariant_mode_sharing_gives_the_same_bits_for_fewer_samples(invariant_pair):
    plain, shared = invariant_pair
    seen = set()
    for _, _, r in plain.sent:
        assert r["invariant"]
        seen |= kinds_of(r["segments"])
    assert seen == {"partial", "fallback", "clip-end"}, seen
    assert_same_jobs(plain.sent, shared.sent)
    print(f"sample-rounds: {plain.samples} generated per job, {shared.samples} generated per state")
    print("states per round:     ", shared.stats["states"])
    print("job-rounds per round: ", shared.stats["jobs_served"])
    print("launch sizes shared:  ", sorted(shared.stats["launch_sizes"].items()))
    assert plain.stats["states"] == plain.stats["jobs_served"] == shared.stats["jobs_served"]
    assert plain.samples == sum(plain.stats["jobs_served"]) and shared.samples == sum(shared.stats["states"])
    assert shared.samples < plain.samples


def test_two_accept_all_and_two_reject_all_jobs_halve_every_round(world):
    """Two accept-all and two reject-all jobs per (video, q): from the round in which they part, the states are exactly half of
    the jobs served.  The first round is the exception the state definition itself makes: all four thresholds of a (video, q)
    still hold the same two key frames, so that round has ONE state per (video, q), 4 for 16 jobs (measured: states
    [4, 8, 8, ...] against jobs served [16, 16, 16, ...]); generating 8 there would be work beyond the distinct states."""
    run = sweep(world, [-100.0, -99.0, 200.0, 201.0], batch_invariant=True, share=True)
    st = run.stats
    print("states per round:     ", st["states"])
    print("job-rounds per round: ", st["jobs_served"])
    assert len(st["states"]) == len(st["jobs_served"]) > 1
    assert st["states"][0] == 4 and st["jobs_served"][0] == 16
    assert all(2 * s == j for s, j in zip(st["states"][1:], st["jobs_served"][1:])), (st["states"], st["jobs_served"])
    for g in range(4):
        a, b, c, d = (r for _, _, r in run.sent[4 * g:4 * g + 4])
        assert a["segments"] == b["segments"] == [("key", 2)] + [("gen", 5)] * 5 + [("gen", 3)]
        assert c["segments"] == d["segments"] == [("key", 2)] * 15
        assert np.array_equal(a["x"], b["x"]) and np.array_equal(c["x"], d["x"])


def test_receivers_reproduce_the_shared_sender_and_share_too(world, L, invariant_pair):  # noqa: F811
    from evc_amd import container
    _, shared = invariant_pair
    jobs = [stream4_of(r, vid, q, world, L) for vid, q, r in shared.sent]
    samples = {}
    for mb in (1, 32):
        for share in (False, True):
            stats = {}
            out = world.dec.decode_jobs(jobs, max_batch=mb, models=world.models, share=share, stats=stats)
            for (vid, q, r), job, x in zip(shared.sent, jobs, out):
                x = x.cpu().numpy()
                assert np.array_equal(x, r["x"]), (mb, share, vid, q, r["thr"])
                assert container.frames_crc(x) == job["crc"]
            samples[(mb, share)] = stats["samples"]
            assert stats["samples"] == sum(k * n for k, n in stats["launch_sizes"].items())
            assert max(stats["launch_sizes"]) <= mb
    print("receiver samples generated (max_batch, share):", samples)
    for mb in (1, 32):
        assert samples[(mb, False)] == sum(1 for _, _, r in shared.sent for k, _ in r["segments"] if k == "gen")
        assert samples[(mb, True)] < samples[(mb, False)]


def test_default_mode_shared_sender_through_the_receiver(world, grid):
    """The shared sweep WITHOUT batch-invariant generation, packed as format 3 and decoded one job per launch and 32 per
    launch: launches of other shapes differ in the last bits, every frame stays >= 60 dB against the
    sender's (the unshared form of this comparison measured 73.3 / 73.4 dB: profiles/NOTES.md), all-key jobs are identical."""
    run = sweep(world, grid, share=True)
    assert run.samples < sum(run.stats["jobs_served"])
    jobs = [stream3_of(r, vid, q, world) for vid, q, r in run.sent]
    for mb in (1, 32):
        out = world.dec.decode_jobs(jobs, max_batch=mb, models=world.models, share=False)
        worst = float("inf")
        for (vid, q, r), x in zip(run.sent, out):
            x = x.cpu().numpy()
            if all(k == "key" for k, _ in r["segments"]):
                assert np.array_equal(x, r["x"]), (mb, vid, q, r["thr"])
            worst = min(worst, min(psnr(x[t], r["x"][t]) for t in range(30)))
        print(f"default mode, shared sender, receiver batch {mb}: minimum over all frames of all jobs {worst:.1f} dB")
        assert worst >= 60.0, (mb, worst)


def test_share_generations_on_the_command_lines(tmp_path, L):  # noqa: F811
    """Fresh child processes, one at a time, each under its own time limit; the first non-zero status ends the test."""
    from evc_amd import container
    out, bits = tmp_path / "out", tmp_path / "bits"
    model = ["--config", os.path.join(REPO, "configs", "mine.yml"), "--synthetic", "--exp", str(tmp_path / "exp"),
             "--config_mod", "model.ngf=32 model.n_head_channels=32", "--data_npy", "missing.npy"]
    thresholds = [200.0, 6.91, -100.0, -101.0]
    send = [sys.executable, os.path.join(REPO, "city_sender.py")] + model + [
        "--output_path", str(out), "--start_idx", "0", "--end_idx", "0", "--subsample", "2", "--q", "3", "--bpp-limit", "1e9",
        "--share-generations"]
    bad = subprocess.run(send + ["--policy", "mask"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "--share-generations applies to the psnr / lpips policy" in bad.stderr, bad.stdout + bad.stderr
    s = subprocess.run(send + ["--policy", "psnr", "--thresholds"] + [str(t) for t in thresholds] +
                       ["--batch-invariant", "--bitstream-dir", str(bits)], cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert s.returncode == 0, s.stdout + s.stderr
    line = [ln for ln in s.stdout.splitlines() if "sample-rounds generated for" in ln]
    assert len(line) == 1 and "job-rounds served" in line[0], s.stdout
    print(line[0])
    names = [container.job_file_name(0, 3, t) for t in thresholds]
    assert sorted(os.listdir(bits)) == sorted(names)
    for n in names:
        job = container.unpack_job((bits / n).read_bytes())
        assert job["format"] == 4 and job["stream_id"] == 0
    recv = [sys.executable, os.path.join(REPO, "city_receiver.py")] + model + ["--bitstream-dir", str(bits)]
    for extra in (["--batch", "1"], ["--batch", "32", "--share-generations"]):
        rx = tmp_path / ("rx" + extra[1])
        r = subprocess.run(recv + ["--output_path", str(rx)] + extra, cwd=tmp_path, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.count("frames: match") == 4 and "MISMATCH" not in r.stdout, r.stdout
        assert ("sample-rounds generated for" in r.stdout) == (len(extra) == 3), r.stdout
        for t in thresholds:
            x = np.load(rx / ("decoded_v0_q3_thr%.2f.npy" % t))
            assert container.frames_crc(x) == container.unpack_job((bits / container.job_file_name(0, 3, t)).read_bytes())["crc"]
