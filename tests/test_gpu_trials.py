"""GPU tests of noise trials: the per-frame squared-error kernel (csrc/metric.hip), ``PsnrDeviceMetric``, the sweep with K = 3
draws per round on the reduced network of tests/test_gpu_batch_invariant.py (DDPM-2, ngf 32), its format-5 / format-6 streams
through the receiver, and the command lines.  The host side is tests/test_trials_host.py.

The sweeps are 2 clips x q {3} x thresholds [-100, 200] + four of ``threshold_grid``: 12 jobs."""
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from test_gpu_batch_invariant import L, psnr, world  # noqa: F401  (fixtures: the library, the reduced world)
from test_trials_host import consistent_choice, gen_segments

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 3
SEED = 5


@pytest.fixture(autouse=True)
def no_range_events(L):  # noqa: F811
    """No test of this module may raise an fp16-split range event."""
    L.range_events(reset=True)
    yield
    assert L.range_events() == 0


# ---- the kernel ------------------------------------------------------------------------------------------------

def frames_pair(n, elems, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 1, (n, elems)).astype(np.float32)
    b = (a + rng.normal(0, 0.05, (n, elems))).astype(np.float32)
    return a, b


def exact(a, b):
    """Per frame: math.fsum of the float64 squares."""
    d = a.astype(np.float64) - b.astype(np.float64)
    return np.asarray([math.fsum((row * row).tolist()) for row in d])


@pytest.mark.parametrize("elems", [1, 5, 1023, 4099, 49152])
def test_frame_sqerr_against_fsum(L, elems):  # noqa: F811
    """|dev - ref| <= (elems + 4) 2^-53 ref: one rounding for the difference, one for the square and elems - 1 for any summation
    order of non-negative terms, and the same again for the reference's squares.  n = 3: odd sizes put rows 1 and 2 off a
    16-byte boundary."""
    a, b = frames_pair(3, elems, 100 + elems)
    ref = exact(a, b)
    dev = L.frame_sqerr(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    assert dev.dtype == torch.float64 and dev.shape == (3,)
    dev = dev.cpu().numpy()
    err = np.abs(dev - ref)
    bound = (elems + 4) * 2.0 ** -53 * ref
    print(f"elems {elems}: relative error {(err / ref).max():.3e}, bound {(elems + 4) * 2.0 ** -53:.3e}")
    assert (ref > 0).all() and (err <= bound).all(), (elems, err / ref)


@pytest.mark.parametrize("elems", [1, 5, 1023, 4099, 49152])
def test_a_frames_value_does_not_depend_on_the_launch(L, elems):  # noqa: F811
    """Alone, at row 0 and at row 6 of a launch of 7, twice, and from a buffer that starts off a 16-byte boundary: one bit
    pattern.  For odd sizes row 6 (and the shifted buffer) is fetched with 4-byte loads, row 0 with 16-byte loads."""
    a, b = frames_pair(7, elems, 200 + elems)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    alone = L.frame_sqerr(ta[3:4].contiguous(), tb[3:4].contiguous())
    for row in (0, 6):
        pa, pb = ta.clone(), tb.clone()
        pa[row], pb[row] = ta[3], tb[3]
        first = L.frame_sqerr(pa, pb)
        again = L.frame_sqerr(pa, pb)
        assert torch.equal(first, again)
        assert torch.equal(first[row:row + 1], alone), (elems, row)
        mask = torch.ones(7, dtype=torch.bool)
        mask[row] = False
        assert torch.equal(first.cpu()[mask], L.frame_sqerr(ta, tb).cpu()[mask])          # the other rows are untouched
    for shift_a, shift_b in ((1, 0), (0, 3), (2, 2)):
        fa = torch.zeros(elems + 4, device="cuda")
        fb = torch.zeros(elems + 4, device="cuda")
        fa[shift_a:shift_a + elems], fb[shift_b:shift_b + elems] = ta[3], tb[3]
        va, vb = fa[shift_a:shift_a + elems].view(1, elems), fb[shift_b:shift_b + elems].view(1, elems)
        assert va.is_contiguous() and va.data_ptr() % 16 == (4 * shift_a) % 16
        assert torch.equal(L.frame_sqerr(va, vb), alone), (elems, shift_a, shift_b)


def test_frame_sqerr_non_finite_values_and_bad_arguments(L):  # noqa: F811
    elems = 4099
    a, b = frames_pair(8, elems, 9)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    a[0, 17] = nan                                   # NaN -> NaN
    a[1, 4098] = inf; b[1, 4098] = inf               # noqa: E702  inf - inf -> NaN
    a[2, 5] = inf                                    # inf against a finite value -> inf
    b[3, 4097] = -inf                                # ... on the other side, in the short last chunk
    a[4, 0] = inf; b[4, 0] = -inf                    # noqa: E702  inf - (-inf) = inf
    a[5, 1] = inf; b[5, 4000] = nan                  # noqa: E702  inf and NaN in one frame -> NaN
    with np.errstate(invalid="ignore", over="ignore"):
        want = np.sum((a.astype(np.float64) - b.astype(np.float64)) ** 2, axis=1)
    assert np.isnan(want[[0, 1, 5]]).all() and np.isposinf(want[[2, 3, 4]]).all() and np.isfinite(want[6:]).all()
    dev = L.frame_sqerr(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()).cpu().numpy()
    assert np.array_equal(np.isnan(dev), np.isnan(want)) and np.array_equal(np.isposinf(dev), np.isposinf(want))
    clean = L.frame_sqerr(torch.from_numpy(a[6:]).cuda(), torch.from_numpy(b[6:]).cuda()).cpu().numpy()
    assert np.array_equal(dev[6:], clean)            # other frames are unaffected, bit for bit
    # the library refuses before any launch
    lib = L.hip_lib()
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    out = torch.full((8,), -1.0, device="cuda", dtype=torch.float64)
    pa, pb, po, st = L.ptr(ta), L.ptr(tb), L.ptr(out), L.stream_ptr()
    assert lib.evc_frame_sqerr_f64(pa, pb, 0, elems, po, st) == -1
    assert lib.evc_frame_sqerr_f64(pa, pb, -1, elems, po, st) == -1
    assert lib.evc_frame_sqerr_f64(pa, pb, 8, 0, po, st) == -1
    assert lib.evc_frame_sqerr_f64(None, pb, 8, elems, po, st) == -1
    assert lib.evc_frame_sqerr_f64(pa, None, 8, elems, po, st) == -1
    assert lib.evc_frame_sqerr_f64(pa, pb, 8, elems, None, st) == -1
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())


def test_device_psnr_equals_cal_psnr(world):  # noqa: F811
    """10 frames of the world's clips: both mean squared errors carry at most elems 2^-53 = 5.5e-12 relative error, and
    10 / ln 10 times their sum is below 5e-11 dB; the bar is 1e-10 dB."""
    from evc_amd import policy as P
    pred, gt = world.clips[0][:10].cuda(), world.clips[1][:10].cuda()
    dev = P.PsnrDeviceMetric().values(pred, gt)
    host = P.PsnrMetric().values(pred, gt)
    want = np.asarray([P.cal_psnr(world.clips[0][i].numpy(), world.clips[1][i].numpy()) for i in range(10)])
    assert dev.dtype == np.float64 and dev.shape == (10,) and np.array_equal(host, want)
    print("device PSNR - cal_psnr (dB):", np.abs(dev - want).max())
    assert np.abs(dev - want).max() <= 1e-10
    same = P.PsnrDeviceMetric().values(pred[:1], pred[:1])
    assert np.isposinf(same).all()                  # identical frames: inf, as cal_psnr


# ---- the sweeps ------------------------------------------------------------------------------------------------

def jobs_of(res):
    return [(vid, q, r) for (vid, q), lst in res.items() for r in lst]


def first_round(r):
    return r["segments"][1][1] if r["segments"][1][0] == "gen" else 0


def stream_of(r, vid, q, world, L):  # noqa: F811
    from evc_amd import container
    extra = {}
    if r["invariant"]:
        extra = dict(plan=(container.PLAN_INVARIANT, L.invariant_plan_revision()), crc=container.frames_crc(r["x"]))
    blob = container.pack_job(r["segments"], r["key_strings"], r["shape"], world.models[q].codec_tag(), r["seed"],
                              r["stream_id"], vid, q, r["thr"], "DDPM", world.cfg.sampling.subsample, world.cfg.sampling.denoise,
                              trials=r["trials"], n_trials=r["n_trials"], **extra)
    return blob, container.unpack_job(blob, expect_codec=world.models[q].codec_tag(),
                                      expect_plan_revision=L.invariant_plan_revision())


@pytest.fixture(scope="module")
def sweeps(world, L):  # noqa: F811
    from evc_amd import policy as P
    from test_gpu_job_stream import threshold_grid
    thr = [-100.0, 200.0] + threshold_grid(world)[::3]
    assert len(thr) == 6

    def run(metric=None, **kw):
        stats = {}
        res = P.run_policy(world.dec, world.models, world.clips, [3], thr, metric or P.PsnrDeviceMetric(), max_batch=32,
                           seed=SEED, bpp_limit=1e9, noise="evc", noise_streams="group", stats=stats, **kw)
        return types.SimpleNamespace(res=res, stats=stats, sent=jobs_of(res))
    s = types.SimpleNamespace(P=P, thr=thr, run=run)
    s.today = run(metric=P.PsnrMetric(), batch_invariant=True)                     # the call as it was: no ``trials``
    s.k3 = run(batch_invariant=True, trials=K)
    return s


def samples(stats):
    return sum(n * c for n, c in stats["launch_sizes"].items())


def test_one_trial_is_todays_sweep_and_todays_bytes(sweeps, world, L):  # noqa: F811
    """``trials=1`` -- on the host metric and on the device metric -- against the call without the argument."""
    from evc_amd import container
    for metric in (sweeps.P.PsnrMetric(), sweeps.P.PsnrDeviceMetric()):
        one = sweeps.run(metric=metric, batch_invariant=True, trials=1)
        assert len(one.sent) == len(sweeps.today.sent) == 12
        assert one.stats["launch_sizes"] == sweeps.today.stats["launch_sizes"]
        for (vid, q, a), (_, _, b) in zip(sweeps.today.sent, one.sent):
            assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["d"], b["d"])
            assert a["bits"] == b["bits"] and a["bpp"] == b["bpp"] and a["segments"] == b["segments"]
            assert b["n_trials"] == 1 and b["trial_bits"] == 0 and not any(b["trials"])
            old = container.pack_job(a["segments"], a["key_strings"], a["shape"], world.models[q].codec_tag(), a["seed"],
                                     a["stream_id"], vid, q, a["thr"], "DDPM", 2, True,
                                     plan=(container.PLAN_INVARIANT, L.invariant_plan_revision()), crc=container.frames_crc(a["x"]))
            new, job = stream_of(b, vid, q, world, L)
            assert new == old and job["format"] == 4


def test_three_trials_batch_invariant(sweeps):
    P, k3 = sweeps.P, sweeps.k3
    assert len(k3.sent) == 12 and all(r["n_trials"] == K and r["invariant"] for _, _, r in k3.sent)
    assert all(n % K == 0 and n <= 30 for n in k3.stats["launch_sizes"])
    for prefixes, chosen in k3.stats["trial_prefixes"]:
        assert len(prefixes) == K
        consistent_choice(P, prefixes, chosen)
    assert sum(1 for _, c in k3.stats["trial_prefixes"] if c is not None) == sum(gen_segments(r) for _, _, r in k3.sent)
    # trial 0 is today's draw from today's frames, so the first round can only gain
    firsts = [(first_round(a), first_round(b)) for (_, _, a), (_, _, b) in zip(sweeps.today.sent, k3.sent)]
    print("first-round accepted frames (K = 1, K = 3):", firsts)
    assert all(b >= a for a, b in firsts)
    for _, _, r in k3.sent:
        assert r["trial_bits"] == 2 * gen_segments(r) and r["bpp"] == (sum(r["bits"]) + r["trial_bits"]) / 128 / 128 / 30
        assert all(t == 0 for (k, _), t in zip(r["segments"], r["trials"]) if k == "key")
    used = sorted({t for _, _, r in k3.sent for (k, _), t in zip(r["segments"], r["trials"]) if k == "gen"})
    print("trials chosen in the sweep:", used, " key frames (K = 1, K = 3):",
          sum(int(r["d"].sum()) for _, _, r in sweeps.today.sent), sum(int(r["d"].sum()) for _, _, r in k3.sent))
    assert any(used), "trial 0 won every round of the sweep: change the sweep's seed"
    # shared rounds: the same jobs, bit for bit, from fewer samples
    sh = sweeps.run(batch_invariant=True, trials=K, share=True)
    for (_, _, a), (_, _, b) in zip(k3.sent, sh.sent):
        assert np.array_equal(a["x"], b["x"]) and a["segments"] == b["segments"] and a["trials"] == b["trials"]
        assert a["bits"] == b["bits"] and a["bpp"] == b["bpp"] and a["key_strings"] == b["key_strings"]
    print("samples generated, unshared / shared:", samples(k3.stats), samples(sh.stats))
    assert samples(sh.stats) < samples(k3.stats) == K * sum(k3.stats["jobs_served"])


def test_receiver_reproduces_the_chosen_draws(sweeps, world, L):  # noqa: F811
    """Format-6 streams at 1 and 32 jobs per launch, shared or not: the sender's frames, one sample per generated segment."""
    from evc_amd import container
    packed = [stream_of(r, vid, q, world, L) for vid, q, r in sweeps.k3.sent]
    assert all(blob[4] == 6 and job["format"] == 6 and job["n_trials"] == K for blob, job in packed)
    jobs = [job for _, job in packed]
    gens = sum(gen_segments(r) for _, _, r in sweeps.k3.sent)
    for share in (False, True):
        for mb in (1, 32):
            stats = {}
            out = world.dec.decode_jobs(jobs, max_batch=mb, models=world.models, share=share, stats=stats)
            for (vid, q, r), job, x in zip(sweeps.k3.sent, jobs, out):
                x = x.cpu().numpy()
                assert np.array_equal(x, r["x"]), (share, mb, vid, r["thr"])
                assert container.frames_crc(x) == job["crc"]
            assert stats["job_rounds"] == gens
            assert stats["samples"] == gens if not share else stats["samples"] < gens


def test_default_mode_streams_stay_within_the_projects_bar(sweeps, world, L):  # noqa: F811
    """Format-5 streams (default generation mode) decoded at 1 and 32 jobs per launch: every frame >= 60 dB against the
    sender's (the bar of test_batched_sender_any_receiver_batch)."""
    run = sweeps.run(trials=K)
    packed = [stream_of(r, vid, q, world, L) for vid, q, r in run.sent]
    assert all(blob[4] == 5 and job["crc"] is None for blob, job in packed)
    for mb in (1, 32):
        out = world.dec.decode_jobs([job for _, job in packed], max_batch=mb, models=world.models)
        worst = float("inf")
        for (vid, q, r), x in zip(run.sent, out):
            x = x.cpu().numpy()
            worst = min(worst, min(psnr(x[t], r["x"][t]) for t in range(30)))
        print(f"receiver batch {mb}: minimum over all frames {worst:.1f} dB")
        assert worst >= 60.0, (mb, worst)


# ---- the command lines -----------------------------------------------------------------------------------------

def test_sender_with_trials_then_receiver_in_fresh_processes(tmp_path):
    from evc_amd import container
    out, bits = tmp_path / "out", tmp_path / "bits"
    model = ["--config", os.path.join(REPO, "configs", "mine.yml"), "--synthetic", "--exp", str(tmp_path / "exp"),
             "--config_mod", "model.ngf=32 model.n_head_channels=32", "--data_npy", "missing.npy"]
    thresholds = [200.0, 6.91, -100.0]
    send = [sys.executable, os.path.join(REPO, "city_sender.py")] + model + [
        "--output_path", str(out), "--start_idx", "0", "--end_idx", "0", "--subsample", "2", "--q", "3", "--policy", "psnr",
        "--thresholds"] + [str(t) for t in thresholds] + ["--bpp-limit", "1e9", "--bitstream-dir", str(bits),
                                                          "--noise-trials", "3", "--batch-invariant"]
    bad = subprocess.run(send + ["--noise", "torch"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "--noise" in bad.stderr and not bits.exists() and not out.exists()
    s = subprocess.run(send, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert s.returncode == 0, s.stdout + s.stderr
    assert "noise: evc" in s.stdout and s.stdout.count(" trials 3 (+") == 3, s.stdout
    names = [container.job_file_name(0, 3, t) for t in thresholds]
    assert sorted(os.listdir(bits)) == sorted(names)
    bpp = np.load(out / "output_0" / "bpp_0.npy")
    for i, (n, t) in enumerate(zip(names, thresholds)):
        job = container.unpack_job((bits / n).read_bytes())
        assert job["format"] == 6 and job["n_trials"] == 3
        side = 2 * sum(1 for k, _ in job["segments"] if k == "gen")
        assert f" trials 3 (+{side} bits)" in s.stdout
        assert container.payload_bits(job["key_strings"]) + side == round(float(bpp[i]) * 128 * 128 * 30)
    r = subprocess.run([sys.executable, os.path.join(REPO, "city_receiver.py")] + model +
                       ["--bitstream-dir", str(bits), "--output_path", str(tmp_path / "rx")], cwd=tmp_path,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("frames: match") == 3 and "MISMATCH" not in r.stdout, r.stdout
