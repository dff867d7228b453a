"""Sender policy: which frames are transmitted as ELIC key frames and which are left to the generator.

Restates ``SenderCity.update`` / ``decide_5to5`` / ``decide_5to5_lpips`` and the sweep of the reference's main loop
(city_sender.py:353-437, 495-607): per (video, q, threshold) job, starting from two key frames, generate 5 frames
from the last two decoded ones, keep the longest prefix whose quality metric passes the threshold, and when not a
single frame passes, key-code the next two frames instead.  The reference runs the jobs strictly one after another
(1 video x 2 q x 28 thresholds, a fresh sampler + checkpoint reload per job); they are independent, so here ALL
active jobs -- every (video, q, threshold) -- advance in lockstep: each round stacks their conditioning frames along
the batch axis of one score-network launch (``max_batch`` per launch), and the key frames a round needs are coded in
one batched ELIC call per q, once per (video, q, frame) however many thresholds fall back to it.

Noise: every job draws from its own counter-based stream (seed, job id, round, step), so a job's frames do not depend
on which other jobs share its launch -- the batched sweep and a one-job-at-a-time run make the same decisions.  With
``noise="evc"`` the stream is the project's own specification N1 (csrc/noise.hip) keyed by (seed, job id, start frame, step),
which a receiver can derive from the job stream alone; the result then carries the job's program (``segments``) and key-frame
strings, everything ``container.pack_job`` needs.

Shared rounds (``noise_streams="group", share=True``): all thresholds of one (video, q) then draw from ONE stream, so two jobs
that hold the same frames would generate the same chunk; ``StateGrouper`` finds them by the identity of their last two frames
and each round generates once per distinct state instead of once per job.

Noise trials (``trials=K``, noise="evc"): the sender knows the original, so it draws every round K times -- trial t keys N1 with
start frame + 65536 t, trial 0 is the plain key -- in the same launches, and each job keeps the draw ``choose_trial`` prefers
under its own threshold: the longest accepted prefix, then the better mean, then the lowest trial.  The job's program names the
trial of every generated segment (container formats 5 / 6) for ceil(log2 K) bits, which ``bpp`` includes; a receiver generates
the chosen draw only.  ``PsnrDeviceMetric`` judges the K-fold candidates where they are (csrc/metric.hip).

Metrics: ``PsnrMetric`` is the reference's ``decide_5to5`` rule (accept while PSNR >= threshold, cal_psnr of
city_sender.py:257-260).  ``CallableMetric`` is the hook for ``decide_5to5_lpips`` (accept while distance <=
threshold): LPIPS needs torchvision's pretrained AlexNet, which cannot be fetched offline, so the metric is supplied
by the user (``--policy lpips --metric pkg.module:function`` or the ``lpips`` package when it is importable).
"""
import functools
import importlib
import os
import time

import numpy as np
import torch

from . import lib as L
from .elic import coded_batch, estimated_batch  # noqa: F401  (the sweep's key-frame calls; importable from here as before)
from .report import cal_psnr


class PsnrMetric:
    """decide_5to5 (city_sender.py:353-374): a generated frame is kept while PSNR(pred, gt) >= threshold."""
    name = "psnr"

    def values(self, pred, gt):
        p, g = pred.detach().cpu().numpy(), gt.detach().cpu().numpy()
        return np.asarray([cal_psnr(p[i], g[i]) for i in range(p.shape[0])])

    @staticmethod
    def accept(value, thr):
        return value >= thr

    @staticmethod
    def better(a, b):
        """Whether value a is strictly better than b: the higher PSNR."""
        return a > b


class PsnrDeviceMetric(PsnrMetric):
    """PsnrMetric with the sum on the device: ``lib.frame_sqerr`` (csrc/metric.hip) adds every frame's squared error in
    float64 and n doubles come back instead of the frames; 10 log10(1 / mse) is formed on the host in float64.  The sweep with
    noise trials judges K times the candidates and uses this class; ``PsnrMetric`` stays the default."""

    def values(self, pred, gt):
        pred, gt = pred.detach().float().contiguous(), gt.detach().float().contiguous()
        sums = L.frame_sqerr(pred, gt).cpu().numpy()
        with np.errstate(divide="ignore"):          # identical frames: 10 log10(1 / 0) = inf, as cal_psnr
            return 10 * np.log10(1.0 / (sums / (pred.numel() // pred.shape[0])))


class CallableMetric:
    """decide_5to5_lpips (city_sender.py:376-406): kept while distance(pred, gt) <= threshold.  ``fn(pred, gt)`` takes
    two (n, 3, H, W) float tensors in [0, 1] on the device and returns n distances."""
    name = "lpips"

    def __init__(self, fn, name="lpips"):
        self.fn, self.name = fn, name

    def values(self, pred, gt):
        v = self.fn(pred.float(), gt.float())
        return np.asarray(v.detach().cpu().reshape(-1).tolist() if torch.is_tensor(v) else v, dtype=np.float64)

    @staticmethod
    def accept(value, thr):
        return value <= thr

    @staticmethod
    def better(a, b):
        """Whether value a is strictly better than b: the smaller distance."""
        return a < b


def load_metric(policy, spec=None, device="cuda", net="alex"):
    """``psnr`` -> PsnrMetric; ``lpips`` -> the HIP LPIPS-AlexNet (``lpips.LpipsAlex``) when ``spec`` names its weight files
    ("alexnet.pth,alex.pth" or one saved LPIPS state dict), else a CallableMetric around ``spec`` = "package.module:callable"
    (called as fn(pred, gt)), or around the ``lpips`` package (LPIPS(net='alex'), inputs scaled to [-1, 1] as lpips expects --
    the reference feeds [0, 1] frames unnormalised, city_sender.py:389-390; pass your own callable to reproduce that).
    ``net`` = "vgg" / "squeeze" (``--lpips-net``): the weight files are that backbone's, and the rule runs on ``lpips.Lpips``."""
    if policy == "psnr":
        return PsnrMetric()
    if policy != "lpips":
        raise ValueError(f"unknown policy metric {policy!r}")
    if spec and (spec.startswith("file:") or all(os.path.isfile(part) for part in spec.split(","))):
        spec = spec[5:] if spec.startswith("file:") else spec
        # weight files: "alexnet-owt-*.pth,alex.pth" (torchvision backbone + lpips v0.1 linear layers) or one file holding
        # a saved lpips.LPIPS state dict -> the HIP implementation (lpips.py); frames are passed as they are, like the reference
        from .lpips import NETS, Lpips, LpipsAlex
        if net not in NETS:
            raise ValueError(f"unknown LPIPS network {net!r}: one of {', '.join(NETS)}")
        if net != "alex":
            other = Lpips.from_spec(spec, net, device)
            return CallableMetric(lambda a, b: other(a, b), name=f"lpips-{net}-hip")
        paths = spec.split(",")
        net = (LpipsAlex.from_files(paths[0], paths[1], device) if len(paths) == 2 else
               LpipsAlex(torch.load(paths[0], map_location="cpu", weights_only=True), device))
        return CallableMetric(lambda a, b: net(a, b), name="lpips-alex-hip")
    if spec:
        mod, _, attr = spec.partition(":")
        fn = getattr(importlib.import_module(mod), attr or "metric")
        return CallableMetric(fn, name=spec)
    try:
        import lpips  # noqa: F401  (needs torchvision's pretrained AlexNet: not available offline)
    except Exception as e:
        raise RuntimeError("--policy lpips needs a perceptual metric: the `lpips` package (with torchvision's pretrained "
                           "AlexNet) is not importable here; pass --metric package.module:callable "
                           "(fn(pred, gt) -> distances for (n,3,H,W) tensors in [0,1]) or use --policy psnr") from e
    net = lpips.LPIPS(net="alex").to(device).eval()
    return CallableMetric(lambda a, b: net(a, b).reshape(-1), name="lpips-alex")


class _Job:
    __slots__ = ("uid", "sid", "vid", "q", "thr", "x", "ids", "d", "bits", "round", "segments", "strings", "trials")

    def __init__(self, uid, vid, q, thr, sid=None):
        self.uid, self.vid, self.q, self.thr = uid, vid, q, thr
        self.sid = uid if sid is None else sid          # id of the noise stream the job draws from
        self.x, self.d, self.bits, self.round = [], [], [], 0
        self.ids = []                                   # identity of every frame of ``x`` (StateGrouper)
        self.segments, self.strings = [], []
        self.trials = []                                # per segment: the noise trial a gen segment was drawn with, 0 for key


def key_id(vid, q, f):
    """Identity of the decoded key frame f of (video, q): the sweep holds it once (``key_cache``)."""
    return ("key", vid, q, f)


def gen_id(serial, t, trial=0):
    """Identity of frame t of the chunk generated, under noise trial ``trial``, for the state with that serial number."""
    return ("gen", serial, t, trial)


class StateGrouper:
    """Which jobs of a round would generate the same chunk (host only; never looks at pixel data).

    Under group noise streams a generation round is a function of (video, q, frames held, last two decoded frames): the
    conditioning pair, the noise key (seed, group id, start frame = frames held, step) and the originals the candidates
    are judged against.  Frames are compared by identity, ``key_id`` / ``gen_id``: two jobs hold the same generated frame
    only when they were members of the same state in the round that made it, and the same key frame whenever they fell
    back at the same frame index.  ``group`` numbers every state it returns with a serial of its own, which names the
    frames generated for it."""

    def __init__(self):
        self.serial = 0

    @staticmethod
    def state_of(job):
        return (job.vid, job.q, len(job.ids), job.ids[-1], job.ids[-2])

    def group(self, jobs, share=True, state=None):
        """jobs: the round's active jobs -> [(serial, [member jobs])], states in the order of their first member, members in the
        order given.  ``state``: job -> its state, a hashable (default ``state_of``, the sender's: ``vid``, ``q``, ``ids``; the
        receiver passes its own).  ``share=False``: every job is a state of its own."""
        state = self.state_of if state is None else state
        states, at = [], {}
        for j in jobs:
            k = state(j) if share else id(j)
            if k not in at:
                at[k] = len(states)
                states.append((self.serial, []))
                self.serial += 1
            states[at[k]][1].append(j)
        return states


TRIAL_SHIFT = 16                   # noise trial t of a round: start frame + 65536 t in the N1 key (trial 0 = the plain key)
MAX_TRIALS = 255                   # a job stream names the trial in one byte


def trial_start(held, trial):
    """The start-frame word of the N1 key of noise trial ``trial`` of the round a job starts holding ``held`` frames."""
    return int(held) | int(trial) << TRIAL_SHIFT


def trial_bits(segments, n_trials):
    """Side information of the noise trials of one job: ceil(log2 K) bits per generated segment."""
    return sum(1 for kind, _ in segments if kind == "gen") * (int(n_trials) - 1).bit_length()


def choose_trial(values, thr, metric):
    """values[t][f]: the metric of candidate frame f under noise trial t; -> (trial, accepted).  a_t = the length of trial t's
    accepted prefix under ``thr``.  The largest a_t wins; among equals the better mean metric over those a_t frames
    (``metric.better``); among equals the lowest trial.  (None, 0) when no trial's first frame is accepted."""
    best, best_a, best_mean = None, 0, None
    for t, a in enumerate(accepted_prefixes(values, thr, metric)):
        if a == 0 or a < best_a:
            continue
        mean = float(np.mean(np.asarray(values[t][:a], dtype=np.float64)))
        if a > best_a or metric.better(mean, best_mean):
            best, best_a, best_mean = t, a, mean
    return best, best_a


def accepted_prefixes(values, thr, metric):
    """a_t of ``choose_trial`` for every trial: the frames accepted before the first one that is not."""
    out = []
    for row in values:
        a = 0
        while a < len(row) and metric.accept(row[a], thr):
            a += 1
        out.append(a)
    return out


def n1_noise(pairs, seed, device):
    """Noise specification N1 for one launch: pairs = per sample (stream id, start frame = frames held when the round starts;
    ``trial_start`` for a noise trial)
    -> ``noise_fn(tag, shape)`` of ``ClipDecoder.generate``.  The keys go up once; every step is one launch for the whole batch
    (step 0 = x_T, step i + 1 = the noise of sampler step i).  Sender and receiver both draw through here."""
    keys = L.noise_keys(pairs, device)
    return lambda tag, shape: L.noise_normal(keys, shape, seed, 0 if tag == "init" else int(tag) + 1)


def count_launch(stats, samples):
    """One generation launch more in ``stats["launch_sizes"]`` = {samples in a launch: launches} (``stats`` may be None)."""
    if stats is not None:
        h = stats.setdefault("launch_sizes", {})
        h[samples] = h.get(samples, 0) + 1


def in_launches(states, n):
    """A round's states (or whatever rides one per sample) in their order, cut into launches of at most n."""
    return [states[c0:c0 + n] for c0 in range(0, len(states), n)]


def generation_launch(decoder, samples, noise_fn, invariant, stats):
    """One generation launch, the sender's and the receiver's: ``samples`` holds one job per sample (anything with ``.x``; the sender
    repeats a state's head once per noise trial), whose last two frames are the conditioning pair.  -> (n, 5, 3, H, W)."""
    cond = torch.stack([torch.stack(j.x[-2:], 0) for j in samples], 0).contiguous()           # (n, 2, 3, H, W)
    pred = decoder.generate(cond, noise_fn=noise_fn, groups=1, invariant=invariant)
    count_launch(stats, len(samples))
    return pred


def torch_noise_seed(seed, sid, at, step):
    """The generator seed of ``noise="torch"``: (20 bits of seed, stream id, 6 bits of round / start frame, 10 bits of step)."""
    return ((((int(seed) & 0xFFFFF) << 20 | sid) << 6 | at) << 10 | step) & (2 ** 63 - 1)


def timed_noise(stats, fn, tag, shape):
    """``fn(tag, shape)``, its host time added to ``stats`` (launches are asynchronous: this is the CPU's share)."""
    t0 = time.perf_counter()
    out = fn(tag, shape)
    stats["noise_host_seconds"] = stats.get("noise_host_seconds", 0.0) + time.perf_counter() - t0
    return out


class _Sweep:
    """The steps of one ``run_policy`` call and what they share: the sender's side of ``decoder._JobRounds``."""

    def __init__(self, decoder, models, clips, qs, thresholds, metric, *, patch, frames, max_batch, seed, bpp_limit, device, log,
                 noise_source, stats, noise, batch_invariant, noise_streams, share, estimate, trials):
        self.decoder, self.models, self.clips, self.qs, self.metric = decoder, models, clips, qs, metric
        self.patch, self.frames, self.max_batch, self.seed, self.bpp_limit = patch, frames, max_batch, seed, bpp_limit
        self.device, self.log, self.noise_source, self.stats, self.noise = device, log, noise_source, stats, noise
        self.batch_invariant, self.noise_streams, self.share = batch_invariant, noise_streams, share
        self.estimate, self.trials = estimate, trials
        self.jobs, uid, gid = [], 0, 0
        for vid in clips:
            for q in qs:
                for thr in thresholds:
                    self.jobs.append(_Job(uid, vid, q, thr, sid=gid if noise_streams == "group" else None))
                    uid += 1
                gid += 1
        self.key_cache = {}             # (vid, q, frame) -> (x_hat on device, bits, strings)
        self.shapes = []                # hyper-latent shape of every ELIC call (all equal: one frame size)
        self.grouper = StateGrouper()

    def check(self):
        """The combinations of settings that mean nothing are refused before any work."""
        noise, noise_source, noise_streams = self.noise, self.noise_source, self.noise_streams
        if noise not in ("torch", "evc"):
            raise ValueError(f"noise must be 'torch' or 'evc', not {noise!r}")
        if self.batch_invariant and noise != "evc":
            raise ValueError("batch_invariant needs noise='evc': torch's generators are not replayable by a receiver, so there is "
                             "nobody to reproduce the frames")
        if noise_streams not in ("job", "group"):
            raise ValueError(f"noise_streams must be 'job' or 'group', not {noise_streams!r}")
        if noise_streams == "group" and noise_source is not None:
            raise ValueError("noise_streams='group' does not combine with noise_source, which is keyed per (job, round)")
        if self.share and noise_streams != "group":
            raise ValueError("share=True needs noise_streams='group': jobs that draw from streams of their own never generate "
                             "the same frames, so there is nothing to share")
        self.trials = trials = int(self.trials)
        if trials < 1:
            raise ValueError(f"trials must be >= 1, not {trials}")
        if trials > 1:
            if noise != "evc" or noise_source is not None:
                raise ValueError("trials > 1 needs noise='evc' and no noise_source: the receiver regenerates the chosen draw from the "
                                 "trial number alone, which only the keyed noise of specification N1 allows")
            if trials > self.max_batch:
                raise ValueError(f"trials = {trials} > max_batch = {self.max_batch}: the trials of a state ride in one launch, and "
                                 "max_batch counts samples")
            if trials > MAX_TRIALS:
                raise ValueError(f"trials = {trials} > {MAX_TRIALS}: a job stream names the trial in one byte")
        if self.batch_invariant:
            self.decoder._refuse_recovery()
        if noise == "evc" and noise_source is None:
            cfg = self.decoder.config
            if getattr(cfg.model, "gamma", False):
                raise NotImplementedError("noise='evc': noise specification N1 defines Gaussian noise only (config.model.gamma is set)")
            if float(getattr(cfg.sampling, "t_min", -1) or -1) > 0:
                raise NotImplementedError("noise='evc': noise specification N1 has no draw for a t_min > 0 start")

    def start(self):
        """The originals go to the device, and every job starts from its first two key frames (city_sender.py:521-524)."""
        self.gt_dev = {vid: c.to(device=self.device, dtype=torch.float32) for vid, c in self.clips.items()}
        self.size = next(iter(self.clips.values())).shape[-2:]
        self.key_round(self.jobs)

    def ensure_keys(self, wanted):
        """Code every missing (vid, q, frame) of ``wanted``: one batched ELIC encode + decode per q."""
        for q in self.qs:
            todo = sorted({k for k in wanted if k[1] == q and k not in self.key_cache})
            for part in in_launches(todo, self.max_batch):
                x = torch.stack([self.gt_dev[v][f] for (v, _, f) in part], 0)
                xh, bits, strings, shape = (estimated_batch if self.estimate else coded_batch)(self.models[q], x, self.patch)
                self.shapes.append(tuple(shape))
                for i, k in enumerate(part):
                    self.key_cache[k] = (xh[i], bits[i], None if strings is None else strings[i])

    def add_keys(self, job, fs):
        """The coded frames ``fs`` become the job's next segment, ("key", len(fs))."""
        for f in fs:
            xh, b, st = self.key_cache[(job.vid, job.q, f)]
            job.x.append(xh); job.bits.append(b); job.d.append(1); job.strings.append(st)
            job.ids.append(key_id(job.vid, job.q, f))
        if len(fs):
            job.segments.append(("key", len(fs)))
            job.trials.append(0)

    def key_round(self, jobs):
        """jobs: those that go on from key frames, in the order they were judged -- the next two frames of each (at the clip's end
        the one that is left; frames 0 and 1 of a job that holds none).  Coded in one call for all of them, then added job by job."""
        fs = [(0, 1) if not j.x else [f for f in (len(j.x), len(j.x) + 1) if f < self.frames] for j in jobs]
        self.ensure_keys({(j.vid, j.q, f) for j, mine in zip(jobs, fs) for f in mine})
        for j, mine in zip(jobs, fs):
            self.add_keys(j, mine)

    def drawn_noise(self, batch, tag, shape):
        """``noise_source``'s or torch's noise for one launch: one counter-based stream per (job, round, step) -- per (group, start
        frame, step) under group streams --: independent of the batch composition."""
        step = 0 if tag == "init" else int(tag) + 1
        out = torch.empty(shape, device=self.device, dtype=torch.float32)
        for i, (j, _) in enumerate(batch):
            if self.noise_source is not None:
                out[i] = self.noise_source((j.vid, j.q, j.thr), j.round, step, tuple(shape[1:])).to(self.device)
                continue
            g = torch.Generator(device=self.device)
            g.manual_seed(torch_noise_seed(self.seed, j.sid, len(j.x) if self.noise_streams == "group" else j.round, step))
            out[i] = torch.randn(shape[1:], device=self.device, dtype=torch.float32, generator=g)
        return out

    def noise_for(self, batch):
        """batch: per sample (job, noise trial) -> the ``noise_fn`` of its launch, timed when there are ``stats``."""
        if self.noise == "evc" and self.noise_source is None:
            fn = n1_noise([(j.sid, trial_start(len(j.x), t)) for j, t in batch], self.seed, self.device)
        else:
            fn = functools.partial(self.drawn_noise, batch)
        return fn if self.stats is None else functools.partial(timed_noise, self.stats, fn)

    def generation_round(self, states):
        """states: [(serial, members)] of the round.  max_batch counts samples: a state's K trials share its launch, sample
        k * K + t being state k under noise trial t.  -> the jobs that kept no frame, in the order they were judged."""
        fallback = []
        for part in in_launches(states, self.max_batch // self.trials):
            batch = [(members[0], t) for _, members in part for t in range(self.trials)]      # a state's members hold the same frames
            pred = generation_launch(self.decoder, [j for j, _ in batch], self.noise_for(batch),
                                     True if self.batch_invariant else None, self.stats)
            fallback += self.judge(pred, part)
        return fallback

    def judge(self, pred, part):
        """One launch's candidates ``pred`` for the states ``part``: the metric of every candidate frame in one call, then each
        member judges its state's [trial][frame] table by its own threshold.  -> the members that kept no frame."""
        K, heads = self.trials, [members[0] for _, members in part]
        n_new = [min(pred.shape[1], self.frames - len(j.x)) for j in heads]
        flat_p = torch.cat([pred[k * K + t, :n] for k, n in enumerate(n_new) for t in range(K)], 0)
        flat_g = torch.cat([self.gt_dev[j.vid][len(j.x):len(j.x) + n] for j, n in zip(heads, n_new) for t in range(K)], 0)
        vals = self.metric.values(flat_p, flat_g)
        fallback, o = [], 0
        for k, (serial, members) in enumerate(part):
            n = n_new[k]
            table = [vals[o + t * n:o + (t + 1) * n] for t in range(K)]
            o += n * K
            fallback += [j for j in members if not self.take(j, serial, pred[k * K:(k + 1) * K], table)]
        return fallback

    def take(self, j, serial, cands, table):
        """Job j keeps, of its state's candidates cands[trial][frame], the prefix ``choose_trial`` picks; -> the frames kept.  A
        rejected round leaves no segment."""
        trial, acc = choose_trial(table, j.thr, self.metric)
        for t in range(acc):
            j.x.append(cands[trial, t]); j.ids.append(gen_id(serial, t, trial)); j.d.append(0)
        j.round += 1
        if acc:
            j.segments.append(("gen", acc))
            j.trials.append(trial)
        if self.trials > 1 and self.stats is not None:
            self.stats.setdefault("trial_prefixes", []).append((tuple(accepted_prefixes(table, j.thr, self.metric)), trial))
        return acc

    def end_round(self, active, states, fallback):
        """The round's statistics and its log line."""
        stats = self.stats
        if stats is not None:
            stats["rounds"] = stats.get("rounds", 0) + 1
            stats["key_frames_coded"] = len(self.key_cache)
            stats.setdefault("states", []).append(len(states))
            stats.setdefault("jobs_served", []).append(len(active))
        if self.log is not None:
            self.log(f"policy round: {len(active)} active jobs" + (f" in {len(states)} states" if self.share else "") +
                     f", {len(fallback)} fell back to key frames")

    def results(self):
        """{(vid, q): [result dict per threshold]}, the thresholds of a (vid, q) cut at the first whose rate reaches ``bpp_limit``."""
        (H, W), frames, out = self.size, self.frames, {}
        for j in self.jobs:
            lst = out.setdefault((j.vid, j.q), [])
            if lst and lst[-1] is None:
                continue                                            # sweep of this (vid, q) already cut
            side = trial_bits(j.segments, self.trials)
            bpp = (sum(j.bits) + side) / H / W / frames
            if bpp >= self.bpp_limit:
                lst.append(None)
                continue
            lst.append(dict(thr=j.thr, x=torch.stack(j.x[:frames], 0).cpu().numpy(), d=np.asarray(j.d[:frames], dtype=np.int64),
                            bits=list(j.bits), bpp=bpp, segments=list(j.segments), stream_id=j.sid, seed=int(self.seed),
                            key_strings=list(j.strings), shape=self.shapes[0], invariant=bool(self.batch_invariant),
                            n_trials=self.trials, trials=list(j.trials), trial_bits=side))
        return {k: [r for r in v if r is not None] for k, v in out.items()}


def run_policy(decoder, models, clips, qs, thresholds, metric, patch=64, frames=30, max_batch=32, seed=0,
               bpp_limit=1.0, device="cuda", log=None, noise_source=None, stats=None, noise="torch", batch_invariant=False,
               noise_streams="job", share=False, estimate=False, trials=1):
    """The reference's sweep, batched.

    decoder:       ClipDecoder (only ``generate`` is used: the generator does not depend on q)
    models:        q -> ElicModel
    clips:         {vid: float tensor (frames, 3, H, W) in [0, 1]} (host)
    noise_source:  optional ``fn(job, round, step, shape) -> tensor`` (job = (vid, q, thr); step 0 = x_T, step i+1 = the
                   noise of sampler step i) replacing the per-job device generators -- parity tests inject the noise the
                   CPU oracle loop uses
    noise:         "torch" -- one seeded ``torch.Generator`` per (job, round, step) -- or "evc": noise specification N1
                   (DESIGN.md section 5), one ``evc_noise_normal_f32`` launch per step keyed by (seed, stream id = the job's
                   number, start frame = frames the job holds when the round starts, step).  Only "evc" can be replayed
                   by a receiver (container.pack_job / ClipDecoder.decode_jobs); ``noise_source`` wins over both
    batch_invariant: generate on the score network's batch-invariant view: a job's frames then do not
                   depend on the launches it rode in, so a receiver reproduces them bit for bit at any batch size
                   (container format 4).  Needs noise="evc", as job streams do; every result then carries ``invariant=True``
    noise_streams: "job" -- every job draws from a stream of its own (stream id = the job's number) -- or "group": the stream id
                   of a job is the index of its (video, q) pair in the sweep's order (video-major, then q), so all thresholds
                   of one (video, q) share a stream.  The key of a round is then (seed, group id, start frame, step), for
                   noise="torch" the generator seed mixes the same four; results carry ``stream_id`` = the group id, which is
                   all a receiver needs.  Within one job no key is used twice, as before (the start frame strictly
                   increases).  Two jobs of a group in different states at the same start frame draw the same noise for
                   different conditioning frames: the jobs of one (video, q) are correlated samples, which is harmless
                   because each job is reported on its own.  ``noise_source`` is keyed per (job, round) and does not combine
                   with "group" (ValueError)
    share:         generate once per distinct state instead of once per job (needs noise_streams="group").  Each round the
                   active jobs are grouped by (video, q, frames held, identity of the last two frames) -- ``StateGrouper`` --,
                   one conditioning pair per state is stacked (``max_batch`` states per launch), the metric is evaluated
                   once per candidate frame of a state, and every member applies its own threshold and keeps the same frame
                   tensors.  Jobs that diverge are in different states the next round; jobs that fall back to the same key
                   frames merge again.  With ``batch_invariant`` every job's frames are bitwise what share=False gives under
                   the same streams; in the default mode they differ in the last bits, as frames of launches of other
                   shapes do
    estimate:      key frames go through ``estimated_batch`` instead of ``coded_batch`` (--entropy-estimation): the same frames,
                   ``bits`` are float estimates and there are no strings (``key_strings`` holds None: such results cannot be
                   packed into job streams)
    trials:        K noise trials per round (needs noise="evc" without ``noise_source``, K <= max_batch, K <= 255).  Every state of
                   a round is generated K times in the same launches -- the conditioning pair repeated, trial t drawing the key
                   (seed, stream id, start frame + 65536 t, step), trial 0 today's key; ``max_batch`` counts samples, so a launch
                   holds max_batch // K states --, the metric is evaluated once per (state, trial, frame), and every member job
                   keeps the frames of the trial ``choose_trial`` picks under its own threshold.  The trial is part of a frame's
                   identity (``gen_id``), so under ``share`` two jobs are one state only if they kept the same trial's frames.
                   Results carry ``n_trials`` = K, ``trials`` (per segment: 0 for key, the chosen trial for gen) and
                   ``trial_bits`` = gen segments x ceil(log2 K), which ``bpp`` and the ``bpp_limit`` cut include;
                   ``stats["trial_prefixes"]`` lists per executed job-round (a_0 .. a_{K-1}, chosen).  K = 1 is the sweep as it
                   always was, bit for bit
    stats:         optional dict, filled with the launch-size histogram {samples (= states) in a launch: generation launches},
                   the number of generation rounds and of key frames coded, the host seconds spent drawing noise, and per
                   round the number of states generated (``states``) and of active jobs they served (``jobs_served``)
    Returns {(vid, q): [dict(thr, x (frames,3,H,W) float32 numpy, d (frames,) int, bits [..], bpp, segments, stream_id,
    seed, key_strings, shape, n_trials, trials, trial_bits)]} with, per (vid, q), the thresholds in the given order cut at the first one whose rate reaches
    ``bpp_limit`` bits per pixel (``if NN_bpp >= 1.0: break``, city_sender.py:563-564).  ``segments`` is the job's program in
    order: ("key", n) for n key frames decoded in one ELIC call (the initial pair, each fall-back pair, 1 at the clip's
    end), ("gen", n) for a round of which n >= 1 frames were kept (a rejected round leaves no frame and no entry: its noise
    key is never reused, because the fall-back moves the start frame on); ``key_strings`` the key frames' strings in order."""
    run = _Sweep(decoder, models, clips, qs, thresholds, metric, patch=patch, frames=frames, max_batch=max_batch, seed=seed,
                 bpp_limit=bpp_limit, device=device, log=log, noise_source=noise_source, stats=stats, noise=noise,
                 batch_invariant=batch_invariant, noise_streams=noise_streams, share=share, estimate=estimate, trials=trials)
    run.check()
    run.start()
    while True:
        active = [j for j in run.jobs if len(j.x) < frames]
        if not active:
            break
        states = run.grouper.group(active, share)            # [(serial, members)]: one generated sample per state and trial
        fallback = run.generation_round(states)
        run.key_round(fallback)                              # city_sender.py:538-548: key-code the next two frames
        run.end_round(active, states, fallback)
    return run.results()


def rd_envelope(bpp, metric_mean, higher_is_better):
    """The rate-distortion frontier of one video's sweep: the part of the convex hull of the (bpp, metric) points
    between the leftmost point and the best-metric point -- upper-left chain for PSNR, lower-left chain for LPIPS --
    which is what ``process_data_and_save`` keeps (function.py:148-204).  scipy's ConvexHull lists the vertices
    counter-clockwise from an arbitrary start; the reference slices that list with index arithmetic that is only
    right when the start happens to fall outside the chain (``range(highest, leftmost + 1)``), so the chain is walked
    cyclically here instead.  Returns a (2, n) array [bpp; metric]; fewer than 3 points (or collinear ones) are
    returned as they are."""
    pts = np.stack([np.asarray(bpp, dtype=np.float64), np.asarray(metric_mean, dtype=np.float64)], 1)
    if len(pts) < 3:
        return pts.T.copy()
    try:
        from scipy.spatial import ConvexHull
        hull = ConvexHull(points=pts)
    except Exception:
        return pts.T.copy()
    v = list(hull.vertices)
    n = len(v)
    left = int(np.argmin(pts[v, 0]))
    if higher_is_better:       # counter-clockwise, the upper chain runs from the highest point back to the leftmost
        start, stop = int(np.argmax(pts[v, 1])), left
    else:                      # ... and the lower chain from the leftmost point on to the lowest
        start, stop = left, int(np.argmin(pts[v, 1]))
    sel, i = [start], start
    while i != stop:
        i = (i + 1) % n
        sel.append(i)
    return pts[[v[i] for i in sel]].T.copy()
