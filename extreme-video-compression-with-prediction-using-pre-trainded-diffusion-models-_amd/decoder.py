"""Receiver: decode a batch of 30-frame clips from key-frame bitstreams + the transmit mask ``d``.

The reference never separates sender and receiver: ``city_sender.py:521-550`` runs the generator inside the
sender and keeps only the bit count.  The receiver side implied by that loop is restated here: frames with
``d == 1`` are ELIC key frames (decoded from their strings), runs of ``d == 0`` are generated, up to 5 at a
time, by the diffusion sampler conditioned on the last two decoded frames
(``SenderCity.update`` / ``generate_frame``, city_sender.py:326-351, 408-437), always 5 frames per call, of
which the receiver keeps as many as the mask says.

Clips are independent, so they are stacked along the batch axis of every kernel launch: all clips of a batch
must share the same mask (they do in the benchmark pattern; the sender policy can group by mask).
"""
import numpy as np
import torch

from . import keystrings as KS, lib as L, policy as P
from .recovery import generate_with_recovery, recovery_mode, supports_recovery


def all_generated_mask(frames=30, key=2, chunk=5):
    """2 key frames then generated chunks (the "maximum of 5 generation cycles"+ pattern of ret/readme.md:38)."""
    d = np.zeros(frames, dtype=np.int64)
    d[:key] = 1
    return d


class ClipDecoder:
    def __init__(self, scorenet, elic_model, config, sampler, groups=1, range_recovery=None, log=print, batch_invariant=False):
        self.net, self.elic, self.config, self.sampler = scorenet, elic_model, config, sampler
        # batch_invariant: ``generate`` runs on the network's batch-invariant view by default (a sample's frames then do not
        # depend on the launch it rides in); ``generate(..., invariant=)`` / format-4 jobs of ``decode_jobs`` choose per call
        self.batch_invariant = bool(batch_invariant)
        self._inv_net = None
        self.device = scorenet.device
        self.groups = groups          # concurrent clip groups (HIP streams) during generation
        self._stream_pool = []
        # "layer": a chunk whose fp16-split operands may have left their range is regenerated with the layers that raised
        # the event demoted to the bf16 split (recovery.py); "off" (default, or EVC_RANGE_RECOVERY): the caller's
        # check_numerics stops the run.  Networks without event sites (UNetDDPM, pseudo-3-D) keep the "off" behaviour.
        self.range_recovery = recovery_mode(range_recovery)
        if getattr(scorenet, "TILED", False) and self.range_recovery == "layer":
            raise ValueError("joint generation over tiles (TiledScoreNet) does not combine with range recovery "
                             "(range_recovery='layer'): recovery is not built for a network that runs a canvas as several "
                             "launches per step; run with EVC_CONV_ARITH=bf16x6 (no range assumption) instead")
        if self.batch_invariant:
            self._refuse_recovery()
            self.invariant_net()           # fail now for a network without the mode
        self.log = log
        self.chunks = 0               # generated chunks so far (recovery log lines name them)
        self.recovery_passes = []     # passes of every chunk recovery regenerated

    def recovers(self):
        return self.range_recovery == "layer" and supports_recovery(self.net)

    def _refuse_recovery(self):
        if self.range_recovery == "layer":
            raise ValueError("batch-invariant generation does not combine with range recovery (range_recovery='layer'): one "
                             "sample's event would demote layers for every sample and for the rest of the run, and a "
                             "receiver could not know which")

    def invariant_net(self):
        """The batch-invariant view of the score network (shares its packed weights), built on first use."""
        if self._inv_net is None:
            if getattr(self.net, "batch_invariant", False):
                self._inv_net = self.net
            elif hasattr(self.net, "invariant_view"):
                self._inv_net = self.net.invariant_view()
            else:
                raise NotImplementedError(f"batch-invariant generation is not built for {type(self.net).__name__}")
        return self._inv_net

    @torch.no_grad()
    def generate(self, cond_frames, noise_fn=None, generator=None, groups=None, invariant=None):
        """cond_frames: (B, 2, 3, H, W) in [0, 1] on the device -> (B, 5, 3, H, W) in [0, 1].
        = SenderCity.generate_frame (city_sender.py:326-351) without the per-chunk checkpoint reload.

        ``groups`` > 1 splits the batch into that many clip groups that are sampled concurrently, each on its
        own HIP stream (clips are independent): idle CUs during one group's small kernels / partial tile rounds
        run another group's convolutions.  Per-clip results do not depend on the grouping when noise is injected
        (``noise_fn`` is then called per group with the group's slice bounds).

        With range recovery on, the state of every noise source is saved first and restored before each regeneration:
        ``generator`` (the per-group generators of ``groups`` > 1 are seeded from it, so they replay too), the device's
        default generator when ``generator`` is None (exact for one group; several groups without a generator draw their
        seeds from the host entropy pool and replay with new noise), and the network's ``cond_generator``; ``noise_fn``
        must be deterministic (the policy sweep's counter-based noise is)."""
        self.chunks += 1
        invariant = self.batch_invariant if invariant is None else bool(invariant)
        if invariant:
            self._refuse_recovery()
            return self._generate(cond_frames, noise_fn, generator, groups, net=self.invariant_net())
        if not self.recovers():
            return self._generate(cond_frames, noise_fn, generator, groups)
        net = self.net
        saved_gen = generator.get_state() if generator is not None else None
        saved_default = torch.cuda.get_rng_state(self.device) if generator is None and noise_fn is None else None
        cgen = getattr(net, "cond_generator", None)
        saved_cond = cgen.get_state() if cgen is not None else None

        def restore():
            if saved_gen is not None:
                generator.set_state(saved_gen)
            if saved_default is not None:
                torch.cuda.set_rng_state(saved_default, self.device)
            if saved_cond is not None:
                cgen.set_state(saved_cond)

        res = {}

        def run():
            res["frames"], res["raw"] = self._generate(cond_frames, noise_fn, generator, groups, with_raw=True)
            return res["raw"]          # the sampler's output before inverse_data_transform (its clamp keeps NaN, but turns an inf into 0 / 1)

        _, passes, new = generate_with_recovery(run, restore, net, where=f"chunk {self.chunks}", log=self.log)
        if new:
            self.recovery_passes.append(passes)
        return res["frames"]

    def _generate(self, cond_frames, noise_fn, generator, groups, with_raw=False, net=None):
        from . import sampler as S
        cfg = self.config
        net = self.net if net is None else net
        B, _, C, H, W = cond_frames.shape
        groups = self.groups if groups is None else groups
        groups = max(1, min(int(groups), B))
        if getattr(net, "SPADE", False):
            # the SPADE network caches its per-chunk gamma / beta maps for ONE conditioning tensor: interleaved clip groups
            # would each pass their own slice and rebuild all maps on every forward (~20 ms against a 15 ms forward)
            groups = 1
        if getattr(net, "TILED", False):
            # the tiled view gathers the tiles of ONE conditioning tensor per chunk (tiled.py): per-group slices would be
            # gathered again on every forward
            groups = 1
        cond = cond_frames.reshape(B, -1, H, W).contiguous()
        if cfg.data.rescaled:
            cond = L.scale_clamp(cond, 2.0, -1.0)                          # data_transform: 2x - 1
        ch = cfg.data.channels * cfg.data.num_frames
        kw = dict(final_only=True, denoise=cfg.sampling.denoise, subsample_steps=getattr(cfg.sampling, "subsample", None),
                  clip_before=getattr(cfg.sampling, "clip_before", True))
        step_gen = S.get_step_generator(self.sampler)

        def draw(tag, lo, hi, gen_):
            shp = (hi - lo, ch, H, W)
            if noise_fn is not None:
                return noise_fn(tag, (B, ch, H, W))[lo:hi].to(self.device).contiguous()
            return torch.randn(shp, device=self.device, dtype=torch.float32, generator=gen_)

        if groups == 1 or step_gen is None:
            x_T = draw("init", 0, B, generator)
            step_noise = None if noise_fn is None else (lambda i, x: draw(i, 0, B, None))
            out = self.sampler(x_T, net, cond=cond, noise_fn=step_noise, generator=generator, **kw)
            pred = out[-1].contiguous()
        else:
            bounds = [(g * B // groups, (g + 1) * B // groups) for g in range(groups)]
            main = torch.cuda.current_stream()
            streams = self._streams(groups)
            if hasattr(net, "prepare_labels"):
                # AdaGN table rows are shared state: build every row this sampler will read (F-PNDM: incl. the
                # Runge-Kutta midpoints and -1) on the main stream, which all group streams wait on below
                net.prepare_labels(S.label_set(self.sampler, net, kw["subsample_steps"], kw["denoise"]))
            gens = []
            for (lo, hi), st in zip(bounds, streams):
                st.wait_stream(main)
                with torch.cuda.stream(st):
                    gen_g = None
                    if noise_fn is None:
                        gen_g = torch.Generator(device=self.device)
                        gen_g.manual_seed(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=generator, device=self.device))
                                          if generator is not None else torch.seed() % (2 ** 31))
                    x_T = draw("init", lo, hi, gen_g)
                    sn = None if noise_fn is None else (lambda i, x, lo=lo, hi=hi: draw(i, lo, hi, None))
                    gens.append(step_gen(x_T, net, cond=cond[lo:hi].contiguous(), noise_fn=sn, generator=gen_g, **kw))
            outs = S.run_interleaved(gens, streams)
            for st in streams:
                main.wait_stream(st)
            pred = torch.cat([o[-1] for o in outs], dim=0).contiguous()
        frames = L.scale_clamp(pred, 0.5, 0.5, (0.0, 1.0)) if cfg.data.rescaled else \
            L.scale_clamp(pred, 1.0, 0.0, (0.0, 1.0))                         # inverse_data_transform
        frames = frames.reshape(B, cfg.data.num_frames, C, H, W)
        return (frames, pred) if with_raw else frames

    def _streams(self, n):
        while len(self._stream_pool) < n:
            self._stream_pool.append(torch.cuda.Stream(device=self.device))
        return self._stream_pool[:n]

    @torch.no_grad()
    def decode(self, d, key_strings, shape, frames=30, noise_fn=None, generator=None, key_frames=None, size=None):
        """d: (frames,) 0/1 mask shared by the batch; key_strings: list over key-frame positions (in order) of
        ``[y_strings, z_strings]`` for the whole batch.  Returns (B, frames, 3, H, W) float32 on the device.
        ``key_frames``: the decoded key frames themselves, one (B, 3, H, W) device tensor per key-frame position, for a sender
        that estimated its rate and has no strings (``ElicModel.estimate``); ``key_strings`` and ``shape`` are then not read.
        ``size`` = (H, W): the key frames are cropped to it before anything is generated from them (a whole-frame canvas whose
        size is no multiple of the ELIC padding; default: they are used as decoded)."""
        crop = (lambda x: x) if size is None else (lambda x: x[..., :size[0], :size[1]])
        d = np.asarray(d).reshape(-1)
        out = []
        k = 0
        t = 0
        n_key = int(d[:frames].sum())
        assert len(key_frames if key_frames is not None else key_strings) >= n_key, "not enough key frames for the mask"
        while t < frames:
            if d[t] == 1:
                # decode every consecutive key frame of this run in one batched ELIC call
                run = 0
                while t + run < frames and d[t + run] == 1:
                    run += 1
                if key_frames is not None:
                    out.append(crop(torch.stack(list(key_frames[k:k + run]), 1)))
                    k += run
                    t += run
                    continue
                x_hat = crop(self.elic.decompress(KS.merge(key_strings[k:k + run]), shape)["x_hat"])      # (run*B, 3, H, W)
                B = x_hat.shape[0] // run
                x_hat = x_hat.reshape(run, B, *x_hat.shape[1:]).permute(1, 0, 2, 3, 4)
                out.append(x_hat)
                k += run
                t += run
            else:
                assert t >= 2, "a generated frame needs two decoded frames before it"
                run = 0
                while t + run < frames and d[t + run] == 0 and run < self.config.data.num_frames:
                    run += 1
                prev = torch.cat(out, dim=1)[:, -2:]
                gen = self.generate(prev.contiguous(), noise_fn=noise_fn, generator=generator)
                out.append(gen[:, :run])
                t += run
        return torch.cat(out, dim=1)[:, :frames].contiguous()

    @torch.no_grad()
    def decode_jobs(self, jobs, max_batch=32, models=None, size=None, share=False, stats=None, patch=64):
        """Decode policy-job streams (``container.unpack_job`` dicts; possibly different q, masks and program lengths).

        All jobs advance in lockstep, as ``policy.run_policy`` advances them on the sender: each round every unfinished job
        executes its next segment.  The jobs whose segment is ("gen", n) are stacked along the batch axis of one
        ``generate`` call (``max_batch`` per launch), each drawing the noise of its own key (seed, stream id, start frame =
        frames it holds so far, step) -- noise specification N1; a segment of noise trial t of a format-5 / format-6 stream
        draws start frame + 65536 t, the one draw the sender chose: its K trials never multiply the receiver's work -- and
        keep the first n frames; the jobs whose segment is
        ("key", n) decode its n frames in one ``decompress`` call per q (several jobs share a call up to ``max_batch``
        frames; a segment is never split).  ``models``: q -> ElicModel (default: this decoder's own model for every q);
        ``size`` = (H, W) of a frame (default: the generator's image size): the ELIC output is cropped to it, as the sender
        crops its padded frames.  A stream whose hyper-latent ``shape`` is not that of a frame of ``size`` padded to ``patch``
        (the sender's --patch; (ceil(H / 64), ceil(W / 64)) for the default 64) was made for frames of another size and is
        refused (``StreamSizeError``, a ValueError) instead of being cropped to this one.
        The generator settings of the streams (sampler, subsample steps, denoise) must be the ones
        this decoder was built with.  Format-4 jobs (``job["plan"]`` set: generated in batch-invariant mode) run their
        generation rounds on the network's batch-invariant view, in launches of their own: their frames are the sender's
        bit for bit at any ``max_batch``.

        ``share=True`` does every distinct piece of work of a round once (the receiving side of ``run_policy(share=True)``;
        nothing in a stream says it was shared, and nothing is guessed).  A key frame is identified by (q, its string bytes):
        each distinct key frame of a round is decoded once, ``max_batch`` frames per call, whichever jobs name it.  A generation
        state is (seed, stream id, format-4 flag, frames held, noise trial, identities of the last two frames): the jobs of a state draw the
        same noise for the same conditioning frames, so one sample is generated per state (``max_batch`` states per launch)
        and each job keeps the first n frames its own segment names.  Streams of a sender with one noise stream per job have
        distinct stream ids and merge on key frames only.  Jobs advance by segment, so two jobs share a state only while they
        execute it in the same round.  Format-4 jobs keep launches of their own and their frames are the sender's bit for bit
        either way.  ``stats``: optional dict; ``launch_sizes`` {samples in a launch: launches}, ``samples`` (generated samples),
        ``job_rounds`` (generation segments executed) and ``key_frames_decoded`` are added up in it.
        Returns one (frames, 3, H, W) float32 device tensor per job."""
        run = _JobRounds(self, jobs, max_batch, models, size, share, stats, patch)
        run.check_jobs()
        while True:
            todo = [j for j in run.jobs if j.pos < len(j.stream["segments"])]
            if not todo:
                break
            run.generation_round([j for j in todo if j.segment[0] == "gen"])
            run.key_round([j for j in todo if j.segment[0] == "key"])
            for j in todo:
                j.pos += 1
        return [torch.stack(j.x, 0).contiguous() for j in run.jobs]


class _RxJob:
    """One job stream (a ``container.unpack_job`` dict) while ``decode_jobs`` executes it: its decoded frames ``x``, under ``share``
    their identities ``ids`` (("key", q, n) for the n-th distinct key frame, ``policy.gen_id``), the next segment ``pos`` and the
    number of key frames consumed ``used``."""

    def __init__(self, stream):
        self.stream, self.x, self.ids, self.pos, self.used = stream, [], [], 0, 0

    @property
    def segment(self):
        return self.stream["segments"][self.pos]

    @property
    def trial(self):
        """The noise trial of the gen segment in execution (formats 5 / 6; 0 in a stream without trials)."""
        return self.stream["trials"][self.pos] if self.stream.get("n_trials", 1) > 1 else 0

    def segment_strings(self):
        """Per frame of the key segment in execution, its strings."""
        return self.stream["key_strings"][self.used:self.used + self.segment[1]]

    def take_keys(self, frames, names=()):
        """The key segment is done: its frames and, under ``share``, their identities."""
        self.x, self.ids, self.used = self.x + frames, self.ids + list(names), self.used + len(frames)


class _JobRounds:
    """The steps of one ``ClipDecoder.decode_jobs`` call and what they share."""

    def __init__(self, decoder, streams, max_batch, models, size, share, stats, patch=64):
        cfg = decoder.config
        self.decoder, self.max_batch, self.share, self.stats, self.patch = decoder, max_batch, share, stats, int(patch)
        self.jobs = [_RxJob(s) for s in streams]
        self.size = size if size is not None else (cfg.data.image_size, cfg.data.image_size)
        self.channels = cfg.data.channels * cfg.data.num_frames
        self.model_of = (lambda q: decoder.elic) if models is None else (lambda q: models[q])
        self.grouper, self.key_names = P.StateGrouper(), {}

    def count(self, name, n):
        if self.stats is not None:
            self.stats[name] = self.stats.get(name, 0) + n

    def check_jobs(self):
        """Every stream is one this decoder can replay: known noise, the generator settings it was built with, a sound program."""
        from . import container as Cn, sampler as S
        cfg = self.decoder.config
        mine = (getattr(cfg.sampling, "subsample", None) or 0, bool(cfg.sampling.denoise))
        for job in (j.stream for j in self.jobs):
            if job["noise_spec"] != Cn.NOISE_N1:
                raise ValueError(f"unknown noise specification id {job['noise_spec']}")
            if S.get_sampler(job["sampler"]) is not self.decoder.sampler or (job["subsample"], job["denoise"]) != mine:
                raise ValueError(f"job stream v{job['vid']} q{job['q']} thr {job['thr']:.2f} was generated with "
                                 f"{job['sampler']}-{job['subsample']} denoise={job['denoise']}: build the decoder with them")
            Cn.check_segments(job["segments"], job["frames"], len(job["key_strings"]))
            check_stream_size(job, self.size, self.patch)
            if job.get("n_trials", 1) > 1:
                Cn.check_trials(job["segments"], job["trials"], job["n_trials"])

    def generation_round(self, gen):
        """gen: the jobs whose segment is ("gen", n).  One seed per noise launch, one generation plan per score-network launch;
        within those one sample per state (``share``; else per job), ``max_batch`` samples per launch."""
        launch_of = lambda j: (j.stream["seed"], j.stream.get("plan") is not None)      # noqa: E731
        for seed, inv in sorted({launch_of(j) for j in gen}):
            same = [j for j in gen if launch_of(j) == (seed, inv)]
            states = self.grouper.group(same, self.share, state=lambda j: (j.stream["stream_id"], len(j.x), j.trial, j.ids[-1], j.ids[-2]))
            self.count("job_rounds", len(same))
            self.count("samples", len(states))
            for part in P.in_launches(states, self.max_batch):
                heads = [members[0] for _, members in part]                              # a state's members hold the same frames
                noise = P.n1_noise([(j.stream["stream_id"], P.trial_start(len(j.x), j.trial)) for j in heads], seed, self.decoder.device)
                pred = P.generation_launch(self.decoder, heads, noise, inv, self.stats)
                assert pred.shape[1] * pred.shape[2] == self.channels
                for k, (serial, members) in enumerate(part):
                    for j in members:                                                    # each keeps what its own segment names
                        n = j.segment[1]
                        j.x += [pred[k, t] for t in range(n)]
                        j.ids += [P.gen_id(serial, t, j.trial) for t in range(n)]

    def decode_keys(self, q, strings, jobs):
        """strings: per frame, in launch order, of key frames of ``jobs`` -> the frames of one ``decompress`` call of q's model,
        cropped to the frame size as the sender crops its padded frames."""
        shape = jobs[0].stream["shape"]
        assert all(tuple(j.stream["shape"]) == tuple(shape) for j in jobs), "one frame size per decoder"
        H, W = self.size
        return self.model_of(q).decompress(KS.merge(strings), shape)["x_hat"][:, :, :H, :W]

    def key_name(self, q, strings):
        """(q, string bytes) -> a small id; the bytes are kept once."""
        return ("key", q, self.key_names.setdefault((q,) + KS.flat(strings), len(self.key_names)))

    def key_round(self, key):
        """key: the jobs whose segment is ("key", n): per q, ``shared_keys`` or ``segment_keys``."""
        for q in sorted({j.stream["q"] for j in key}):
            (self.shared_keys if self.share else self.segment_keys)(q, [j for j in key if j.stream["q"] == q])

    def shared_keys(self, q, same):
        """Every distinct key frame of the round once, in first-seen order, ``max_batch`` per call, for the jobs that name it."""
        names = [[self.key_name(q, s) for s in j.segment_strings()] for j in same]
        want = {}
        for j, mine in zip(same, names):
            for name, s in zip(mine, j.segment_strings()):
                want.setdefault(name, s)
        order, frame_of = list(want), {}
        for c0 in range(0, len(order), self.max_batch):
            part = order[c0:c0 + self.max_batch]
            frame_of.update(zip(part, self.decode_keys(q, [want[name] for name in part], same)))
        self.count("key_frames_decoded", len(order))
        for j, mine in zip(same, names):
            j.take_keys([frame_of[name] for name in mine], mine)

    def segment_keys(self, q, same):
        """Whole segments in job order, packed greedily up to ``max_batch`` frames per call: a segment is never split."""
        while same:
            part, n = [], 0
            while same and (not part or n + same[0].segment[1] <= self.max_batch):
                n += same[0].segment[1]
                part.append(same.pop(0))
            x_hat = iter(self.decode_keys(q, [s for j in part for s in j.segment_strings()], part))
            self.count("key_frames_decoded", n)
            for j in part:
                j.take_keys([next(x_hat) for _ in range(j.segment[1])])


LATENT_STRIDE = 64             # frame samples per hyper-latent sample of ELIC (g_a: 16, h_a: 4)


def latent_shape(size, patch=64):
    """The hyper-latent shape of an (H, W) frame zero-padded to multiples of ``patch`` (``elic.pad_to_patch``)."""
    return tuple(-(-int(n) // patch) * patch // LATENT_STRIDE for n in size)


class StreamSizeError(ValueError):
    """A job stream was made for frames of another size than the one it is decoded at."""


def check_stream_size(job, size, patch=64):
    """A job stream decodes at the frame size it was made for: its hyper-latent ``shape`` must be ``latent_shape(size)``."""
    got, want = tuple(int(v) for v in job["shape"]), latent_shape(size, patch)
    if got != want:
        made = " x ".join(f"{(n - 1) * LATENT_STRIDE + 1}..{n * LATENT_STRIDE}" for n in got)
        raise StreamSizeError(f"job stream v{job['vid']} q{job['q']} thr {job['thr']:.2f} was made for frames of {made} (rows x columns; "
                              f"hyper-latent shape {got}), not for the {size[0]} x {size[1]} it is decoded at (shape {want}): pass "
                              f"the sender's frame size")


def total_bits(key_strings):
    return KS.bits(key_strings)
