"""GPU tests of batch-invariant mode: in that mode the numbers computed for one sample are a function
of that sample's inputs, its step label and the weights only.  Every comparison of a sample alone against the same sample
inside a batch is ``torch.equal`` / ``np.array_equal``; the only tolerances are the project's existing accuracy bars
against the reference goldens (2e-4 per forward, 5e-4 per trajectory: DESIGN.md section 5).

The CPU side (the plan query, container format 4, the refusals) is tests/test_invariant_plan.py."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import golden, rnd
from test_invariant_plan import FULL_SIZE_CONVS

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1, 2, 3, 5, 9, 32)


@pytest.fixture(scope="module")
def L():
    import evc_amd  # noqa: F401
    from evc_amd import lib
    lib.hip_lib()
    return lib


@pytest.fixture(autouse=True)
def no_range_events(L):
    """No test of this module may raise an fp16-split range event."""
    L.range_events(reset=True)
    yield
    assert L.range_events() == 0


def rows_of(B):
    """Which of three fixed samples sits at the first, a middle and the last row of a batch of B (later entries win)."""
    at = {0: 0}
    at[B // 2] = 1
    at[B - 1] = 2
    return at


def batch_of(pool, B, fill):
    """A batch of B rows of ``pool`` (samples 0..2 at the rows ``rows_of`` names, filler samples elsewhere)."""
    at = rows_of(B)
    idx = [at.get(r, 3 + (r + fill) % (pool.shape[0] - 3)) for r in range(B)]
    return pool[torch.tensor(idx, device=pool.device)].contiguous(), at


def magnitudes(n, device):
    """Per-sample scales spanning several powers of two: neighbours land in different bins of the fp16 split's scale."""
    return torch.tensor([4.0 ** ((i * 5) % 7 - 3) for i in range(n)], device=device)


# ---- per op -----------------------------------------------------------------------------------------------------

def test_chan_stats_and_bound_words_per_sample(L):
    g = torch.Generator(device="cuda").manual_seed(5)
    for H, C in ((8, 768), (16, 576), (32, 384), (128, 192)):
        pool = torch.randn(12, H, H, C, device="cuda", generator=g) * magnitudes(12, "cuda")[:, None, None, None]
        alone = {}
        for s in range(3):
            x = pool[s:s + 1].contiguous()
            st = L.chan_stats(x, invariant=True)
            w = torch.zeros(1, dtype=torch.int32, device="cuda")
            coef = L.gn_coeffs([st], H * H, 32, 1e-5, bound=w, invariant=True)
            w3 = torch.zeros(3, dtype=torch.int32, device="cuda")
            L.moments_bound(st, 0, C // 3, w3, invariant=True)
            alone[s] = (st, coef, w, w3)
        assert len({int(alone[s][2]) for s in range(3)}) == 3          # different magnitudes: different bound words
        for B in BATCHES:
            x, at = batch_of(pool, B, B)
            st = L.chan_stats(x, invariant=True)
            w = torch.zeros(B, dtype=torch.int32, device="cuda")
            ca, cs = L.gn_coeffs([st], H * H, 32, 1e-5, bound=w, invariant=True)
            w3 = torch.zeros(3 * B, dtype=torch.int32, device="cuda")
            L.moments_bound(st, 0, C // 3, w3, invariant=True)
            for r, s in at.items():
                ast, acoef, aw, aw3 = alone[s]
                assert torch.equal(st[r], ast[0]), (H, B, r)
                assert torch.equal(ca[r], acoef[0][0]) and torch.equal(cs[r], acoef[1][0]), (H, B, r)
                assert int(w[r]) == int(aw) and torch.equal(w3.view(B, 3)[r], aw3), (H, B, r)


def _conv_case(L, cfg, n, pool_n=8):
    """Operands of one convolution configuration for ``pool_n`` samples of different magnitude."""
    H, W, C0, C1, Co, K, arith, coef, act, x2c, bound = cfg
    g = torch.Generator(device="cuda").manual_seed(2000 + n)
    C = C0 + C1
    raw = bool(bound)                               # the launch reads a raw tensor scaled from its element bound
    assert not (raw and coef)
    mag = magnitudes(pool_n, "cuda")[:, None, None, None] if (raw or x2c) else 1.0
    c = types.SimpleNamespace(cfg=cfg, raw=raw)
    c.x0 = torch.randn(pool_n, H, W, C0, device="cuda", generator=g) * (mag if raw else 1.0)
    c.x1 = torch.randn(pool_n, H, W, C1, device="cuda", generator=g) * (mag if raw else 1.0) if C1 else None
    w = torch.randn(Co, C, K, K, device="cuda", generator=g) / np.sqrt(C * K * K)
    c.wp = L.conv_pack_weights(w, arith)
    c.bias = torch.randn(Co, device="cuda", generator=g)
    c.res = torch.randn(pool_n, H, W, Co, device="cuda", generator=g) if raw else None
    c.coef = None
    if coef:
        c.coef = (1 + 0.2 * torch.randn(pool_n, C, device="cuda", generator=g), 0.3 * torch.randn(pool_n, C, device="cuda", generator=g))
    c.x2 = c.w2p = None
    if x2c:
        c.x2 = torch.randn(pool_n, H, W, x2c, device="cuda", generator=g) * mag
        c.w2p = L.conv_pack_weights(torch.randn(Co, x2c, 1, 1, device="cuda", generator=g) / np.sqrt(x2c), L.ARITH_F16X3)
    return c


def _conv_run(L, c, idx):
    H, W, C0, C1, Co, K, arith, coef, act, x2c, _ = c.cfg
    sel = torch.tensor(idx, device="cuda")
    B = len(idx)
    pick = lambda t: None if t is None else t[sel].contiguous()      # noqa: E731
    x0, x1 = pick(c.x0), pick(c.x1)
    groups = lambda ch: 32 if ch % 32 == 0 else 1                    # noqa: E731
    bound = x2 = None
    if c.raw:
        bound = torch.zeros(B, dtype=torch.int32, device="cuda")
        L.gn_coeffs([L.chan_stats(x0, invariant=True)] + ([L.chan_stats(x1, invariant=True)] if C1 else []), H * W,
                    groups(C0 + C1), 1e-5, bound=bound, invariant=True)
    if x2c:
        xx = pick(c.x2)
        b2 = torch.zeros(B, dtype=torch.int32, device="cuda")
        L.gn_coeffs([L.chan_stats(xx, invariant=True)], H * W, groups(x2c), 1e-5, bound=b2, invariant=True)
        x2 = (xx, None, c.w2p, b2)
    coef_ = None if c.coef is None else (pick(c.coef[0]), pick(c.coef[1]))
    if Co % 16:          # the output convolution: 15 channels in a 16-wide buffer, no moments (as the network calls it)
        buf = torch.zeros(B, H, W, (Co + 15) // 16 * 16, device="cuda")
        out = L.conv2d_nhwc(x0, c.wp, Co, K, K, bias=c.bias, src1=x1, coef=coef_, act_in=act, out=buf, invariant=True)
        return out[..., :Co], torch.zeros(B, 1, device="cuda"), bound
    out, st = L.conv2d_nhwc(x0, c.wp, Co, K, K, bias=c.bias, src1=x1, coef=coef_, act_in=act, res=pick(c.res),
                            out_scale=0.70710678, in_bound=bound, want_stats=True, x2=x2, invariant=True)
    return out, st, bound


def test_every_conv_launch_of_the_full_size_forward_alone_and_in_a_batch(L):
    """Every distinct convolution launch of the full-size forward (the literal list of tests/test_invariant_plan.py), outputs
    AND moments: row b of the batched launch against the one-sample launch of sample b, B in {1, 2, 3, 5, 9, 32}, first /
    middle / last row; raw operands (1x1 skip convolutions, output projections, fused 1x1 operands) have samples of
    different magnitude, each scaled from its own bound word."""
    n_checked = 0
    for n, cfg in enumerate(FULL_SIZE_CONVS):
        c = _conv_case(L, cfg, n)
        alone = {s: _conv_run(L, c, [s]) for s in range(3)}
        if c.raw or cfg[9]:
            assert bool(torch.isfinite(alone[0][0]).all())
        for B in BATCHES:
            at = rows_of(B)
            idx = [at.get(r, 3 + (r + B) % 5) for r in range(B)]
            out, st, bound = _conv_run(L, c, idx)
            for r, s in at.items():
                assert torch.equal(out[r], alone[s][0][0]), (cfg, B, r)
                assert torch.equal(st[r], alone[s][1][0]), (cfg, B, r, "moments")
                if bound is not None:
                    assert int(bound[r]) == int(alone[s][2][0]), (cfg, B, r, "bound")
                n_checked += 1
        del c, alone
    print(f"{len(FULL_SIZE_CONVS)} convolution configurations, {n_checked} row comparisons, all bitwise equal")


def test_both_attention_kernels_alone_and_in_a_batch(L):
    """The network's (heads, N, D): 2 x 1024 x 192, 3 x 256 x 192 (fp16-split kernel with per-sample q | k | v bounds) and
    4 x 64 x 192 (below 128 keys the f32 kernel serves both), each also on the f32 kernel (no bounds)."""
    g = torch.Generator(device="cuda").manual_seed(9)
    for heads, N in ((2, 1024), (3, 256), (4, 64)):
        C = heads * 192
        pool = torch.randn(8, N, 3 * C, device="cuda", generator=g) * magnitudes(8, "cuda")[:, None, None].clamp(0.25, 4.0)

        def run(idx, f16):
            qkv = pool[torch.tensor(idx, device="cuda")].contiguous()
            B = len(idx)
            b = None
            if f16:
                st = L.chan_stats(qkv.view(B, N, 1, 3 * C), invariant=True)
                b = torch.zeros(3 * B, dtype=torch.int32, device="cuda")
                L.moments_bound(st, 0, C, b, invariant=True)
            return L.attention(qkv, C, heads, bounds=b, invariant=True), b
        for f16 in (True, False):
            alone = {s: run([s], f16) for s in range(3)}
            for B in BATCHES:
                at = rows_of(B)
                out, b = run([at.get(r, 3 + (r + B) % 5) for r in range(B)], f16)
                for r, s in at.items():
                    assert torch.equal(out[r], alone[s][0][0]), (heads, N, f16, B, r)
                    if b is not None:
                        assert torch.equal(b.view(B, 3)[r], alone[s][1]), (heads, N, B, r)


# ---- the full-size network --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def full_nets(L):
    """The full-size (262 M parameter) default network and its batch-invariant view: ONE set of packed weights."""
    from test_gpu_scorenet import build
    net, d, p = build(192, 192, 128, 1234)
    inv = net.invariant_view()
    assert inv.batch_invariant and not net.batch_invariant
    for i, e in net.w.items():
        for k, v in e.items():
            if torch.is_tensor(v):
                assert inv.w[i][k].data_ptr() == v.data_ptr(), (i, k)
    return net, inv


def _b9_inputs():
    x = torch.cat([rnd(600 + i, 1, 15, 128, 128) for i in range(9)], 0).cuda()
    cond = torch.cat([rnd(700 + i, 1, 6, 128, 128) for i in range(9)], 0).cuda()
    return x, cond


def rel(a, b):
    a = a.detach().float().cpu().numpy() if torch.is_tensor(a) else a
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def test_invariant_forward_meets_the_accuracy_bars_of_the_default(full_nets):
    """The new arithmetic against the reference goldens at the existing 2e-4 of max|ref|: B = 1 and B = 9."""
    _, inv = full_nets
    g = golden("forward_full")
    x, cond = rnd(51, 1, 15, 128, 128).cuda(), rnd(52, 1, 6, 128, 128).cuda()
    o = inv(x, torch.tensor([500]), cond=cond).cpu()
    e1 = max(rel(o.reshape(-1)[::60].numpy(), g["samples"]), rel(o[0, :, 0, :].numpy(), g["first_row"]))
    g = golden("forward_full_b9")
    x, cond = _b9_inputs()
    o = inv(x, torch.tensor([500] * 9), cond=cond).cpu().reshape(9, -1)
    e9 = max(rel(o[i, ::60].numpy(), g["samples"][i]) for i in range(9))
    print(f"invariant full-size forward vs reference goldens: B=1 {e1:.2e}, B=9 {e9:.2e} (bar 2e-4)")
    assert e1 < 2e-4 and e9 < 2e-4


def test_full_size_forward_rows_equal_the_one_sample_forward(full_nets, L):
    """Nine samples, one of them (sample 3, input and conditioning frames x 4) scaled so that its raw-operand bounds land
    in another power-of-two bin than its neighbours' and one scaled down, in batches of 2 .. 32 and at rotating rows,
    against their own B = 1 forwards.  The default network on the
    same batches does NOT reproduce its own B = 1 bits (asserted, so the comparison is not vacuous)."""
    net, inv = full_nets
    x, cond = _b9_inputs()
    x[3] *= 4.0
    cond[3] *= 4.0
    x[6] *= 0.125
    cond[6] *= 0.125
    labels = [500, 500, 99, 500, 500, -0.5, 500, 99, 500]
    alone, bins = [], []
    for s in range(9):
        alone.append(inv(x[s:s + 1].contiguous(), torch.tensor([labels[s]]), cond=cond[s:s + 1].contiguous()))
        # the first bound slot of a forward: the element bound of the first 1x1 skip convolution's raw operand
        bins.append((int(inv._bounds[0]) >> 23) & 0xff)
    print("power-of-two bins (biased exponent of the squared bound) of the nine samples:", bins)
    assert bins[3] != bins[2] and bins[3] != bins[4], bins
    differs = 0
    for B in (2, 3, 5, 6, 8, 9, 32):
        idx = [(r + B) % 9 for r in range(B)]              # the same sample sits at other rows in other batches
        sel = torch.tensor(idx, device="cuda")
        lab = torch.tensor([labels[s] for s in idx])
        o = inv(x[sel].contiguous(), lab, cond=cond[sel].contiguous())
        words = inv._bounds[:B].tolist()
        for r, s in enumerate(idx):
            assert torch.equal(o[r], alone[s][0]), (B, r, s)
            assert (words[r] >> 23) & 0xff == bins[s], (B, r, s)
        if B in (2, 9):
            d = net(x[sel].contiguous(), lab, cond=cond[sel].contiguous())
            d1 = net(x[idx[0]:idx[0] + 1].contiguous(), lab[:1], cond=cond[idx[0]:idx[0] + 1].contiguous())
            differs += int(not torch.equal(d[0], d1[0]))
    assert differs > 0, "the default mode reproduced its B = 1 bits: this test shows nothing"
    assert L.range_events() == 0


def test_literal_conv_list_is_what_a_real_forward_launches(full_nets, L):
    _, inv = full_nets
    inv.prepare_labels([500])                   # (the label table's own launches are not part of a forward)
    for B in (1, 9):
        prof = []
        L.CONV_PROFILE = prof
        try:
            inv.forward_label(rnd(900, B, 15, 128, 128).cuda(), 500, rnd(901, B, 6, 128, 128).cuda())
        finally:
            L.CONV_PROFILE = None
        torch.cuda.synchronize()
        seen = {(c["H"], c["W"], c["C0"], c["C1"], c["Co"], c["K"], c["arith"], int(c["coef"]), c["act_in"], c["x2"], int(c["bound"]))
                for c in (r["call"] for r in prof)}
        assert all(r["call"]["invariant"] for r in prof)
        assert seen == set(FULL_SIZE_CONVS), (B, seen ^ set(FULL_SIZE_CONVS))


def test_invariant_attention_ignores_the_process_wide_switches(L):
    """``evc_attention_set_option`` moves the default dispatch (which kernel from how many keys, K / V images or not); the
    invariant plan is a function of (heads, N, D) only."""
    g = torch.Generator(device="cuda").manual_seed(11)
    heads, N, C = 3, 256, 576
    qkv = torch.randn(2, N, 3 * C, device="cuda", generator=g)
    b = torch.zeros(6, dtype=torch.int32, device="cuda")
    L.moments_bound(L.chan_stats(qkv.view(2, N, 1, 3 * C), invariant=True), 0, C, b, invariant=True)
    b1 = torch.zeros(3, dtype=torch.int32, device="cuda")
    L.moments_bound(L.chan_stats(qkv.view(2, N, 1, 3 * C)), 0, C, b1)
    want, dflt = L.attention(qkv, C, heads, bounds=b, invariant=True), L.attention(qkv, C, heads, bounds=b1)
    try:
        L.attention_set_option("f16_min_keys", 1 << 20)
        L.attention_set_option("kv_planes", 0)
        assert torch.equal(L.attention(qkv, C, heads, bounds=b, invariant=True), want)
        assert not torch.equal(L.attention(qkv, C, heads, bounds=b1), dflt)       # the default dispatch did move (f32 kernel)
    finally:
        L.attention_set_option("f16_min_keys", 128)
        L.attention_set_option("kv_planes", 1)


def _reduced_base(seed=41):
    from evc_amd.scorenet import ScoreNet
    from oracle.scorenet import Dims, seeded_params
    from test_gpu_scorenet import make_config
    return ScoreNet(make_config(32, 32, 32), seeded_params(Dims(ngf=32, n_head_channels=32, image_size=32), seed))


def test_label_rows_do_not_depend_on_what_else_is_prepared(L):
    """The AdaGN table of an invariant network: the rows of three labels prepared in one call equal, bitwise, the row each
    label gets when it is prepared alone on a fresh view, and when the labels arrive in another grouping.  (The default
    network evaluates all new labels as one launch of R pixels, whose plan follows R.)"""
    base = _reduced_base()
    labels = [500.0, 99.0, -0.5, 7.0, 998.0]
    together = base.invariant_view()
    together.prepare_labels(labels)
    row = lambda net, v: net._table[net._rows[net._key(v)]]          # noqa: E731
    regroup = base.invariant_view()
    regroup.prepare_labels(labels[3:])
    regroup.prepare_labels(labels[:3])
    for v in labels:
        alone = base.invariant_view()
        alone.prepare_labels([v])
        assert alone._n_rows == 1
        assert torch.equal(row(alone, v), row(together, v)), v
        assert torch.equal(row(regroup, v), row(together, v)), v
    assert together._table.data_ptr() != base._table.data_ptr() and base._n_rows == 0


def test_view_refuses_after_the_base_network_demotes(L):
    """The view shares the packed weights: once ``demote`` repacks some of them on the base network the view's fixed
    arithmetic is gone, and it says so instead of computing other bits."""
    base = _reduced_base()
    view = base.invariant_view()
    x, cond = rnd(42, 2, 15, 32, 32).cuda(), rnd(43, 2, 6, 32, 32).cuda()
    view(x, torch.tensor([500, 500]), cond=cond)
    with pytest.raises(ValueError, match="demoted"):
        view.demote([0])
    assert base.demote([0]) == [0]
    with pytest.raises(ValueError, match="demoted"):
        view(x, torch.tensor([500, 500]), cond=cond)
    with pytest.raises(ValueError, match="demoted"):
        base.invariant_view()
    base(x, torch.tensor([500, 500]), cond=cond)                     # the base network itself goes on


# ---- chains on the reduced networks -----------------------------------------------------------------------------

def test_reduced_net_ddpm_trajectory_golden_in_invariant_mode(L):
    """The 32 x 32 reduced network (levels down to 2 x 2: tiles that hold many samples, per-row scales) through 5 DDPM steps +
    denoise against the reference trajectory at the existing 5e-4; and sample 0 alone equals sample 0 of the pair."""
    from evc_amd import sampler
    from evc_amd.scorenet import ScoreNet
    from oracle.scorenet import Dims, seeded_params
    from test_gpu_scorenet import make_config
    g = golden("samplers_ngf32")
    net = ScoreNet(make_config(32, 32, 32), seeded_params(Dims(ngf=32, n_head_channels=32, image_size=32), 41), batch_invariant=True)
    x_T, cond = rnd(42, 2, 15, 32, 32).cuda(), rnd(43, 2, 6, 32, 32).cuda()
    noises = [rnd(100 + i, 2, 15, 32, 32) for i in range(5)]
    out = sampler.ddpm_sampler(x_T, net, cond=cond, subsample_steps=5, denoise=True, clip_before=True,
                               final_only=True, noise_fn=lambda i, x: noises[i])
    err = rel(out, g["ddpm"])
    print(f"invariant reduced-net DDPM trajectory vs reference golden: {err:.2e} (bar 5e-4)")
    assert out.shape == g["ddpm"].shape and err < 5e-4
    one = sampler.ddpm_sampler(x_T[:1].contiguous(), net, cond=cond[:1].contiguous(), subsample_steps=5, denoise=True,
                               clip_before=True, final_only=True, noise_fn=lambda i, x: noises[i][:1])
    assert torch.equal(one[-1][0], out[-1][0])


@pytest.fixture(scope="module")
def world(L):
    """The reduced network of tests/test_gpu_job_stream.py (32 / 32 / 128, DDPM-2), two ELIC models, two seeded clips."""
    from evc_amd import sampler as S, synthetic
    from evc_amd.config import default_config
    from evc_amd.decoder import ClipDecoder
    from evc_amd.elic import ElicModel
    from evc_amd.scorenet import ScoreNet
    from oracle import scorenet as ON
    cfg = default_config(32, 32, 128, subsample=2)
    net = ScoreNet(cfg, ON.seeded_params(ON.Dims(ngf=32, n_head_channels=32, image_size=128), 3))
    models = {3: ElicModel(synthetic.elic_state_dict(3)), 4: ElicModel(synthetic.elic_state_dict(4))}
    dec = ClipDecoder(net, None, cfg, S.get_sampler("DDPM"))
    clips = {v: torch.from_numpy(synthetic.make_clips(v + 1, seed=11)[v].astype(np.float32) / 255) for v in (0, 1)}
    return types.SimpleNamespace(cfg=cfg, net=net, models=models, dec=dec, clips=clips)


def test_generate_a_sample_alone_and_inside_a_batch_of_seven(world, L):
    K = (9, 12)
    others = [(1, 2), (2, 2), (9, 13), (3, 12), (8, 12), K, (9, 11)]
    g = torch.Generator(device="cuda").manual_seed(3)
    cond7 = torch.rand(7, 2, 3, 128, 128, device="cuda", generator=g)

    def nf(keys):
        keys = L.noise_keys(keys, "cuda")
        return lambda tag, shape: L.noise_normal(keys, shape, 77, 0 if tag == "init" else int(tag) + 1)
    alone = world.dec.generate(cond7[5:6].contiguous(), noise_fn=nf([K]), groups=1, invariant=True)
    batch = world.dec.generate(cond7, noise_fn=nf(others), groups=1, invariant=True)
    assert torch.equal(alone[0], batch[5])
    plain1 = world.dec.generate(cond7[5:6].contiguous(), noise_fn=nf([K]), groups=1)
    plain7 = world.dec.generate(cond7, noise_fn=nf(others), groups=1)
    print("default mode, same comparison: equal =", bool(torch.equal(plain1[0], plain7[5])))


def psnr(a, b):
    mse = float(np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2))
    return float("inf") if mse == 0 else 10 * np.log10(1.0 / mse)


def stream_of(r, vid, q, world, L):
    from evc_amd import container
    blob = container.pack_job(r["segments"], r["key_strings"], r["shape"], world.models[q].codec_tag(), r["seed"],
                              r["stream_id"], vid, q, r["thr"], "DDPM", world.cfg.sampling.subsample, world.cfg.sampling.denoise,
                              plan=(container.PLAN_INVARIANT, L.invariant_plan_revision()), crc=container.frames_crc(r["x"]))
    job = container.unpack_job(blob, expect_codec=world.models[q].codec_tag(), expect_plan_revision=L.invariant_plan_revision())
    assert job["format"] == 4
    return job


def test_invariant_sweep_any_receiver_batch_reproduces_the_sender(world, L):
    """The 56-job sweep of test_batched_sender_any_receiver_batch, generated in invariant mode at 32 jobs per launch and
    decoded at 1, 5 and 32 jobs per launch: every frame of every job equals the sender's (the default mode reaches 73 dB
    here: profiles/NOTES.md).  With the mode flag ignored this test fails at the first generated frame that differs."""
    from evc_amd import container, policy as P
    from test_gpu_job_stream import kinds_of, threshold_grid
    thr = [-100.0, 200.0] + threshold_grid(world)
    res = P.run_policy(world.dec, world.models, world.clips, [3, 4], thr, P.PsnrMetric(), max_batch=32, seed=5, bpp_limit=1e9,
                       noise="evc", batch_invariant=True)
    sent = [(vid, q, r) for vid in (0, 1) for q in (3, 4) for r in res[(vid, q)]]
    assert len(sent) == 2 * 2 * 14 and all(r["invariant"] for _, _, r in sent)
    seen = set()
    for _, _, r in sent:
        seen |= kinds_of(r["segments"])
    assert seen == {"partial", "fallback", "clip-end"}, seen
    jobs = [stream_of(r, vid, q, world, L) for vid, q, r in sent]
    for mb in (1, 5, 32):
        out = world.dec.decode_jobs(jobs, max_batch=mb, models=world.models)
        bad = []
        for (vid, q, r), job, x in zip(sent, jobs, out):
            x = x.cpu().numpy()
            if not np.array_equal(x, r["x"]):
                bad.append((vid, q, r["thr"], min(psnr(x[t], r["x"][t]) for t in range(30))))
            else:
                assert container.frames_crc(x) == job["crc"]
        print(f"receiver batch {mb}: {len(sent) - len(bad)} of {len(sent)} jobs identical to the sender's frames")
        assert not bad, (mb, bad[:4])


def chained_job(world, L, invariant):
    """key 2 + 14 x gen 2, packed by hand the way test_segmentation_matters packs programs."""
    from evc_amd import container
    from evc_amd.policy import coded_batch
    m = world.models[3]
    _, _, strings, shape = coded_batch(m, world.clips[0][:2].cuda(), 64)
    prog = [("key", 2)] + [("gen", 2)] * 14
    extra = dict(plan=(container.PLAN_INVARIANT, L.invariant_plan_revision()), crc=0) if invariant else {}
    blob = container.pack_job(prog, strings, shape, m.codec_tag(), 5, 1, 0, 3, 0.0, "DDPM", 2, True, **extra)
    return container.unpack_job(blob, expect_codec=m.codec_tag())


def test_fourteen_chained_rounds_alone_and_among_31_other_jobs(world, L):
    """The case that measures 45.6 dB in the default mode (profiles/NOTES.md): every round starts from frames the previous
    round generated, so a last-bit difference grows by about 5 dB per round.  In invariant mode the job decoded alone and in
    a batch with 31 other jobs gives the same 30 frames.  The other jobs: the same program under other noise keys and
    shorter programs, so the launch shrinks as they finish."""
    from evc_amd import container
    job = chained_job(world, L, True)
    others = []
    for k in range(31):
        o = dict(job)
        o["stream_id"] = 100 + k
        if k % 3 == 0:                       # 2 key + 5 rounds of 2 + ... : other lengths
            o["segments"] = [("key", 2)] + [("gen", 5)] * 5 + [("gen", 3)]
            o["d"] = container.check_segments(o["segments"], 30, 2)
        others.append(o)
    alone = world.dec.decode_jobs([job], models=world.models)[0]
    among = world.dec.decode_jobs(others[:17] + [job] + others[17:], max_batch=32, models=world.models)[17]
    assert alone.shape == (30, 3, 128, 128)
    per = [psnr(alone[t].cpu().numpy(), among[t].cpu().numpy()) for t in range(30)]
    print(f"14 chained rounds, alone vs among 31 jobs, invariant mode: min PSNR {min(per)} dB")
    assert torch.equal(alone, among)


# ---- the command lines ------------------------------------------------------------------------------------------

def test_invariant_sender_then_receivers_in_fresh_processes(tmp_path, L):
    from evc_amd import container
    out, bits = tmp_path / "out", tmp_path / "bits"
    model = ["--config", os.path.join(REPO, "configs", "mine.yml"), "--synthetic", "--exp", str(tmp_path / "exp"),
             "--config_mod", "model.ngf=32 model.n_head_channels=32", "--data_npy", "missing.npy"]
    thresholds = [200.0, 6.91, -100.0]      # all key frames; chained short rounds; everything accepted
    send = [sys.executable, os.path.join(REPO, "city_sender.py")] + model + [
        "--output_path", str(out), "--start_idx", "0", "--end_idx", "0", "--subsample", "2", "--q", "3", "--policy", "psnr",
        "--thresholds"] + [str(t) for t in thresholds] + ["--bpp-limit", "1e9", "--bitstream-dir", str(bits)]
    s = subprocess.run(send + ["--batch-invariant"], cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert s.returncode == 0, s.stdout + s.stderr
    names = [container.job_file_name(0, 3, t) for t in thresholds]
    assert sorted(os.listdir(bits)) == sorted(names)
    for n in names:
        assert (bits / n).read_bytes()[4] == 4
    recv = [sys.executable, os.path.join(REPO, "city_receiver.py")] + model + ["--bitstream-dir", str(bits)]
    for batch in (1, 32):
        rx = tmp_path / f"rx{batch}"
        r = subprocess.run(recv + ["--output_path", str(rx), "--batch", str(batch)], cwd=tmp_path, capture_output=True,
                           text=True, timeout=900)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.count("frames: match") == 3 and "MISMATCH" not in r.stdout, r.stdout
        for t in thresholds:
            x = np.load(rx / ("decoded_v0_q3_thr%.2f.npy" % t))
            job = container.unpack_job((bits / container.job_file_name(0, 3, t)).read_bytes())
            assert container.frames_crc(x) == job["crc"]
            img = np.load(out / "output_0" / ("city_output_npy_idx0_q3_thr%.2f.npy" % t))[128:]     # lower half: decoded frames
            if img.dtype == np.float32:
                sender = np.stack([img[:, f * 128:(f + 1) * 128].transpose(2, 0, 1) for f in range(30)])
                if container.frames_crc(sender) == job["crc"]:       # the saved array holds the frames unaltered
                    assert np.array_equal(x, sender), t
    # one byte of a stored CRC flipped: MISMATCH and a non-zero status
    broken = tmp_path / "broken"
    broken.mkdir()
    blob = bytearray((bits / names[1]).read_bytes())
    crc_at = 8 + __import__("struct").calcsize(container._JOB_HEAD) + 3
    blob[crc_at] ^= 0x40
    (broken / names[1]).write_bytes(bytes(blob))
    r = subprocess.run(recv[:-1] + [str(broken), "--output_path", str(tmp_path / "rxb")], cwd=tmp_path, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode != 0 and "frames: MISMATCH" in r.stdout, r.stdout + r.stderr
    # a format-3 directory decodes as before: no verdict line, status 0
    bits3 = tmp_path / "bits3"
    s = subprocess.run(send[:-1] + [str(bits3), "--output_path", str(tmp_path / "out3")], cwd=tmp_path, capture_output=True,
                       text=True, timeout=900)
    assert s.returncode == 0, s.stdout + s.stderr
    assert all((bits3 / n).read_bytes()[4] == 3 for n in names)
    r = subprocess.run(recv[:-1] + [str(bits3), "--output_path", str(tmp_path / "rx3")], cwd=tmp_path, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "frames:" not in r.stdout, r.stdout + r.stderr
