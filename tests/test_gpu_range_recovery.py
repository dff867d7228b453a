"""GPU tests of the per-layer range recovery: per-site attribution of the fp16-split range events (evc_*_site_f32),
``ScoreNet.demote`` (exact against a network built demoted), chunk replay through ``ClipDecoder`` (bit-identical to the
demoted network on the same noise), the cascade of hidden overflows, the refusals, and the CLI flag end to end.

"Overflowing" networks are the seeded ones with one act-norm's AdaGN projection (Dense_0: scale and shift rows) multiplied
by a large factor -- what a trained checkpoint with large ``(1 + scale)`` rows looks like to the range test."""
import os
import time

import numpy as np
import pytest
import torch

from conftest import rnd

pytestmark = pytest.mark.gpu

BIG = 1e5          # AdaGN factor: |shift| alone is far beyond fp16's operand limit 65504 / 8
UP, DOWN = 13, 30  # res-blocks of the ngf=32 / 32x32 program with a 1x1 skip convolution: one in the encoder, one in the decoder


def setup_module(module):
    import evc_amd  # noqa: F401
    from evc_amd import lib as L
    L.hip_lib()


@pytest.fixture(autouse=True)
def clean_events():
    from evc_amd import lib as L
    L.range_events(reset=True)
    yield
    L.range_events(reset=True)


def params(seed, inflate=()):
    from oracle.scorenet import Dims, seeded_params
    d = Dims(ngf=32, n_head_channels=32, image_size=32)
    p = seeded_params(d, seed)
    for i in inflate:
        for k in (f"unet.all_modules.{i}.actnorm1.Dense_0.weight", f"unet.all_modules.{i}.actnorm1.Dense_0.bias"):
            p[k] = p[k] * BIG
    return p


def config(subsample=None):
    from evc_amd.config import default_config
    return default_config(32, 32, 32) if subsample is None else default_config(32, 32, 32, subsample=subsample)


def net_of(p, **kw):
    from evc_amd.scorenet import ScoreNet
    return ScoreNet(config(), p, **kw)


def site(net, tag, module):
    return next(s["site"] for s in net.sites if s["tag"] == tag and s["module"] == module)


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max())


def inputs():
    return rnd(92, 2, 15, 32, 32).cuda(), rnd(93, 2, 6, 32, 32).cuda()


def test_site_attribution_names_the_overflowing_block():
    from evc_amd import lib as L
    x, cond = inputs()
    clean = net_of(params(91))
    L.site_events(clean, reset=True)
    clean.forward_label(x, 500, cond)
    assert L.site_events(clean, reset=True) == {} and L.range_events(reset=True) == 0
    assert int(clean.site_words.abs().sum()) == 0

    net = net_of(params(91, inflate=[UP]))
    L.site_events(net, reset=True)
    net.forward_label(x, 500, cond)
    ev = L.site_events(net)
    glob = L.range_events(reset=True)
    s = site(net, "res1", UP)
    assert {k for k, b in ev.items() if b & L.RANGE_F16_OPERAND} == {s}, ev
    # whatever else reported is the NaN of that overflow, downstream of it
    assert all(b == L.RANGE_NONFINITE and k > s for k, b in ev.items() if k != s), ev
    acc = 0
    for b in ev.values():
        acc |= b
    assert glob == acc and glob & L.RANGE_F16_OPERAND
    assert L.site_events(net, reset=True) == ev and L.site_events(net) == {}       # one read, then cleared


def test_site_exports_raise_both_words_and_nothing_when_clean():
    """The bare exports: the same condition raises the device word and site_events[site]; a clean call touches neither."""
    from evc_amd import lib as L
    torch.manual_seed(0)
    x = torch.randn(2, 8, 8, 32, device="cuda")
    part = L.chan_stats(x)
    words = L.site_word_arena(4, x.device)
    gamma, beta = torch.ones(32, device="cuda"), torch.zeros(32, device="cuda")
    L.gn_coeffs([part], 64, 8, 1e-5, mode=1, gamma=gamma, beta=beta, site=L.Site(words, 1))
    b = torch.zeros(3, dtype=torch.int32, device="cuda")
    L.moments_bound(part, 0, 8, b, site=L.Site(words, 2))
    assert L.range_events() == 0 and words.tolist() == [0, 0, 0, 0]
    L.gn_coeffs([part], 64, 8, 1e-5, mode=1, gamma=gamma * 1e6, beta=beta, site=L.Site(words, 1))
    assert L.range_events(reset=True) == L.RANGE_F16_OPERAND and words.tolist() == [0, L.RANGE_F16_OPERAND, 0, 0]
    L.gn_coeffs([part], 64, 8, 1e-5, mode=1, gamma=gamma * 1e6, beta=beta, site=L.Site(words, 3, quiet=True))
    assert L.range_events() == 0 and words[3].item() == L.RANGE_F16_OPERAND       # quiet: site word only
    x[1, 2, 3, 5] = float("nan")
    part = L.chan_stats(x)
    words.zero_()
    L.moments_bound(part, 0, 8, b, site=L.Site(words, 2))
    assert L.range_events(reset=True) == L.RANGE_NONFINITE and words.tolist() == [0, 0, L.RANGE_NONFINITE, 0]


@pytest.mark.parametrize("graphs", [False, True])
def test_demote_is_exact(graphs):
    from evc_amd import lib as L
    x, cond = inputs()
    p = params(91, inflate=[UP])
    net = net_of(p, use_graphs=graphs)
    net.forward_label(x, 500, cond)                      # overflows (and, with graphs, captures a graph)
    L.range_events(reset=True)
    S = [site(net, "res1", UP)]
    t0 = time.perf_counter()
    assert net.demote(S) == S
    print(f"demote: {1e3 * (time.perf_counter() - t0):.2f} ms for {net.demoted_sites()}")
    assert not net._graphs
    L.site_events(net, reset=True)
    out = net.forward_label(x, 500, cond).clone()
    assert L.range_events(reset=True) == 0
    assert all(k in S for k in L.site_events(net, reset=True))       # only the (quiet) demoted site may still report
    ref = net_of(p, demote=S).forward_label(x, 500, cond)
    L.range_events(reset=True)
    assert torch.equal(out, ref)
    if graphs:
        assert len(net._graphs) == 1
        assert torch.equal(net.forward_label(x, 500, cond), ref)     # replay of the recaptured graph
    old = os.environ.get("EVC_CONV_ARITH")
    try:
        os.environ["EVC_CONV_ARITH"] = "bf16x6"
        n6 = net_of(p)
    finally:
        if old is None:
            os.environ.pop("EVC_CONV_ARITH", None)
        else:
            os.environ["EVC_CONV_ARITH"] = old
    o6 = n6.forward_label(x, 500, cond)
    L.range_events(reset=True)
    assert bool(torch.isfinite(out).all()) and rel(out, o6) < 2e-4


def decoder(net, recovery, lines=None, groups=1):
    from evc_amd import sampler as S
    from evc_amd.decoder import ClipDecoder
    return ClipDecoder(net, None, config(subsample=3), S.get_sampler("DDPM"), groups=groups, range_recovery=recovery,
                       log=(lines.append if lines is not None else print))


def cond_frames(seed=5):
    return torch.from_numpy(np.random.default_rng(seed).random((2, 2, 3, 32, 32), dtype=np.float32)).cuda()


@pytest.mark.parametrize("groups", [1, 2])
def test_chunk_replay_is_exact(groups):
    from evc_amd import lib as L
    p = params(91, inflate=[UP])
    net = net_of(p)
    lines = []
    dec = decoder(net, "layer", lines, groups)
    t0 = time.perf_counter()
    out = dec.generate(cond_frames(), generator=torch.Generator(device="cuda").manual_seed(11))
    t_chunk = time.perf_counter() - t0
    assert L.range_events() == 0
    assert bool(torch.isfinite(out).all())
    demoted = net.demoted_sites()
    assert site(net, "res1", UP) in demoted and dec.recovery_passes == [2]
    assert len(lines) == 1 and demoted[site(net, "res1", UP)] in lines[0] and "chunk 1" in lines[0]
    print(f"replayed chunk: {t_chunk * 1e3:.1f} ms in all, repack {net.demote_seconds * 1e3:.2f} ms ({lines[0]})")
    ref_net = net_of(p, demote=list(demoted))
    ref = decoder(ref_net, "off", groups=groups).generate(cond_frames(), generator=torch.Generator(device="cuda").manual_seed(11))
    assert L.range_events(reset=True) == 0
    assert torch.equal(out, ref)
    # the next chunk of the recovered network is clean at once
    dec.generate(cond_frames(6), generator=torch.Generator(device="cuda").manual_seed(12))
    assert dec.recovery_passes == [2] and net.demoted_sites() == demoted


def test_cascade_needs_several_passes():
    from evc_amd import lib as L
    p = params(91, inflate=[UP, DOWN])
    net = net_of(p)
    lines = []
    dec = decoder(net, "layer", lines)
    out = dec.generate(cond_frames(), generator=torch.Generator(device="cuda").manual_seed(11))
    assert L.range_events() == 0 and bool(torch.isfinite(out).all())
    assert {site(net, "res1", UP), site(net, "res1", DOWN)} <= set(net.demoted_sites())
    assert dec.recovery_passes[0] >= 3          # the upstream NaN hides the downstream overflow for one pass
    assert len(lines) == 1
    ref = decoder(net_of(p, demote=list(net.demoted_sites())), "off").generate(
        cond_frames(), generator=torch.Generator(device="cuda").manual_seed(11))
    assert torch.equal(out, ref)


def test_refusals():
    from evc_amd import cli, lib as L
    # a NaN in the conditioning frames: no site to demote, refused, nothing demoted
    net = net_of(params(91))
    c = cond_frames()
    c[1, 0, 2, 7, 7] = float("nan")
    with pytest.raises(cli.NumericsError, match="no site left to demote"):
        decoder(net, "layer").generate(c, generator=torch.Generator(device="cuda").manual_seed(11))
    assert net.demoted_sites() == {}
    L.range_events(reset=True)
    # recovery off: the overflowing network stops the run exactly as before
    bad = net_of(params(91, inflate=[UP]))
    frames = decoder(bad, "off").generate(cond_frames(), generator=torch.Generator(device="cuda").manual_seed(11))
    assert bad.demoted_sites() == {}
    with pytest.raises(cli.NumericsError, match="EVC_CONV_ARITH=bf16x6"):
        cli.check_numerics(frames, "chunk")


def test_cli_range_recovery_end_to_end(tmp_path, monkeypatch, capsys):
    import evc_amd  # noqa: F401
    from evc_amd import cli, config as C
    from evc_amd.scorenet import build_program, dims_from_config
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.chdir(tmp_path)
    mods = "model.ngf=32 model.n_head_channels=32"
    cfg, _ = C.load_config(os.path.join(repo, "configs", "mine.yml"), mods)
    prog = build_program(dims_from_config(cfg))
    blk = next(i for i, m in enumerate(prog) if m["kind"] == "res" and m["cin"] != m["cout"])
    monkeypatch.setenv("EVC_SYNTHETIC_ADAGN_SCALE", f"all_modules.{blk}.actnorm1={BIG}")
    monkeypatch.delenv("EVC_RANGE_RECOVERY", raising=False)
    out = tmp_path / "out"
    base = ["--config", os.path.join(repo, "configs", "mine.yml"), "--synthetic", "--exp", str(tmp_path / "exp"),
            "--data_npy", "missing.npy", "--output_path", str(out), "--start_idx", "0", "--end_idx", "0",
            "--subsample", "2", "--q", "3", "--config_mod", mods]
    capsys.readouterr()
    cli.main(base + ["--range-recovery", "layer"])
    log = capsys.readouterr().out
    assert f"demoted all_modules.{blk}.Conv_1" in log and "range recovery: chunk 1" in log, log
    arr = np.load(out / "output_0" / "city_output_npy_idx0_q3_thr0.00.npy")
    assert arr.shape == (2 * 128, 30 * 128, 3) and np.isfinite(arr).all()
    with pytest.raises(cli.NumericsError, match="EVC_CONV_ARITH=bf16x6"):
        cli.main(base)
