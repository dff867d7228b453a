"""CPU tests of the per-layer range recovery (recovery.py, ScoreNet.demote): the pass loop's termination rules on a fake
network, and the score network's event-site table against the packs it actually makes (weights packed by a stand-in that
only records the arithmetic)."""
import os

import pytest
import torch

import evc_amd  # noqa: F401
from evc_amd import cli, config as C, lib as L, recovery as R, synthetic
from evc_amd.scorenet import ScoreNet, range_sites

F16, NF = R.RANGE_F16_OPERAND, R.RANGE_NONFINITE


class FakeNet:
    def __init__(self, n_sites):
        self.sites = [dict(site=k, name=f"m{k}") for k in range(n_sites)]
        self._demoted = []
        self.demote_calls = []

    def demote(self, sites):
        self.demote_calls.append(list(sites))
        self._demoted += [k for k in sites if k not in self._demoted]

    def demoted_sites(self):
        return {k: f"m{k}" for k in sorted(self._demoted)}


def drive(net, script, finite=None):
    """Run the pass loop against scripted (site words, device word) reads; returns (passes, restores, log lines)."""
    reads = iter(script)
    finite = iter(finite or [True] * len(script))
    restores, lines = [], []

    def run():
        return torch.zeros(2) if next(finite) else torch.tensor([0.0, float("nan")])

    def restore():
        restores.append(1)

    _, passes, new = R.generate_with_recovery(run, restore, net, where="chunk 1", log=lines.append, read=lambda: next(reads))
    return passes, new, len(restores), lines


def test_clean_chunk_takes_one_pass_and_demotes_nothing():
    net = FakeNet(4)
    assert drive(net, [({}, 0)]) == (1, [], 0, [])
    assert net.demote_calls == []


def test_cascade_demotes_until_clean_and_logs_once():
    net = FakeNet(6)
    # pass 1: site 1 overflows, its NaN makes the later sites report non-finite; pass 2: site 4 overflows; pass 3: clean
    script = [({1: F16, 2: NF, 3: NF, 4: NF}, F16 | NF), ({4: F16, 5: NF}, F16 | NF), ({}, 0)]
    passes, new, restores, lines = drive(net, script, finite=[False, False, True])
    assert (passes, new, restores) == (3, [1, 4], 2)
    assert net.demote_calls == [[1], [4]]
    assert len(lines) == 1 and "m1 (site 1)" in lines[0] and "m4 (site 4)" in lines[0] and "3 passes" in lines[0]


def test_several_sites_in_one_pass_are_demoted_together():
    net = FakeNet(5)
    passes, new, _, _ = drive(net, [({0: F16, 3: F16 | NF}, F16 | NF), ({}, 0)])
    assert (passes, new) == (2, [0, 3]) and net.demote_calls == [[0, 3]]


def test_a_demoted_site_that_still_reports_is_not_a_new_site():
    net = FakeNet(3)
    net.demote([2])
    net.demote_calls.clear()
    # a demoted site keeps reporting to its own word (not the device word): accepted as clean
    assert drive(net, [({2: F16}, 0)])[:2] == (1, [])
    assert net.demote_calls == []


def test_nonfinite_without_an_overflowing_site_is_refused():
    net = FakeNet(3)
    with pytest.raises(cli.NumericsError, match="no site left to demote"):
        drive(net, [({0: NF, 1: NF, 2: NF}, NF)], finite=[False])
    assert net.demote_calls == []


def test_a_pass_that_demotes_nothing_new_is_refused():
    net = FakeNet(3)
    with pytest.raises(R.NumericsError):
        drive(net, [({1: F16}, F16), ({1: F16, 2: NF}, NF)])     # site 1 demoted, chunk still non-finite: no new site
    assert net.demote_calls == [[1]]


def test_device_word_or_nan_frames_alone_are_refused():
    with pytest.raises(R.NumericsError):
        drive(FakeNet(2), [({}, NF)])
    with pytest.raises(R.NumericsError):
        drive(FakeNet(2), [({}, 0)], finite=[False])


def test_recovery_mode_and_cli_flag(monkeypatch):
    monkeypatch.delenv("EVC_RANGE_RECOVERY", raising=False)
    assert R.recovery_mode() == "off" and R.recovery_mode("layer") == "layer"
    monkeypatch.setenv("EVC_RANGE_RECOVERY", "layer")
    assert R.recovery_mode() == "layer" and R.recovery_mode("off") == "off"
    monkeypatch.setenv("EVC_RANGE_RECOVERY", "bogus")
    with pytest.raises(ValueError):
        R.recovery_mode()
    p = cli.build_parser()
    assert p.parse_args([]).range_recovery is None
    assert p.parse_args(["--range-recovery", "layer"]).range_recovery == "layer"
    with pytest.raises(SystemExit):
        p.parse_args(["--range-recovery", "all"])
    assert cli.NumericsError is R.NumericsError
    assert not R.supports_recovery(object()) and R.supports_recovery(FakeNet(1))


def _host_net(monkeypatch, mods="", cls=ScoreNet):
    """A ScoreNet built on the host: packing only records the arithmetic (dtype) each weight would get."""
    monkeypatch.delenv("EVC_CONV_ARITH", raising=False)
    monkeypatch.setattr(L, "hip_lib", lambda require_device=True: None)
    monkeypatch.setattr(L, "conv_pack_weights", lambda w, arith=None: torch.empty(1, dtype=L._ARITH_DTYPES[arith]))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: None)
    cfg, _ = C.load_config(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs",
                                        "mine.yml"), "model.ngf=32 model.n_head_channels=32 " + mods)
    sd = synthetic.diffusion_state_dict(cfg, 0)
    return cls(cfg, sd, device="cpu")


@pytest.mark.parametrize("mods", ["", "model.spade=True"])
def test_site_table_covers_every_fp16_split_pack_exactly_once(monkeypatch, mods):
    if "spade" in mods:
        from evc_amd.scorenet_spade import SpadeScoreNet as cls
    else:
        cls = ScoreNet
    net = _host_net(monkeypatch, mods, cls)
    f16 = {(i, k) for i, e in net.w.items() for k, v in e.items()
           if torch.is_tensor(v) and L.packed_arith(v) == L.ARITH_F16X3}
    assert f16 and f16 <= set(net._wsrc)
    covered = [c for st in net.sites for c in st["consumers"] if c[1] != "attention"]
    assert len(covered) == len(set(covered))                          # no pack guarded by two sites
    assert f16 <= set(covered)                                        # every fp16-split pack guarded by one
    assert all(k in net.w[i] for i, k in covered)
    # one site per coefficient / bound call: 2 per res-block, 2 per attention block, the final norm
    kinds = [m["kind"] for m in net.program]
    assert len(net.sites) == 2 * kinds.count("res") + 2 * kinds.count("attn") + kinds.count("norm")
    assert [st["site"] for st in net.sites] == list(range(len(net.sites)))
    res = next(i for i, m in enumerate(net.program) if m["kind"] == "res")
    assert net.sites[1]["name"] == f"all_modules.{res}.Conv_1"
    assert net.sites[-1]["name"] == f"all_modules.{len(net.program) - 1}"     # the output convolution
    # demoting every site leaves no fp16-split pack, no fp16 attention, no fused skip
    net.demote(range(len(net.sites)))
    assert not any(torch.is_tensor(v) and L.packed_arith(v) == L.ARITH_F16X3 for e in net.w.values() for v in e.values())
    attn = {i for i, m in enumerate(net.program) if m["kind"] == "attn"}
    assert net._attn_f32 == attn
    assert net._unfused == {i for i, m in enumerate(net.program) if m["kind"] == "res"}
    assert set(net.demoted_sites()) == set(range(len(net.sites)))


def test_demote_by_name_is_sticky_and_repacks_only_its_consumers(monkeypatch):
    net = _host_net(monkeypatch)
    st = next(s for s in net.sites if s["tag"] == "res1" and len(s["consumers"]) == 2)
    i = st["module"]
    before = {k: net.w[i][k] for k in ("w0", "w1", "w2")}
    net._graphs["x"] = object()
    assert net.demote([st["name"]]) == [st["site"]]
    assert L.packed_arith(net.w[i]["w1"]) == L.ARITH_BF16X6 and L.packed_arith(net.w[i]["w2"]) == L.ARITH_BF16X6
    assert net.w[i]["w0"] is before["w0"] and i in net._unfused and not net._graphs
    assert net._site_of[("res1", i)].quiet and not net._site_of[("res0", i)].quiet
    assert net.demote([st["site"]]) == []                              # already demoted: nothing to do
    assert net.demoted_sites() == {st["site"]: st["name"]}
    with pytest.raises(KeyError):
        net.demote(["all_modules.999.Conv_0"])


def test_constructor_demote_matches_later_demote(monkeypatch):
    a = _host_net(monkeypatch)
    names = [a.sites[0]["name"], a.sites[-1]["name"]]
    a.demote(names)
    cfg = a.config
    b = ScoreNet(cfg, synthetic.diffusion_state_dict(cfg, 0), device="cpu", demote=names)
    assert a.demoted_sites() == b.demoted_sites()
    assert {(i, k): v.dtype for i, e in a.w.items() for k, v in e.items() if torch.is_tensor(v)} == \
        {(i, k): v.dtype for i, e in b.w.items() for k, v in e.items() if torch.is_tensor(v)}


def test_range_sites_of_the_program_alone():
    from evc_amd.scorenet import build_program
    from oracle.scorenet import Dims
    prog = build_program(Dims(ngf=32, n_head_channels=32, image_size=32))
    sites = range_sites(prog)
    tags = {s["tag"] for s in sites}
    assert tags == {"res0", "res1", "attn_norm", "attn_qkv", "norm"}
    assert all(s["consumers"] for s in sites)
    # with cond_emb the reference's module list has the Embedding at index 2: every later name is one higher
    shifted = range_sites(prog, cond_emb=True)
    assert [s["consumers"] for s in shifted] == [s["consumers"] for s in sites]
    res = sites[0]["module"]
    assert sites[0]["name"] == f"all_modules.{res}.Conv_0" and shifted[0]["name"] == f"all_modules.{res + 1}.Conv_0"
    assert shifted[-1]["name"] == f"all_modules.{len(prog)}"


def test_synthetic_adagn_inflation():
    cfg, _ = C.load_config(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs",
                                        "mine.yml"), "model.ngf=32 model.n_head_channels=32")
    sd = synthetic.diffusion_state_dict(cfg, 0)
    big = synthetic.inflate_adagn(dict(sd), "all_modules.5.actnorm1=1000")
    k = "unet.all_modules.5.actnorm1.Dense_0.weight"
    assert torch.equal(big[k], sd[k] * 1000.0) and torch.equal(big["unet.all_modules.5.actnorm0.Dense_0.weight"],
                                                                sd["unet.all_modules.5.actnorm0.Dense_0.weight"])
    with pytest.raises(KeyError):
        synthetic.inflate_adagn(dict(sd), "all_modules.0.actnorm1=2")
