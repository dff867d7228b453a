"""Host side of the ELIC rate estimate (--entropy-estimation): the density parameters of the entropy bottleneck -- the
synthetic ones, their packing for evc_bottleneck_rate_f32, the two state-dict spellings -- and the CLI's refusal of
--bitstream-dir.  The float64 formulas are those of tests/elic_rate_ref.py."""
import os

import numpy as np
import pytest
import torch

import elic_rate_ref as R

import evc_amd  # noqa: F401
from evc_amd import entropy, synthetic


def _sigmoid(v):
    return 1 / (1 + np.exp(-v))


def test_zero_factor_density_is_the_logistic():
    """Factors 0, positive matrices whose product down the chain is 1/s, last bias -med/s: the factorised density of the symbol
    k is sigmoid((k + 1/2 - med) / s) - sigmoid((k - 1/2 - med) / s), in float64 to rounding."""
    rng = np.random.default_rng(0)
    s = 0.5 + 2.5 * rng.random(12)
    med = 0.3 * rng.standard_normal(12)
    raw = entropy.logistic_density_params(s, med, dtype=torch.float64)
    assert all(float(f.abs().max()) == 0.0 for f in raw[2])
    k = np.arange(-40, 41, dtype=np.float64)
    x = torch.from_numpy(med[:, None] + k[None, :])                     # (C, n): the dequantised values k + med
    logits = R.logits_cumulative(x, *raw, torch.float64).numpy()
    np.testing.assert_allclose(logits, k[None, :] / s[:, None], rtol=0, atol=1e-13)       # (x - med) / s
    # sigmoid(b) - sigmoid(a) of the negative arguments: the form that does not cancel in the right tail
    a, b = -(np.abs(k)[None, :] + 0.5) / s[:, None], -(np.abs(k)[None, :] - 0.5) / s[:, None]
    want = _sigmoid(b) - _sigmoid(a)
    got = R.density(x, *raw, torch.float64).numpy()
    # where lower + upper is exactly 0 the formula's sign is 0 and the likelihood 0 (compressai's own behaviour; the kernel
    # follows it): that can only happen at the symbol 0, when the rounding of med + k - med is symmetric
    lo = R.logits_cumulative(x - 0.5, *raw, torch.float64).numpy()
    up = R.logits_cumulative(x + 0.5, *raw, torch.float64).numpy()
    sym0 = (lo + up) == 0
    assert not sym0[:, k != 0].any() and (got[sym0] == 0).all()
    np.testing.assert_allclose(got[~sym0], want[~sym0], rtol=1e-11, atol=0)


def test_density_variant_shares_every_tensor_with_the_plain_checkpoint():
    plain = synthetic.elic_state_dict(3)
    dens = synthetic.elic_state_dict_with_density(3)
    assert set(plain) < set(dens)
    assert all(torch.equal(plain[k], dens[k]) for k in plain)
    extra = sorted(set(dens) - set(plain))
    assert extra == sorted([f"entropy_bottleneck._matrix{i}" for i in range(5)] + [f"entropy_bottleneck._bias{i}" for i in range(5)] +
                           [f"entropy_bottleneck._factor{i}" for i in range(4)])
    assert tuple(dens["entropy_bottleneck._matrix1"].shape) == (192, 3, 3)
    assert tuple(dens["entropy_bottleneck._bias4"].shape) == (192, 1, 1)


def test_density_matches_the_tables_within_the_quantisers_rounding():
    """Per channel 65536 p(k) of the density against the frequency the table gives the symbol k, over the table's support.
    ``pmf_to_quantized_cdf`` (csrc/rans.cpp) makes that frequency from the pmf in four steps, each with a bound of its own:
    lround(65536 pmf) (1/2, and 0.01 for the pmf going in as float32); rescaling by 65536 / total with floor (total is within
    (n + 1) / 2 of 65536, n + 1 entries rounded: f (n + 1) / (2 * 65536 - (n + 1)), and 1 for the floor); and one count stolen
    per symbol whose frequency came out 0 -- each of those ends at frequency 1, so their number is at most the number Z of
    frequency-1 symbols of the finished table."""
    sd = synthetic.elic_state_dict_with_density(3)
    raw, missing = entropy.density_from_state_dict(sd)
    assert not missing
    cdf = sd["entropy_bottleneck._quantized_cdf"].numpy().astype(np.int64)
    length = sd["entropy_bottleneck._cdf_length"].numpy().reshape(-1)
    offset = sd["entropy_bottleneck._offset"].numpy().reshape(-1)
    med = sd["entropy_bottleneck.quantiles"][:, 0, 1].double()
    worst = 0.0
    for c in range(cdf.shape[0]):
        n = int(length[c]) - 2                                            # symbols of the support (the last entry is the tail)
        freq = np.diff(cdf[c, :n + 1]).astype(np.float64)
        k = np.arange(n, dtype=np.float64) + offset[c]
        x = (med[c] + torch.from_numpy(k))[None, :]
        p = R.density(x, *[[t[c:c + 1] for t in grp] for grp in raw], torch.float64).numpy()[0]
        z = float((np.diff(cdf[c, :n + 2]) == 1).sum())
        bound = 0.5 + 0.01 + 1.0 + freq * (n + 1) / (2 * 65536 - (n + 1)) + z
        err = np.abs(65536.0 * p - freq)
        assert (err <= bound).all(), (c, float(err.max()), float(bound.min()))
        worst = max(worst, float((err - z).max()))
    assert worst < 3.0          # away from the stolen counts the table IS the density to a count or two


def test_packing_round_trips():
    rng = np.random.default_rng(5)
    C = 7
    t = lambda *shape: torch.from_numpy(rng.standard_normal(shape))
    F = entropy.EB_FILTERS
    mats = [t(C, F[i + 1], F[i]) for i in range(5)]
    bias = [t(C, F[i + 1], 1) for i in range(5)]
    fact = [t(C, F[i + 1], 1) for i in range(4)]
    table = entropy.pack_density(mats, bias, fact)
    assert table.shape == (C, 58) and table.dtype == torch.float32 and entropy.DENSITY_FLOATS == 58
    m2, b2, f2 = entropy.unpack_density(table)
    for i in range(5):
        assert torch.equal(m2[i], torch.nn.functional.softplus(mats[i]).float())          # float64 transform, rounded once
        assert torch.equal(b2[i], bias[i].float())
    for i in range(4):
        assert torch.equal(f2[i], torch.tanh(fact[i]).float())
    # the layout the kernel reads: 3+3+3, then 9+3+3 three times, then 3+1; matrices row-major [out][in]
    assert torch.equal(table[:, 0:3], m2[0].reshape(C, 3)) and torch.equal(table[:, 6:9], f2[0].reshape(C, 3))
    assert float(table[2, 9 + 3 * 1 + 2]) == float(m2[1][2, 1, 2])
    assert torch.equal(table[:, 54:57], m2[4].reshape(C, 3)) and torch.equal(table[:, 57], b2[4].reshape(C))


def _bare_model(sd):
    """An ElicModel that only went through the density part of its constructor (the rest needs a GPU)."""
    from evc_amd.elic import ElicModel
    m = ElicModel.__new__(ElicModel)
    m.device = torch.device("cpu")
    m._load_density(sd)
    return m


def test_both_key_spellings_load_and_missing_keys_fail_in_estimate_only():
    a = synthetic.elic_state_dict_with_density(4)
    b = synthetic.elic_state_dict_with_density(4, naming="later")
    assert "entropy_bottleneck._matrix0" in a and "entropy_bottleneck.matrices.0" in b and "entropy_bottleneck._matrix0" not in b
    ma, mb = _bare_model(a), _bare_model(b)
    assert ma.density.shape == (192, 58) and torch.equal(ma.density, mb.density)
    plain = synthetic.elic_state_dict(4)
    m = _bare_model(plain)                                   # loads: coding needs the tables only
    assert m.density is None
    with pytest.raises(entropy.DensityParametersMissing) as e:
        m.estimate(torch.zeros(1, 3, 64, 64))
    assert "entropy_bottleneck._matrix0" in str(e.value) and "entropy_bottleneck._factor3" in str(e.value)
    del a["entropy_bottleneck._bias2"]                       # one key short: named alone
    with pytest.raises(entropy.DensityParametersMissing) as e:
        _bare_model(a).estimate(torch.zeros(1, 3, 64, 64))
    assert "_bias2" in str(e.value) and "_matrix0" not in str(e.value)


def test_cli_refuses_estimation_with_a_bitstream_dir(tmp_path, monkeypatch, capsys):
    from evc_amd import cli
    monkeypatch.chdir(tmp_path)
    d = tmp_path / "d"
    with pytest.raises(SystemExit) as e:
        cli.main(["--synthetic", "--entropy-estimation", "--bitstream-dir", str(d), "--exp", str(tmp_path / "exp"),
                  "--output_path", str(tmp_path / "out")])
    assert isinstance(e.value.code, str) and "--entropy-estimation" in e.value.code and "--bitstream-dir" in e.value.code
    assert os.listdir(tmp_path) == []                        # nothing was created: no stream dir, no exp dir, no output
