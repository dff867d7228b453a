"""GPU tests of the ELIC rate estimate (csrc/rate.hip, ElicModel.estimate, --entropy-estimation) against the float64
restatement tests/elic_rate_ref.py.

Tolerance of the bit sums.  The yardstick is the same formula evaluated by torch in float32 on the CPU, against float64, on
the very inputs of the case: e_sym, its largest per-symbol difference, and e_sum, its largest relative difference of a sample's
total.  The kernels may be 4 x as far from float64, no more.  Measured figures are kept in profiles/NOTES.md."""
import os

import numpy as np
import pytest
import torch

import elic_rate_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678


def _report(what, gpu, e_gpu, e_cpu):
    print(f"[elic-rate] {what}: gpu {e_gpu:.3e}  cpu-fp32 yardstick {e_cpu:.3e}  bound {4 * e_cpu:.3e}  ({gpu})")


def check_totals(what, got, bits64, bits32, dims):
    """got: (B,) float64 totals of the kernel; bits64 / bits32: per-symbol restatements (0 where a site is not of the pass)."""
    e_sym, e_sum = R.yardstick(bits64, bits32, dims)
    want = bits64.sum(dims)
    rel = float(((got - want).abs() / want.abs()).max())
    _report(what + " e_sum", f"e_sym cpu {e_sym:.3e}", rel, e_sum)
    assert rel <= 4 * e_sum, (what, rel, e_sum)


# ---- rate pass, kernel level ---------------------------------------------------------------------------------------------------
def pass_inputs(seed, B, C, H, W):
    """ms (B, H, W, ld) with ld > 2C and the means / scales at non-zero offsets, y (B, H, W, ld_y) with the slice at c0 > 0.
    Scales log-uniform over [0.02, 64]; y - mu mostly within a few sigma; at the pixels (0, 0) (an anchor) and (0, 1) (a
    non-anchor) of every sample: exact .5 ties (round half to even, up and down) and outliers far beyond the 1e-9 floor."""
    rng = np.random.default_rng(seed)
    mean_off, scale_off, c0 = 3, 5 + C, 2
    ld, ld_y = 2 * C + 9, C + 7
    ms = rng.standard_normal((B, H, W, ld)).astype(np.float32)
    y = rng.standard_normal((B, H, W, ld_y)).astype(np.float32)
    mu = (3 * rng.standard_normal((B, H, W, C))).astype(np.float32)
    sigma = np.exp(rng.uniform(np.log(0.02), np.log(64.0), (B, H, W, C))).astype(np.float32)
    yc = (mu + np.maximum(sigma, 0.11) * 1.5 * rng.standard_normal((B, H, W, C)).astype(np.float32)).astype(np.float32)
    for w in (0, 1):
        mu[:, 0, w, 0:2] = 1.25
        yc[:, 0, w, 0] = 3.75                  # y - mu = 2.5 -> 2
        yc[:, 0, w, 1] = 4.75                  # y - mu = 3.5 -> 4
        if C > 4:
            mu[:, 0, w, 4] = -0.75
            yc[:, 0, w, 4] = -1.25             # y - mu = -0.5 -> -0
        sigma[:, 0, w, 2:4] = (0.05, 2.0)
        yc[:, 0, w, 2] = mu[:, 0, w, 2] + 9.0           # 9 / 0.11 sigma
        yc[:, 0, w, 3] = mu[:, 0, w, 3] - 40.0          # 20 sigma
    ms[..., mean_off:mean_off + C] = mu
    ms[..., scale_off:scale_off + C] = sigma
    y[..., c0:c0 + C] = yc
    return dict(ms=torch.from_numpy(ms), y=torch.from_numpy(y), mean_off=mean_off, scale_off=scale_off, c0=c0, C=C)


def pass_reference(inp, parity, dtype):
    """-> (y_hat (B, H, W, C) float32 on the full grid, bits (B, H, W, C) in dtype, 0 off the pass's sites, site mask (H, W))."""
    C, c0 = inp["C"], inp["c0"]
    mu = inp["ms"][..., inp["mean_off"]:inp["mean_off"] + C]
    sigma = inp["ms"][..., inp["scale_off"]:inp["scale_off"] + C]
    y_hat, bits = R.gaussian_bits(inp["y"][..., c0:c0 + C], mu, sigma, dtype)
    site = R.checkerboard(mu.shape[1], mu.shape[2], parity)
    return y_hat, torch.where(site[None, :, :, None], bits, torch.zeros((), dtype=dtype)), site


def run_pass(inp, parity, sel=slice(None)):
    from evc_amd import lib as L
    ms, y = inp["ms"][sel].cuda().contiguous(), inp["y"][sel].cuda().contiguous()
    y_hat = torch.full_like(y, SENTINEL)
    bits = L.elic_rate_pass(ms, inp["mean_off"], inp["scale_off"], inp["C"], y, inp["c0"], parity, y_hat)
    assert bits.dtype == torch.float64
    return y_hat.cpu(), bits.cpu()


def bitwise_equal(a, b):
    """Same float32 bit patterns, any NaN counting as equal to any NaN."""
    a, b = a.contiguous(), b.contiguous()
    nan = torch.isnan(a) & torch.isnan(b)
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | nan).all())


def expected_y_hat(inp, ref_y_hat, site):
    want = torch.full_like(inp["y"], SENTINEL)
    c0, C = inp["c0"], inp["C"]
    want[..., c0:c0 + C] = torch.where(site[None, :, :, None], ref_y_hat, want[..., c0:c0 + C])
    return want


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("C,H,W", [(16, 4, 4), (192, 8, 8), (32, 4, 8)])
def test_rate_pass_against_float64(C, H, W, parity, B):
    inp = pass_inputs(100 + C + H, 3, C, H, W)
    sel = slice(0, B)
    y_hat, bits = run_pass(inp, parity, sel)
    ref_y_hat, b64, site = pass_reference(inp, parity, torch.float64)
    _, b32, _ = pass_reference(inp, parity, torch.float32)
    # quantised values at the pass's sites bitwise those of torch's float32 rint(y - mu) + mu, everything else untouched
    assert bitwise_equal(y_hat, expected_y_hat(inp, ref_y_hat, site)[sel])
    at = torch.where(site)
    assert float(ref_y_hat[0, at[0][0], at[1][0], 0]) == 2.0 + 1.25 and float(ref_y_hat[0, at[0][0], at[1][0], 1]) == 4.0 + 1.25
    assert float(b64[0, at[0][0], at[1][0], 2]) == R.FLOOR_BITS == float(b64[0, at[0][0], at[1][0], 3])       # the outliers hit the floor
    check_totals(f"rate pass C{C} H{H} W{W} parity {parity} B{B}", bits, b64[sel], b32[sel], (1, 2, 3))
    if B == 3:        # sample 0 alone: the same 64-bit pattern as one of three
        _, alone = run_pass(inp, parity, slice(0, 1))
        assert alone.view(torch.int64)[0] == bits.view(torch.int64)[0]


def test_rate_pass_per_symbol():
    """One site per sample (C = 1, H = 1, W = 2, parity 0: the site is w = 0): bits[b] is one symbol's -log2 p, which gives the
    per-symbol distance from float64 the sums hide."""
    from evc_amd import lib as L
    n = 4096
    rng = np.random.default_rng(7)
    mu = (3 * rng.standard_normal(n)).astype(np.float32)
    sigma = np.exp(rng.uniform(np.log(0.02), np.log(64.0), n)).astype(np.float32)
    yv = (mu + np.maximum(sigma, 0.11) * 2.0 * rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    ms = torch.zeros(n, 1, 2, 2)
    ms[:, 0, 0, 0], ms[:, 0, 0, 1] = torch.from_numpy(mu), torch.from_numpy(sigma)
    y = torch.zeros(n, 1, 2, 1)
    y[:, 0, 0, 0] = torch.from_numpy(yv)
    y_hat = torch.full((n, 1, 2, 1), SENTINEL).cuda()
    bits = L.elic_rate_pass(ms.cuda(), 0, 1, 1, y.cuda(), 0, 0, y_hat).cpu()
    want_y, b64 = R.gaussian_bits(y[:, 0, 0, 0], ms[:, 0, 0, 0], ms[:, 0, 0, 1], torch.float64)
    _, b32 = R.gaussian_bits(y[:, 0, 0, 0], ms[:, 0, 0, 0], ms[:, 0, 0, 1], torch.float32)
    assert bitwise_equal(y_hat.cpu()[:, 0, 0, 0], want_y) and bool((y_hat.cpu()[:, 0, 1, 0] == SENTINEL).all())
    e_sym = float((b32.double() - b64).abs().max())
    got = float((bits - b64).abs().max())
    _report("rate pass e_sym", f"{n} symbols", got, e_sym)
    assert got <= 4 * e_sym


# ---- bottleneck kernel ------------------------------------------------------------------------------------------------------------
def bottleneck_inputs(seed, B, C, h, w):
    """Random density parameters with non-zero factors (the tanh terms count), values of a few units plus, in every sample,
    values far in both tails (the sign flip of the sigmoid difference, the floor)."""
    rng = np.random.default_rng(seed)
    F = R.FILTERS
    t = lambda scale, *shape: torch.from_numpy((scale * rng.standard_normal(shape)).astype(np.float32))
    mats = [t(0.5, C, F[i + 1], F[i]) - 1.0 for i in range(5)]          # softplus ~ 0.3: a gain near 1 per layer of three
    bias = [t(0.5, C, F[i + 1], 1) for i in range(5)]
    fact = [t(1.0, C, F[i + 1], 1) for i in range(4)]
    med = t(0.3, C)
    z = t(4.0, B, C, h, w)
    z[:, 0, 0, 0], z[:, 1, 0, 0], z[:, 2, 0, 0], z[:, 3, 0, 0] = 300.0, -300.0, 25.0, -25.0
    return dict(z=z, med=med, raw=(mats, bias, fact), C=C)


def run_bottleneck(inp, sel=slice(None), ld=None):
    from evc_amd import entropy, lib as L
    C = inp["C"]
    z = inp["z"][sel].permute(0, 2, 3, 1).contiguous()                   # NHWC
    if ld is not None:
        wide = torch.full(z.shape[:3] + (ld,), 7.0)
        wide[..., :C] = z
        z = wide
    out = torch.full_like(z, SENTINEL).cuda()
    table = entropy.pack_density(*inp["raw"]).cuda()
    z_hat, bits = L.bottleneck_rate(z.cuda(), C, inp["med"].cuda(), table, out=out)
    assert z_hat is out and bits.dtype == torch.float64
    return z_hat.cpu(), bits.cpu()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C,h,w", [(192, 1, 1), (192, 2, 2), (8, 2, 4)])
def test_bottleneck_rate_against_float64(C, h, w, B):
    inp = bottleneck_inputs(200 + C + h, 3, C, h, w)
    sel = slice(0, B)
    ld = C + 4 if C == 8 else None                                       # one case with a row stride wider than C
    z_hat, bits = run_bottleneck(inp, sel, ld)
    want_z, b64 = R.bottleneck_bits(inp["z"], inp["med"], *inp["raw"], torch.float64)
    _, b32 = R.bottleneck_bits(inp["z"], inp["med"], *inp["raw"], torch.float32)
    assert bitwise_equal(z_hat[..., :C], want_z[sel].permute(0, 2, 3, 1))
    assert bool((z_hat[..., C:] == SENTINEL).all())                      # nothing but the C channels is written
    assert float(b64[:, 0, 0, 0].max()) == R.FLOOR_BITS == float(b64[:, 1, 0, 0].max())      # both far tails hit the floor
    assert bool(torch.isfinite(b64).all())
    check_totals(f"bottleneck C{C} h{h} w{w} B{B}", bits, b64[sel], b32[sel], (1, 2, 3))
    if B == 3:
        _, alone = run_bottleneck(inp, slice(0, 1), ld)
        assert alone.view(torch.int64)[0] == bits.view(torch.int64)[0]


# ---- non-finite values ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where,value", [("y", float("nan")), ("mu", float("nan")), ("sigma", float("nan")), ("y", float("inf"))])
def test_rate_pass_non_finite_follows_torch(where, value):
    C, H, W = 16, 4, 4
    clean = pass_inputs(31, 3, C, H, W)
    _, clean_bits = run_pass(clean, 0)
    bad = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in clean.items()}
    h, w, c = 2, 2, 5                                                    # an anchor site: (h + w) even
    col = {"y": bad["c0"], "mu": bad["mean_off"], "sigma": bad["scale_off"]}[where] + c
    (bad["y"] if where == "y" else bad["ms"])[1, h, w, col] = value
    y_hat, bits = run_pass(bad, 0)
    ref_y_hat, b64, site = pass_reference(bad, 0, torch.float64)
    _, b32, _ = pass_reference(bad, 0, torch.float32)
    assert bitwise_equal(y_hat, expected_y_hat(bad, ref_y_hat, site))    # torch's NaN / inf in y_hat, at that site only
    assert not bool(torch.isfinite(y_hat[1, h, w, bad["c0"] + c])) or where == "sigma"
    if np.isnan(value):
        assert bool(torch.isnan(b64[1, h, w, c])) and bool(torch.isnan(bits[1]))
    else:                                                                # +inf: that symbol costs the floor value
        assert float(b64[1, h, w, c]) == R.FLOOR_BITS
        check_totals("rate pass +inf", bits[1:2], b64[1:2], b32[1:2], (1, 2, 3))
    for b in (0, 2):                                                     # the other samples: the clean run's bit patterns
        assert bits.view(torch.int64)[b] == clean_bits.view(torch.int64)[b]


def test_bottleneck_non_finite_follows_torch():
    inp = bottleneck_inputs(41, 3, 8, 2, 4)
    _, clean_bits = run_bottleneck(inp)
    inp["z"][1, 3, 1, 2] = float("nan")
    z_hat, bits = run_bottleneck(inp)
    want_z, b64 = R.bottleneck_bits(inp["z"], inp["med"], *inp["raw"], torch.float64)
    assert bitwise_equal(z_hat, want_z.permute(0, 2, 3, 1)) and bool(torch.isnan(z_hat[1, 1, 2, 3]))
    assert bool(torch.isnan(b64[1, 3, 1, 2])) and bool(torch.isnan(bits[1]))
    for b in (0, 2):
        assert bits.view(torch.int64)[b] == clean_bits.view(torch.int64)[b]


def test_argument_checks():
    from evc_amd import lib as L
    inp = pass_inputs(1, 1, 16, 4, 4)
    ms, y = inp["ms"].cuda(), inp["y"].cuda()
    y_hat = torch.zeros_like(y)
    with pytest.raises(L.EvcKernelError):                                # odd W
        L.elic_rate_pass(ms[:, :, :3].contiguous(), 3, 21, 16, y[:, :, :3].contiguous(), 2, 0, y_hat[:, :, :3].contiguous())
    with pytest.raises(L.EvcKernelError):                                # C <= 0
        L.elic_rate_pass(ms, 3, 21, 0, y, 2, 0, y_hat)
    with pytest.raises(L.EvcKernelError):                                # the slice would leave y's row
        L.elic_rate_pass(ms, 3, 21, 16, y, 8, 0, y_hat)
    lib = L.hip_lib()
    assert lib.evc_elic_rate_pass_f32(None, 41, 3, 21, 16, L.fptr(y), 23, 2, 1, 4, 4, 0, L.fptr(y_hat), None, None) == -1
    assert lib.evc_bottleneck_rate_f32(None, 8, 8, 1, 2, 4, None, None, None, None, None) == -1


# ---- model level ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    import evc_amd  # noqa: F401
    from evc_amd import synthetic
    from evc_amd.elic import ElicModel
    sd = synthetic.elic_state_dict_with_density(3)
    return sd, ElicModel(sd)


def model_reference(sd, est, dtype):
    """Per-frame (bits_y, bits_z) of the restatement fed the GPU's own y, per-pass means / scales and z."""
    from evc_amd import entropy
    y = est["y"].cpu()
    B = y.shape[0]
    by = torch.zeros(B, dtype=torch.float64)
    for p in est["passes"]:
        mu, sigma = p["means"].cpu(), p["scales"].cpu()
        g = mu.shape[1]
        _, bits = R.gaussian_bits(y[:, p["c0"]:p["c0"] + g], mu, sigma, dtype)
        site = R.checkerboard(y.shape[2], y.shape[3], p["parity"])
        by += torch.where(site[None, None], bits.double(), torch.zeros((), dtype=torch.float64)).sum((1, 2, 3))
    raw, missing = entropy.density_from_state_dict(sd)
    assert not missing
    med = sd["entropy_bottleneck.quantiles"][:, 0, 1]
    _, bz = R.bottleneck_bits(est["z"].cpu(), med, *raw, dtype)
    return by, bz.double().sum((1, 2, 3))


@pytest.mark.parametrize("size", [64, 128])
def test_estimate_decodes_what_the_coded_path_decodes(model, size):
    from evc_amd import synthetic
    sd, m = model
    x = torch.from_numpy(synthetic.make_clips(1, seed=3, frames=3, size=size)[0].astype(np.float32) / 255)
    enc = m.compress(x, return_latents=True)
    dec = m.decompress(enc["strings"], enc["shape"], return_latents=True)
    est = m.estimate(x, return_latents=True)
    assert est["shape"] == enc["shape"] == (size // 64, size // 64)
    assert torch.equal(est["x_hat"], dec["x_hat"])
    assert torch.equal(est["y_hat"], dec["y_hat"]) and torch.equal(est["z_hat"], dec["z_hat"])
    assert torch.equal(est["y"], enc["y"]) and len(est["passes"]) == 10
    assert est["bits_y"].dtype == est["bits_z"].dtype == torch.float64 and est["bits_y"].shape == (3,)
    y64, z64 = model_reference(sd, est, torch.float64)
    y32, z32 = model_reference(sd, est, torch.float32)
    # y and z apart, then the total.  On THIS checkpoint the float32 yardstick of z is large: its density is an exactly
    # symmetric logistic, so at the symbol 0 float32 arithmetic often gives lower + upper == 0, sign 0 and the floor for a
    # likelihood that is really ~0.2 (tests/test_elic_rate_host.py shows the same at float64 where it is exact); the kernel
    # evaluates the density in double and stays with float64.  The y part is the one this yardstick bites on.
    for what, got, w64, w32 in (("y", est["bits_y"], y64, y32), ("z", est["bits_z"], z64, z32),
                                ("y + z", est["bits_y"] + est["bits_z"], y64 + z64, y32 + z32)):
        e_sum = float(((w32 - w64).abs() / w64).max())
        rel = float(((got - w64).abs() / w64).max())
        _report(f"model {size}x{size} {what} e_sum", f"bits {got.tolist()}", rel, e_sum)
        assert rel <= 4 * e_sum, (what, rel, e_sum)
    one = m.estimate(x[:1])                                              # frame 0 alone: the same bits, to the last one
    assert one["bits_y"].view(torch.int64)[0] == est["bits_y"].view(torch.int64)[0]
    assert one["bits_z"].view(torch.int64)[0] == est["bits_z"].view(torch.int64)[0]
    assert torch.equal(one["x_hat"][0], est["x_hat"][0])


def test_estimate_names_the_missing_density():
    from evc_amd import entropy, synthetic
    from evc_amd.elic import ElicModel, inference_estimate
    m = ElicModel(synthetic.elic_state_dict(3))                          # loads and codes as ever
    with pytest.raises(entropy.DensityParametersMissing, match="entropy_bottleneck._matrix0"):
        inference_estimate(m, torch.zeros(3, 64, 64))


def test_inference_estimate_and_estimated_batch(model):
    from evc_amd import policy as P, synthetic
    from evc_amd.elic import inference, inference_estimate
    sd, m = model
    x = torch.from_numpy(synthetic.make_clips(1, seed=3, frames=2, size=128)[0].astype(np.float32) / 255)
    img = x[0][:, :100, :120]
    x_hat, bits = inference_estimate(m, img, patch=64)
    coded_hat, coded_bits = inference(m, img, patch=64)
    assert isinstance(bits, float) and torch.equal(x_hat, coded_hat.to(x_hat.device)) and bits != coded_bits
    xh, b, strings, shape = P.estimated_batch(m, x.cuda(), 64)
    xc, bc, _, shape_c = P.coded_batch(m, x.cuda(), 64)
    assert strings is None and tuple(shape) == tuple(shape_c) and torch.equal(xh, xc)
    assert all(isinstance(v, float) for v in b) and len(b) == 2 and b != [float(v) for v in bc]


# ---- CLI -----------------------------------------------------------------------------------------------------------------------
def test_cli_entropy_estimation(tmp_path, monkeypatch):
    """--entropy-estimation: the same saved frames as without it, the rate from the estimate."""
    import evc_amd  # noqa: F401
    from evc_amd import cli, synthetic
    from evc_amd.elic import ElicModel
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.chdir(tmp_path)
    base = ["--config", os.path.join(repo, "configs", "mine.yml"), "--synthetic", "--exp", str(tmp_path / "exp"),
            "--data_npy", "missing.npy", "--start_idx", "0", "--end_idx", "0", "--subsample", "2", "--q", "3",
            "--config_mod", "model.ngf=32 model.n_head_channels=32"]
    cli.main(base + ["--output_path", str(tmp_path / "coded")])
    cli.main(base + ["--output_path", str(tmp_path / "est"), "--entropy-estimation"])
    name = "city_output_npy_idx0_q3_thr0.00.npy"
    a, b = np.load(tmp_path / "coded" / "output_0" / name), np.load(tmp_path / "est" / "output_0" / name)
    assert a.shape == (2 * 128, 30 * 128, 3) and np.array_equal(a, b)
    bpp_coded, bpp_est = np.load(tmp_path / "coded" / "output_0" / "bpp_0.npy"), np.load(tmp_path / "est" / "output_0" / "bpp_0.npy")
    assert bpp_coded.shape == bpp_est.shape == (1,)
    m = ElicModel(synthetic.elic_state_dict_with_density(3))
    clip = torch.from_numpy(synthetic.make_clips(1, seed=1234)[0][:2].astype(np.float32) / 255.0)       # --seed's default
    bits = []
    for f in (0, 1):                                                     # the sender estimates frame 0 and frame 1 of the batch apart
        est = m.estimate(clip[f:f + 1])
        bits.append((est["bits_y"] + est["bits_z"]).tolist()[0])
    assert bpp_est[0] == sum(bits) / 128 / 128 / 30
    print(f"[elic-rate] cli bpp: estimated {bpp_est[0]:.6f} coded {bpp_coded[0]:.6f}")
    assert bpp_est[0] != bpp_coded[0]


def test_cli_entropy_estimation_in_the_policy_sweep(tmp_path, monkeypatch):
    """The sweep's key frames (``key_cache``) take the estimation path too: a threshold nothing passes key-codes all 30 frames,
    and the job's bpp is the sum of the 30 estimates -- whatever batches the sweep estimated them in."""
    import evc_amd  # noqa: F401
    from evc_amd import cli, synthetic
    from evc_amd.elic import ElicModel
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.chdir(tmp_path)
    cli.main(["--config", os.path.join(repo, "configs", "mine.yml"), "--synthetic", "--exp", str(tmp_path / "exp"),
              "--data_npy", "missing.npy", "--output_path", str(tmp_path / "out"), "--start_idx", "0", "--end_idx", "0",
              "--subsample", "2", "--q", "3", "--config_mod", "model.ngf=32 model.n_head_channels=32",
              "--policy", "psnr", "--thresholds", "200", "--bpp-limit", "1e9", "--entropy-estimation"])
    bpp = np.load(tmp_path / "out" / "output_0" / "bpp_0.npy")
    m = ElicModel(synthetic.elic_state_dict_with_density(3))
    clip = torch.from_numpy(synthetic.make_clips(1, seed=1234)[0].astype(np.float32) / 255.0)
    est = m.estimate(clip)
    bits = (est["bits_y"] + est["bits_z"]).tolist()
    assert bpp.shape == (1,) and bpp[0] == sum(bits) / 128 / 128 / 30
    saved = np.load(tmp_path / "out" / "output_0" / "city_output_npy_idx0_q3_thr200.00.npy")[128:]      # the decoded row of frames
    want = est["x_hat"].cpu().numpy().transpose(0, 2, 3, 1)
    assert np.array_equal(saved, np.concatenate(list(want), axis=1))
