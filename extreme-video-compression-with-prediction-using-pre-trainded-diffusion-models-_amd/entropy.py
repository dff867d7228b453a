"""Host-side entropy-model logic for the ELIC codec, on top of the native range-ANS coder (libevc_rans.so).

Mirrors what the reference reaches through compressai 1.1.5 (Appendix B of SURVEY.md):
``EntropyBottleneck.{compress,decompress}`` for the hyper-latent z and the table builder
``GaussianConditional.update`` (+ C++ ``pmf_to_quantized_cdf``) used when a checkpoint has to be synthesised.
The per-symbol CDF index of the Gaussian-conditional slices is computed on the GPU
(evc_elic_gather_params_f32); only int32 indexes / symbols cross the PCIe link.
"""
import math

import numpy as np
import torch

from . import lib as L

SCALES_MIN, SCALES_MAX, SCALES_LEVELS = 0.11, 256, 64


def get_scale_table(lo=SCALES_MIN, hi=SCALES_MAX, levels=SCALES_LEVELS):
    """reference Network.py:23-27."""
    return torch.exp(torch.linspace(math.log(lo), math.log(hi), levels))


class Tables:
    """Quantised CDF table set of one entropy model: cdf (n, ld) int32, length (n,), offset (n,)."""

    def __init__(self, cdf, length, offset):
        self.cdf = np.ascontiguousarray(np.asarray(cdf, dtype=np.int32))
        self.length = np.ascontiguousarray(np.asarray(length, dtype=np.int32).reshape(-1))
        self.offset = np.ascontiguousarray(np.asarray(offset, dtype=np.int32).reshape(-1))

    @classmethod
    def from_state_dict(cls, sd, prefix):
        return cls(sd[prefix + "._quantized_cdf"].cpu().numpy(), sd[prefix + "._cdf_length"].cpu().numpy(),
                   sd[prefix + "._offset"].cpu().numpy())

    def encode(self, symbols, indexes):
        return L.rans_encode(symbols, indexes, self.cdf, self.length, self.offset)

    def decode(self, data, indexes):
        return L.rans_decode(data, indexes, self.cdf, self.length, self.offset)


def gaussian_conditional_tables(scale_table, tail_mass=1e-9, precision=16):
    """``GaussianConditional.update()``: per scale a discretised zero-mean Gaussian + tail-mass symbol."""
    scale_table = torch.as_tensor(scale_table, dtype=torch.float32)
    # _standardized_quantile(tail_mass / 2) = scipy.stats.norm.ppf
    multiplier = -float(torch.distributions.Normal(0.0, 1.0).icdf(torch.tensor(tail_mass / 2, dtype=torch.float64)))
    pmf_center = torch.ceil(scale_table * multiplier).int()
    pmf_length = 2 * pmf_center + 1
    max_length = int(pmf_length.max())
    samples = torch.abs(torch.arange(max_length).int() - pmf_center[:, None]).float()
    s = scale_table.unsqueeze(1)
    std_cum = lambda v: 0.5 * torch.erfc(-(2 ** -0.5) * v)
    upper = std_cum((0.5 - samples) / s)
    lower = std_cum((-0.5 - samples) / s)
    pmf = upper - lower
    tail = 2 * lower[:, :1]
    cdf = np.zeros((len(pmf_length), max_length + 2), dtype=np.int32)
    for i in range(len(pmf_length)):
        prob = torch.cat((pmf[i, :pmf_length[i]], tail[i]), dim=0).numpy()
        c = L.pmf_to_quantized_cdf(prob, precision)
        cdf[i, :len(c)] = c
    return Tables(cdf, (pmf_length + 2).numpy(), (-pmf_center).numpy())


def logistic_bottleneck_tables(scales, tail_mass=1e-9, precision=16):
    """Synthetic stand-in for ``EntropyBottleneck.update()`` (its learned density is not needed to decode:
    the decoder only reads tables + medians, which real checkpoints ship)."""
    scales = np.asarray(scales, dtype=np.float64)
    half_w = np.ceil(scales * math.log(2 / tail_mass - 1)).astype(np.int32) + 1
    pmf_length = 2 * half_w + 1
    cdf = np.zeros((len(scales), int(pmf_length.max()) + 2), dtype=np.int32)
    sig = lambda v: 1 / (1 + np.exp(-v))
    for i, (s, hw) in enumerate(zip(scales, half_w)):
        k = np.arange(-hw, hw + 1, dtype=np.float64)
        pmf = sig((k + 0.5) / s) - sig((k - 0.5) / s)
        tail = max(1 - pmf.sum(), 1e-12)
        c = L.pmf_to_quantized_cdf(np.concatenate([pmf, [tail]]).astype(np.float32), precision)
        cdf[i, :len(c)] = c
    return Tables(cdf, pmf_length + 2, -half_w)


class EntropyBottleneckCodec:
    """z path: index = channel id, symbol = round(z - median) (compressai EntropyBottleneck)."""

    def __init__(self, tables, medians):
        self.tables = tables
        self.medians = np.asarray(medians, dtype=np.float32).reshape(-1)
        self.channels = self.tables.cdf.shape[0]

    def _indexes(self, size):
        return np.broadcast_to(np.arange(self.channels, dtype=np.int32)[:, None, None],
                               (self.channels, size[0], size[1])).reshape(-1)

    def compress(self, z):
        """z: (B, C, h, w) float32 host array -> list of B byte strings."""
        z = np.asarray(z, dtype=np.float32)
        idx = self._indexes(z.shape[-2:])
        out = []
        for b in range(z.shape[0]):
            sym = np.rint(z[b] - self.medians[:, None, None]).astype(np.int32)   # round half to even
            out.append(self.tables.encode(sym.reshape(-1), idx))
        return out

    def decompress(self, strings, size):
        """-> z_hat (B, C, h, w) float32 host array."""
        idx = self._indexes(size)
        out = np.empty((len(strings), self.channels, size[0], size[1]), dtype=np.float32)
        for b, s in enumerate(strings):
            sym = self.tables.decode(s, idx).reshape(self.channels, size[0], size[1])
            out[b] = sym.astype(np.float32) + self.medians[:, None, None]
        return out


# ---- the factorised density of the hyper-latent (rate estimation: ElicModel.estimate) ----------------------------------------
EB_FILTERS = (1, 3, 3, 3, 3, 1)         # EntropyBottleneck(filters=(3, 3, 3, 3)): widths of the logits-cumulative chain
DENSITY_FLOATS = 58                     # per channel: 3+3+3, 3 x (9+3+3), 3+1
# compressai 1.1.5 (the reference's pin) registers _matrix{i} / _bias{i} / _factor{i}; later releases matrices.{i} / biases.{i} /
# factors.{i} (ParameterLists).  Neither spelling could be checked against the package: both are accepted.
_DENSITY_NAMES = (("_matrix{i}", "matrices.{i}"), ("_bias{i}", "biases.{i}"), ("_factor{i}", "factors.{i}"))


class DensityParametersMissing(RuntimeError):
    """The checkpoint holds quantised CDF tables but not the density they were built from: it codes, it cannot estimate."""


def density_from_state_dict(sd, prefix="entropy_bottleneck"):
    """-> ((matrices[5], biases[5], factors[4]) as float64 tensors, []) or (None, [missing keys, first spelling])."""
    n = len(EB_FILTERS) - 1
    groups, missing = [], []
    for (old, new), count in zip(_DENSITY_NAMES, (n, n, n - 1)):
        got = []
        for i in range(count):
            keys = [f"{prefix}.{old.format(i=i)}", f"{prefix}.{new.format(i=i)}"]
            k = next((k for k in keys if k in sd), None)
            if k is None:
                missing.append(keys[0])
            else:
                got.append(sd[k].detach().to("cpu", torch.float64))
        groups.append(got)
    return (None, missing) if missing else (tuple(groups), [])


def pack_density(matrices, biases, factors):
    """Raw parameters (matrices[i]: (C, out_i, in_i), biases[i]: (C, out_i, 1), factors[i]: (C, out_i, 1)) -> float32 (C, 58):
    softplus(matrix) / bias / tanh(factor) per layer, taken once in float64 and rounded to fp32 (evc_bottleneck_rate_f32)."""
    C = matrices[0].shape[0]
    cols = []
    for i in range(len(EB_FILTERS) - 1):
        fo, fi = EB_FILTERS[i + 1], EB_FILTERS[i]
        assert tuple(matrices[i].shape) == (C, fo, fi) and tuple(biases[i].shape) == (C, fo, 1), (i, matrices[i].shape)
        cols.append(torch.nn.functional.softplus(matrices[i].double()).reshape(C, fo * fi))
        cols.append(biases[i].double().reshape(C, fo))
        if i < len(EB_FILTERS) - 2:
            assert tuple(factors[i].shape) == (C, fo, 1), (i, factors[i].shape)
            cols.append(torch.tanh(factors[i].double()).reshape(C, fo))
    table = torch.cat(cols, 1).float().contiguous()
    assert table.shape == (C, DENSITY_FLOATS)
    return table


def unpack_density(table):
    """Inverse of the layout of ``pack_density``: -> (softplus(matrices)[5], biases[5], tanh(factors)[4]), shaped as the raw ones."""
    C = table.shape[0]
    mats, bias, fact, o = [], [], [], 0
    for i in range(len(EB_FILTERS) - 1):
        fo, fi = EB_FILTERS[i + 1], EB_FILTERS[i]
        mats.append(table[:, o:o + fo * fi].reshape(C, fo, fi)); o += fo * fi
        bias.append(table[:, o:o + fo].reshape(C, fo, 1)); o += fo
        if i < len(EB_FILTERS) - 2:
            fact.append(table[:, o:o + fo].reshape(C, fo, 1)); o += fo
    assert o == DENSITY_FLOATS == table.shape[1]
    return mats, bias, fact


def logistic_density_params(scales, medians, dtype=torch.float32):
    """Raw density parameters for which the factorised density is the logistic ``logistic_bottleneck_tables`` discretises:
    factors 0 (no tanh term), every matrix entry softplus^-1(a / fan_in) with a = s ** -0.2, so each layer multiplies its
    (equal) inputs by a and the chain by 1 / s; biases 0 but the last, -median / s: logits(x) = (x - median) / s."""
    s = torch.as_tensor(np.asarray(scales), dtype=torch.float64)
    med = torch.as_tensor(np.asarray(medians), dtype=torch.float64)
    C = s.numel()
    a = s ** -0.2
    mats, bias, fact = [], [], []
    for i in range(len(EB_FILTERS) - 1):
        fo, fi = EB_FILTERS[i + 1], EB_FILTERS[i]
        raw = torch.log(torch.expm1(a / fi))                         # softplus(raw) = a / fi
        mats.append(raw.reshape(C, 1, 1).expand(C, fo, fi).contiguous().to(dtype))
        b = torch.zeros(C, fo, 1, dtype=torch.float64)
        if i == len(EB_FILTERS) - 2:
            b[:, 0, 0] = -med / s
        bias.append(b.to(dtype))
        if i < len(EB_FILTERS) - 2:
            fact.append(torch.zeros(C, fo, 1, dtype=dtype))
    return mats, bias, fact
