"""Restatement, in torch, of the two likelihood formulas of the ELIC rate estimate (csrc/rate.hip), written from their
definition (compressai 1.1.5 ``GaussianConditional.forward`` / ``EntropyBottleneck.forward`` in eval mode):

Gaussian-conditional pass, per site:
    sym = rint(y - mu);  y_hat = sym + mu;  v = |sym|;  s = max(sigma, 0.11)
    p = 1/2 erfc(-(0.5 - v) / (s sqrt 2)) - 1/2 erfc(-(-0.5 - v) / (s sqrt 2));  p = max(p, 1e-9);  bits = -log2 p
factorised density, per element of channel c:
    zq = rint(z - med_c) + med_c;  lower = L_c(zq - 0.5), upper = L_c(zq + 0.5);  sgn = -sign(lower + upper)
    p = |sigmoid(sgn upper) - sigmoid(sgn lower)|;  p = max(p, 1e-9)
    L_c: logits = x; for layer i in 0..4: logits = softplus(M_i) logits + b_i; if i < 4: logits += tanh(f_i) tanh(logits)

Quantisation (rint, the sums y_hat / zq) is always float32, as in the model.  Everything after it is evaluated in ``dtype``:
float64 is the reference the kernels are compared with; float32 -- the same formulas as torch evaluates them on the CPU --
is the yardstick of the tolerance (how far plain fp32 arithmetic is from float64 on the same inputs).  The bounds are
``torch.max(x, bound)``, which keeps a NaN; 0.11 and 1e-9 are the float32 values compressai holds them as."""
import numpy as np
import torch

SCALE_BOUND = float(np.float32(0.11))
LIKELIHOOD_BOUND = float(np.float32(1e-9))
FLOOR_BITS = -float(torch.log2(torch.tensor(LIKELIHOOD_BOUND, dtype=torch.float64)))      # what a floored symbol costs
FILTERS = (1, 3, 3, 3, 3, 1)


def _bound(x, b):
    return torch.max(x, torch.tensor(b, dtype=x.dtype))


def gaussian_bits(y, mu, sigma, dtype=torch.float64):
    """y, mu, sigma: float32 tensors of one shape -> (y_hat float32, bits per element in ``dtype``)."""
    y, mu, sigma = y.float(), mu.float(), sigma.float()
    sym = torch.round(y - mu)
    y_hat = sym + mu
    v = sym.abs().to(dtype)
    s = _bound(sigma.to(dtype), SCALE_BOUND)
    const = -(2 ** -0.5)
    upper = 0.5 * torch.erfc(const * ((0.5 - v) / s))
    lower = 0.5 * torch.erfc(const * ((-0.5 - v) / s))
    p = _bound(upper - lower, LIKELIHOOD_BOUND)
    return y_hat, -torch.log2(p)


def logits_cumulative(x, matrices, biases, factors, dtype):
    """x: (C, n) in ``dtype``; raw parameters matrices[i] (C, out, in), biases[i] (C, out, 1), factors[i] (C, out, 1)."""
    logits = x[:, None, :]
    for i in range(len(FILTERS) - 1):
        m = torch.nn.functional.softplus(matrices[i].to(dtype))
        logits = (m[:, :, :, None] * logits[:, None, :, :]).sum(2) + biases[i].to(dtype)
        if i < len(FILTERS) - 2:
            logits = logits + torch.tanh(factors[i].to(dtype)) * torch.tanh(logits)
    return logits[:, 0, :]


def density(zq, matrices, biases, factors, dtype=torch.float64):
    """Unbounded likelihood of the quantised values zq (C, n): |sigmoid(sgn upper) - sigmoid(sgn lower)|."""
    zq = zq.to(dtype)
    lower = logits_cumulative(zq - 0.5, matrices, biases, factors, dtype)
    upper = logits_cumulative(zq + 0.5, matrices, biases, factors, dtype)
    sgn = -torch.sign(lower + upper)
    return (torch.sigmoid(sgn * upper) - torch.sigmoid(sgn * lower)).abs()


def bottleneck_bits(z, medians, matrices, biases, factors, dtype=torch.float64):
    """z: (B, C, h, w) float32, medians (C,) -> (z_hat float32 (B, C, h, w), bits per element in ``dtype``)."""
    z = z.float()
    med = medians.float()[None, :, None, None]
    zq = torch.round(z - med) + med
    B, C = z.shape[:2]
    p = density(zq.permute(1, 0, 2, 3).reshape(C, -1), matrices, biases, factors, dtype)
    p = _bound(p, LIKELIHOOD_BOUND).reshape(C, B, *z.shape[2:]).permute(1, 0, 2, 3)
    return zq, -torch.log2(p)


def checkerboard(H, W, parity):
    """Boolean (H, W): the sites of a pass -- anchors (parity 0) where (h + w) is even, non-anchors where it is odd."""
    h = torch.arange(H)[:, None]
    w = torch.arange(W)[None, :]
    return ((h + w) % 2) == parity


def yardstick(bits64, bits32, dims):
    """(e_sym, e_sum) of a batch: the largest per-symbol difference of the fp32 evaluation from the fp64 one, and the largest
    relative difference of a sample's total (per-symbol values added in float64 on both sides; ``dims``: the axes of a sample)."""
    b32 = bits32.double()
    e_sym = float((b32 - bits64).abs().max())
    t64, t32 = bits64.sum(dims), b32.sum(dims)
    return e_sym, float(((t32 - t64).abs() / t64.abs()).max())
