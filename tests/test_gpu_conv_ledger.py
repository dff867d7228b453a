"""GPU parity of every plan class of the convolution (tests/conv_ledger.py): one test per entry of ``CASES``.  Each entry is run
on the kernel instance the ledger states for it -- the name ``lib.CONV_PROFILE`` records must be that one -- and compared with
``F.conv2d`` in float64 on the device, applied to the float64 on-load transform of the same inputs.

Bars are those of the existing test of the same family (tests/test_gpu_ops.py), relative to max |ref|:
    3e-6  conv_wide_kernel and every launch with a fused 1x1 operand   (test_conv_wide_kernel_..., test_conv3x3_with_fused_1x1_operand)
    5e-6  long K, >= 1536 * 9 products per output                       (test_conv_bf16x6_is_not_less_accurate_than_f32_mfma)
    2e-6  raw operands scaled by an element bound                       (test_conv_f16x3_on_raw_input_with_moment_bound)
and for every other class the rule of test_conv_bf16x6_is_not_less_accurate_than_f32_mfma: the same case under EVC_ARITH_F32
(exact products, fp32 accumulation) against the same reference, and at most twice its max error.  Measured errors per class:
profiles/NOTES.md."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ledger as ledger
from conftest import rnd

pytestmark = pytest.mark.gpu

SCALE = 0.70710678
SAMPLE_SCALES = (1.0, 8.0, 0.125)      # invariant mode, raw operands: one bound word per sample, so one magnitude per sample


@pytest.fixture(scope="module")
def L():
    import evc_amd  # noqa: F401
    from evc_amd import lib
    lib.hip_lib()   # raises if libevc_hip.so is missing or the device is not gfx950: no silent fallback
    return lib


def fixed_bar(c):
    """The bar of the case's family, None where the family has no precedent (then: twice the error of EVC_ARITH_F32)."""
    if c.cls[0].startswith("conv_wide_kernel") or c.x2:
        return 3e-6
    if c.K * c.K * (c.C0 + c.C1) >= 1536 * 9:
        return 5e-6
    if c.bound:
        return 2e-6
    return None


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def per_sample(t, scales):
    return t * torch.tensor([scales[b % len(scales)] for b in range(t.shape[0])], dtype=t.dtype).view(-1, 1, 1, 1)


def bound_of(L, parts, HW, B, invariant):
    """The element bound word(s) of a raw operand (a virtual concat of ``parts``), as the network makes them: by the
    coefficient kernel, from the operand's moments; one word per sample in invariant mode."""
    word = torch.zeros(B if invariant else 1, dtype=torch.int32, device="cuda")
    C = sum(p.shape[-1] for p in parts)
    L.gn_coeffs([L.chan_stats(p, invariant=invariant) for p in parts], HW, C // 16, 1e-5, bound=word, invariant=invariant)
    return word


def rel_err(out, ref, by_sample):
    """max |out - ref| / max |ref|; per sample (and the worst of them) where every sample has its own scale."""
    e = (out.double() - ref).abs()
    if by_sample:
        return float((e.amax(dim=(1, 2, 3)) / ref.abs().amax(dim=(1, 2, 3))).max())
    return float(e.max() / ref.abs().max())


@pytest.mark.parametrize("c", ledger.CASES, ids=[ledger.case_id(c) for c in ledger.CASES])
def test_conv_plan_class_against_fp64(L, c):
    B, H, W, C0, C1, Co, K = c.B, c.H, c.W, c.C0, c.C1, c.Co, c.K
    C = C0 + C1
    kernel, kind = c.cls[0], c.cls[1]
    raw_scales = SAMPLE_SCALES if c.invariant and (c.bound or c.x2) else (1.0,)
    x = rnd(900, B, C, H, W)
    if c.bound:
        x = per_sample(x, raw_scales)
    x = nhwc(x).cuda()
    x0, x1 = x[..., :C0].contiguous(), (x[..., C0:].contiguous() if C1 else None)
    w = (rnd(901, Co, C, K, K) / np.sqrt(K * K * C)).cuda()
    bias, res = rnd(902, Co).cuda(), nhwc(rnd(903, B, Co, H, W)).cuda()
    kw = dict(bias=bias, src1=x1, res=res, out_scale=SCALE, splits=c.splits)
    pre = nchw(x).double()
    if c.coef:
        a, s = (1 + 0.2 * rnd(904, B, C)).cuda(), (0.3 * rnd(905, B, C)).cuda()
        kw.update(coef=(a, s))
        pre = pre * a.double()[:, :, None, None] + s.double()[:, :, None, None]
    if c.act:
        assert c.act == L.ACT_SILU
        kw.update(act_in=L.ACT_SILU)
        pre = F.silu(pre)
    ref = F.conv2d(pre, w.double(), bias.double(), padding=K // 2)
    f32_kw = dict(kw)                                   # the exact-product run takes neither a bound nor the invariant plan
    if c.bound:
        kw.update(in_bound=bound_of(L, [x0] + ([x1] if C1 else []), H * W, B, c.invariant))
    if c.x2:
        x2 = nhwc(per_sample(rnd(906, B, c.x2, H, W), raw_scales)).cuda()
        xa, xb = (x2[..., :c.x2 - 16].contiguous(), x2[..., c.x2 - 16:].contiguous()) if c.x2 >= 32 else (x2, None)
        w2 = (rnd(907, Co, c.x2, 1, 1) / np.sqrt(c.x2)).cuda()
        kw.update(x2=(xa, xb, L.conv_pack_weights(w2, L.ARITH_F16X3),
                      bound_of(L, [xa] + ([xb] if xb is not None else []), H * W, B, c.invariant)))
        ref = ref + F.conv2d(nchw(x2).double(), w2.double())
    ref = (ref + nchw(res).double()) * SCALE
    assert L.range_events(reset=True) == 0
    plan = L.conv_plan(B, H, W, C0, C1, Co, K, c.arith, coef=bool(c.coef), act_in=c.act, x2_ci=c.x2, invariant=c.invariant,
                       splits=c.splits)
    stats = plan["stats_runs"] > 0
    wp = L.conv_pack_weights(w, c.arith)

    def run():
        prof = []
        L.CONV_PROFILE = prof
        try:
            r = L.conv2d_nhwc(x0, wp, Co, K, K, want_stats=stats, invariant=c.invariant, **kw)
        finally:
            L.CONV_PROFILE = None
        return (r if stats else (r, None)), prof[0]

    (out, st), prof = run()
    assert prof["kernel"] == kernel, (prof["kernel"], kernel)
    assert prof["split"] == (kind != "none"), (prof["split"], kind)        # split-K slabs exactly for z-split, tail and cut
    err = rel_err(nchw(out), ref, len(raw_scales) > 1)
    bar = fixed_bar(c)
    e32 = None
    if bar is None:
        o32 = L.conv2d_nhwc(x0, L.conv_pack_weights(w, L.ARITH_F32), Co, K, K, **f32_kw)
        e32 = rel_err(nchw(o32), ref, False)
        bar = 2.0 * e32
    print(f"LEDGER {ledger.case_id(c)} | {kernel} | err {err:.3e} | bar {bar:.3e} | f32 {'-' if e32 is None else format(e32, '.3e')}")
    assert err <= bar, (err, bar, e32)
    if stats:
        o = out.double().reshape(B, H * W, Co)
        want = torch.stack([o.sum(1), (o * o).sum(1)], -1)
        got = st.double().sum(1)
        assert float((got - want).abs().max() / want.abs().max()) < 1e-5
    (again, st2), _ = run()
    assert torch.equal(again, out) and (not stats or torch.equal(st2, st))
