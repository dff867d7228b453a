"""GPU parity of every plan class of the attention (tests/attention_ledger.py): one test per entry of ``CASES``.  Each entry is
run on the kernel instance the ledger states for it -- the plan ``lib.ATTN_PROFILE`` records must be that one -- and compared
with float64 softmax attention on the device.

Inputs: k grows along the keys by linspace(0.3, 4.0, N), so the score maximum moves from tile to tile and key parts have very
different maxima; v = rnd + 1.5, a non-zero mean, so that a wrong softmax denominator (a padded key counted, a part's l dropped
in the merge) shows at full size in the output.  Bound words come from chan_stats + moments_bound, as the network makes them.
Invariant cases on the fp16 split give every sample its own magnitude m in (1, 8, 0.125), hence its own bound words: q * m,
k / m, v * m.  The scores are then those of m = 1 -- at q * m and k * m they would be m^2 times as large, 64 times at m = 8, and
an fp32 rounding of a score near 250 is already 1.5e-5 of a softmax weight: no fp32 kernel could meet the bar below, and the
figure would say nothing about the kernel -- while the three words of a sample differ from those of its neighbours in all of q,
k and v.  Errors are taken per sample there, relative to the sample's own max |ref|.

Bar: max |out - ref| / max |ref| <= 2e-5, the bar of these kernels against float64 in tests/test_gpu_attention_short.py and
tests/test_gpu_ops.py.  The same error of a float32 torch restatement on the same inputs is printed next to it (``LEDGER``
lines; the table is in profiles/NOTES.md).  Key-split classes also agree with the single-pass evc_attention_f32 within 2e-6
(test_attention_key_split_matches_single_pass)."""
import ctypes

import pytest
import torch

import attention_ledger as ledger
from conftest import rnd

pytestmark = pytest.mark.gpu

BAR, SPLIT_BAR = 2e-5, 2e-6
PAD = 8                                   # columns of ``out`` behind the heads * D the kernel owns
TAIL = 4096                               # bytes of workspace behind what the plan asks for
CANARY = 0x7FC0BEEF                       # a NaN: a partial result or a tile image read before it was written poisons the output
SAMPLE_SCALES = (1.0, 8.0, 0.125)         # invariant mode, fp16 split: one triple of bound words per sample
SCORE_BYTES = 256 << 20                   # float64 scores of one reference chunk


@pytest.fixture(scope="module")
def L():
    import evc_amd  # noqa: F401
    from evc_amd import lib
    lib.hip_lib()   # raises if libevc_hip.so is missing or the device is not gfx950: no silent fallback
    return lib


def make_qkv(c):
    B, N, C = c.B, c.N, c.heads * c.D
    q = rnd(910, B, N, C)
    k = rnd(911, B, N, C) * torch.linspace(0.3, 4.0, N)[None, :, None]
    v = rnd(912, B, N, C) + 1.5
    if c.invariant and c.f16:
        m = torch.tensor([SAMPLE_SCALES[b % 3] for b in range(B)]).view(B, 1, 1)
        q, k, v = q * m, k / m, v * m
    return torch.cat([q, k, v], 2).cuda()


def softmax_attention(qkv, heads, dtype):
    """softmax(q k^T / sqrt(D)) v of a (B, N, 3C) q | k | v tensor in ``dtype`` on the device, a few samples at a time."""
    B, N, C3 = qkv.shape
    C = C3 // 3
    D = C // heads
    out = torch.empty(B, N, C, dtype=dtype, device=qkv.device)
    step = max(1, SCORE_BYTES // (heads * N * N * 8))
    for b in range(0, B, step):
        q, k, v = [t.reshape(-1, N, heads, D).permute(0, 2, 1, 3) for t in qkv[b:b + step].to(dtype).split(C, dim=2)]
        w = torch.softmax(torch.einsum("bhqd,bhkd->bhqk", q, k) * (D ** -0.5), dim=-1)
        out[b:b + step] = torch.einsum("bhqk,bhkd->bhqd", w, v).permute(0, 2, 1, 3).reshape(-1, N, C)
    return out


def rel_err(out, ref, by_sample):
    e = (out.double() - ref.double()).abs()
    if by_sample:
        return float((e.amax(dim=(1, 2)) / ref.double().abs().amax(dim=(1, 2))).max())
    return float(e.max() / ref.double().abs().max())


def bounds_of(L, qkv, C, invariant):
    B, N, _ = qkv.shape
    if invariant:
        b = torch.zeros(3 * B, dtype=torch.int32, device="cuda")
        L.moments_bound(L.chan_stats(qkv.view(B, N, 1, 3 * C), invariant=True), 0, C, b, invariant=True)
    else:
        b = torch.zeros(3, dtype=torch.int32, device="cuda")
        L.moments_bound(L.chan_stats(qkv.view(B, 1, N, 3 * C)), 0, C, b)
    return b


def workspace(c, plan):
    """(what ``lib.attention`` takes as ``ws``, the buffer): plan bytes + TAIL, every word the canary."""
    if c.ws == "none":
        return False, None
    if c.ws == "auto" and plan["ws_bytes"] == 0:
        return None, None
    buf = torch.full(((plan["ws_bytes"] + TAIL) // 4,), CANARY, dtype=torch.int32, device="cuda")
    return buf.view(torch.float32), buf


def launch(L, c, qkv, bounds, plan):
    """One call of the case through ``lib.attention``: (the padded output buffer, the workspace words, the profile record)."""
    B, N, C = qkv.shape[0], c.N, c.heads * c.D
    out = torch.full((B, N, C + PAD), 7.0, device="cuda")
    ws, words = workspace(c, plan)
    prof = []
    L.ATTN_PROFILE = prof
    try:
        with ledger.options(L, c.options):
            L.attention(qkv, C, c.heads, out=out, bounds=bounds, invariant=c.invariant, ws=ws)
    finally:
        L.ATTN_PROFILE = None
    assert len(prof) == 1
    return out, words, prof[0]


def launch_strided(L, c, qkv, bounds, plan):
    """The same call through the C ABI with q, k and v in three tensors of their own, rows C + 12 floats apart (the entry points
    take one row stride for the three)."""
    B, N, C, D = c.B, c.N, c.heads * c.D, c.D
    q, k, v = [torch.full((B, N, C + 12), float("nan"), device="cuda") for _ in range(3)]
    for t, src in zip((q, k, v), qkv.split(C, dim=2)):
        t[..., :C] = src
    out = torch.full((B, N, C + PAD), 7.0, device="cuda")
    ws, _ = workspace(c, plan)
    H = L.hip_lib()
    head = (L.fptr(q), L.fptr(k), L.fptr(v), C + 12, L.fptr(out), C + PAD, B, c.heads, N, D, D ** -0.5)
    wsp = None if ws is None or ws is False else L.ptr(ws)
    with ledger.options(L, c.options):
        if c.invariant:
            rc = H.evc_attention_invariant_f32(*head, None if bounds is None else L.ptr(bounds), wsp, L.stream_ptr())
        elif bounds is not None:
            rc = H.evc_attention_f16x3_f32(*head, L.ptr(bounds), wsp, L.stream_ptr())
        elif c.ws == "none":
            rc = H.evc_attention_f32(*head, L.stream_ptr())
        else:
            rc = H.evc_attention_ws_f32(*head, wsp, L.stream_ptr())
    assert rc == 0, rc
    return out


def _strided_cases():
    """One case per kernel family, the first of the table with more than one key tile."""
    first = {}
    for c in ledger.CASES:
        if c.N > 32:
            first.setdefault(ledger.family(c.cls), ledger.case_id(c))
    assert set(first) == set(ledger.FAMILIES)
    return set(first.values())


STRIDED = _strided_cases()


@pytest.mark.parametrize("c", ledger.CASES, ids=[ledger.case_id(c) for c in ledger.CASES])
def test_attention_plan_class_against_fp64(L, c):
    B, heads, N, D = c.B, c.heads, c.N, c.D
    C = heads * D
    qkv = make_qkv(c)
    bounds = bounds_of(L, qkv, C, c.invariant) if c.f16 else None
    by_sample = bool(c.invariant and c.f16)
    ref = softmax_attention(qkv, heads, torch.float64)
    e32 = rel_err(softmax_attention(qkv, heads, torch.float32), ref, by_sample)
    plan = ledger.case_plan(c, L)
    tail0 = plan["ws_bytes"] // 4

    out, words, prof = launch(L, c, qkv, bounds, plan)
    torch.cuda.synchronize()
    assert ledger.classify(prof, c.invariant) == c.cls, (prof, c.cls)             # the test ran the kernel it names
    assert prof["call"] == (B, heads, N, D, bool(c.f16), bool(c.invariant))
    assert {k: v for k, v in prof.items() if k != "call"} == plan
    err = rel_err(out[..., :C], ref, by_sample)
    print(f"LEDGER {ledger.case_id(c)} | {c.cls[0]}{' split' * c.cls[1]}{' inv' * c.cls[2]} | err {err:.3e} | f32 torch {e32:.3e}")
    assert err <= BAR, (err, e32)
    assert bool((out[..., C:] == 7.0).all())                                      # nothing written behind heads * D
    if words is not None:
        assert bool((words[tail0:] == CANARY).all()), "workspace overrun"

    again, words2, _ = launch(L, c, qkv, bounds, plan)
    assert torch.equal(again, out)
    if words is not None:
        assert bool((words2[tail0:] == CANARY).all())

    if c.invariant and B >= 2:          # sample 0 alone, same bound words: its rows of the batch bit for bit
        alone, _, _ = launch(L, c, qkv[:1].contiguous(), None if bounds is None else bounds[:3].contiguous(),
                             ledger.plan(L, 1, heads, N, D, c.f16, True))
        assert torch.equal(alone[0], out[0])

    if c.cls[1]:
        assert prof["kparts"] >= 2 and prof["merge"]
        single = torch.full((B, N, C + PAD), 7.0, device="cuda")
        L.attention(qkv, C, heads, out=single, ws=False)        # evc_attention_f32: one pass over the keys, no workspace
        e1 = rel_err(out[..., :C], single[..., :C], by_sample)
        print(f"LEDGER {ledger.case_id(c)} | against evc_attention_f32 {e1:.3e}")
        assert e1 <= SPLIT_BAR, e1

    if ledger.case_id(c) in STRIDED:
        assert torch.equal(launch_strided(L, c, qkv, bounds, plan), out)
