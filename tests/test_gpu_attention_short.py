"""The short-sequence attention kernels (csrc/attention.hip: attention_short_kernel / attention_short_f16_kernel, N <= 256
keys, option "short_seq"): one launch of 4-wave workgroups in which the waves cut the reduction over D of S^T = K Q^T and
deal out the D / 32 tiles of O^T = V^T P^T.  Shapes are the smallest at which each mechanism can go wrong."""
import functools

import pytest
import torch

from conftest import rnd

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    import evc_amd  # noqa: F401
    from evc_amd import lib
    lib.hip_lib()   # raises if libevc_hip.so is missing or the device is not gfx950: no silent fallback
    return lib


@pytest.fixture(params=[False, True], ids=["f32mfma", "f16x3"])
def f16(request):
    return request.param


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def attn_ref(qkv, C, heads):
    """float64 torch softmax attention of a (B, N, 3C) q | k | v tensor."""
    B, N, _ = qkv.shape
    D = C // heads
    q, k, v = [t.reshape(B, N, heads, D).permute(0, 2, 1, 3) for t in qkv.double().split(C, dim=2)]
    w = torch.softmax(torch.einsum("bhqd,bhkd->bhqk", q, k) * (D ** -0.5), dim=-1)
    return torch.einsum("bhqk,bhkd->bhqd", w, v).permute(0, 2, 1, 3).reshape(B, N, C)


@functools.lru_cache(maxsize=None)
def case(B, heads, N, D, peaked=False):
    """(qkv on the CPU, float64 reference): computed once per shape, shared by the tests, never modified."""
    C = heads * D
    q, k, v = rnd(61, B, N, C), rnd(62, B, N, C), rnd(63, B, N, C)
    if peaked:      # later keys dominate: the maximum moves from tile to tile (test_attention_peaked_scores_exercise_the_rescale)
        k = k * torch.linspace(0.5, 6.0, N)[None, :, None]
    qkv = torch.cat([q, k, v], 2)
    return qkv, attn_ref(qkv, C, heads)


def bounds_of(L, qkv, C):
    B, N, _ = qkv.shape
    b = torch.zeros(3, dtype=torch.int32, device="cuda")
    L.moments_bound(L.chan_stats(qkv.view(B, 1, N, 3 * C)), 0, C, b)
    return b


def run(L, qkv, C, heads, f16, bounds=None):
    """One attention call in the given arithmetic form.  The fp16 form is used from 128 keys on by default; below that the
    option "f16_min_keys" reaches it."""
    qkv = qkv.cuda()
    if not f16:
        return L.attention(qkv, C, heads)
    try:
        L.attention_set_option("f16_min_keys", 1)
        return L.attention(qkv, C, heads, bounds=bounds_of(L, qkv, C) if bounds is None else bounds)
    finally:
        L.attention_set_option("f16_min_keys", 128)


SHAPES = [(1, 1, 32, 32),       # one key tile
          (1, 4, 64, 192), (2, 2, 64, 192),      # the 8x8 level
          (2, 3, 256, 192),     # the 16x16 level, 8 tiles
          (1, 1, 40, 64),       # ragged last tile
          (3, 1, 200, 128),     # ragged, 7 tiles
          (2, 2, 96, 32),       # 3 tiles; D = 32: two k-steps of the fp16 form for 4 waves, one output tile
          (1, 2, 256, 32)]      # smallest D at the largest N


@pytest.mark.parametrize("B,heads,N,D", SHAPES)
def test_parity_with_float64(L, f16, B, heads, N, D):
    qkv, ref = case(B, heads, N, D)
    assert rel(run(L, qkv, heads * D, heads, f16), ref) < 2e-5


@pytest.mark.parametrize("N", [128, 256])
def test_peaked_scores(L, f16, N):
    qkv, ref = case(1, 1, N, 32, peaked=True)
    assert rel(run(L, qkv, 32, 1, f16), ref) < 2e-5


@pytest.mark.parametrize("B,heads,N,D", [(2, 4, 64, 192), (2, 3, 256, 192), (3, 1, 200, 128)])
def test_option_off_against_on(L, f16, B, heads, N, D):
    qkv, _ = case(B, heads, N, D)
    on = run(L, qkv, heads * D, heads, f16)
    try:
        L.attention_set_option("short_seq", 0)
        off = run(L, qkv, heads * D, heads, f16)
    finally:
        L.attention_set_option("short_seq", 1)
    assert rel(on, off) < 5e-6


@pytest.mark.parametrize("B,heads,N,D", [(2, 2, 64, 192), (2, 3, 256, 192)])
def test_two_calls_are_bitwise_equal(L, f16, B, heads, N, D):
    qkv, _ = case(B, heads, N, D)
    assert torch.equal(run(L, qkv, heads * D, heads, f16), run(L, qkv, heads * D, heads, f16))


@pytest.mark.parametrize("N", [256, 288])
def test_dispatch_boundary(L, f16, N):
    qkv, ref = case(1, 2, N, 64)
    assert rel(run(L, qkv, 128, 2, f16), ref) < 2e-5


@pytest.mark.parametrize("B,heads,N,D", [(2, 2, 64, 192), (1, 2, 200, 64)])
def test_nan_in_q_and_v_as_torch(L, B, heads, N, D):
    """f32 form (an fp16-form bound would be NaN itself): a NaN in q taints that query's row of that head and nothing else, a
    NaN in v[n, d] column d of that (sample, head) for every query, exactly where torch's float64 result is NaN."""
    C = heads * D
    qkv, _ = case(B, heads, N, D)
    h = heads - 1
    for name, (b, n, c) in {"q": (B - 1, N - 1, h * D + 3), "v": (0, 5, 2 * C + h * D + D - 1)}.items():
        x = qkv.clone()
        x[b, n, c] = NAN
        got, ref = run(L, x, C, heads, False).cpu(), attn_ref(x, C, heads)
        bad = torch.isnan(ref)
        assert bad.any() and not bad.all(), name
        assert torch.equal(torch.isnan(got), bad), name
        assert rel(torch.where(bad, torch.zeros_like(got), got), torch.where(bad, torch.zeros_like(ref), ref)) < 2e-5, name
    bad_q = torch.zeros(B, N, C, dtype=torch.bool)
    bad_q[B - 1, N - 1, h * D:(h + 1) * D] = True
    x = qkv.clone()
    x[B - 1, N - 1, h * D + 3] = NAN
    assert torch.equal(torch.isnan(run(L, x, C, heads, False).cpu()), bad_q)


@pytest.mark.parametrize("B,heads,N,D", [(1, 2, 64, 192), (1, 2, 256, 64)])
def test_nan_bound_poisons_the_fp16_form(L, B, heads, N, D):
    C = heads * D
    qkv, _ = case(B, heads, N, D)
    for word in range(3):
        bounds = bounds_of(L, qkv.cuda(), C)
        bounds[word] = 0x7FC00000
        assert bool(torch.isnan(run(L, qkv, C, heads, True, bounds=bounds)).all()), word


@pytest.mark.parametrize("heads,N,D", [(2, 64, 192), (3, 256, 192)])
def test_batch_independence(L, f16, heads, N, D):
    """B = 1 rows are bitwise the same sample's rows at B = 3 (same bound words): a workgroup never spans samples."""
    C = heads * D
    qkv, _ = case(3, heads, N, D)
    bounds = bounds_of(L, qkv.cuda(), C)
    all3 = run(L, qkv, C, heads, f16, bounds=bounds)
    for b in range(3):
        assert torch.equal(run(L, qkv[b:b + 1].contiguous(), C, heads, f16, bounds=bounds)[0], all3[b])
