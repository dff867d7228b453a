"""CPU restatement of noise specification N1, written from the specification, not from the kernel:
Philox4x32-10 in uint64 arithmetic for the 32 x 32 products, the normal stage in float64.

    key     = (seed low 32 bits, seed high 32 bits)
    counter = (j, step, start frame, stream id),  j = index of the 4-element block inside the sample
    words w0..w3 -> elements 4j .. 4j+3:  u = ((w >> 9) + 0.5) * 2^-23,  r = sqrt(-2 ln u(w0)),  theta = 2 pi u(w1):
    r cos theta, r sin theta; the same from (w2, w3)
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of 32-bit words, key: 2 -> 4 uint64 arrays holding the 32-bit output words."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
        p0 = np.uint64(M0) * c[0]                 # < 2^64: exact in uint64
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
    return c


def words(seed, stream_id, start, step, n):
    """The raw words of one sample's step in memory order: (n,) uint32."""
    assert n % 4 == 0
    j = np.arange(n // 4, dtype=np.uint64)
    w = philox4x32_10((j, step, start, stream_id), (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    return np.stack(w, 1).reshape(-1).astype(np.uint32)


def normals(seed, stream_id, start, step, n):
    """One sample's step: (n,) float64."""
    w = words(seed, stream_id, start, step, n).reshape(-1, 2).astype(np.uint64)
    u = ((w >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    r = np.sqrt(-2.0 * np.log(u[:, 0]))
    th = 2.0 * np.pi * u[:, 1]
    return np.stack([r * np.cos(th), r * np.sin(th)], 1).reshape(-1)
