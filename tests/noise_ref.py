"""numpy restatement of the seeded stamp noise (include/dtp.h, dtp_stamp_seeded): Philox4x32-10 in uint64 arithmetic,
Box-Muller in float64, cast to float32 at the end.  The yardstick of csrc/noise.hip on the CPU and the GPU."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57   # multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85   # key increments (before rounds 2..10)
MASK = np.uint64(0xFFFFFFFF)
DRAW_LATENTS, DRAW_EPS_MASKED, DRAW_EPS_CONTEXT, DRAW_INIT_EPS = 0, 1, 2, 3


def philox4x32(ctr, key):
    """ctr uint [..., 4], key uint [..., 2] (broadcastable) -> uint32 [..., 4]: ten rounds of
    (c0,c1,c2,c3) -> (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0))."""
    ctr, key = np.asarray(ctr, dtype=np.uint64), np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (ctr[..., i] & MASK for i in range(4))
    k0, k1 = key[..., 0] & MASK, key[..., 1] & MASK
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2  # 32 x 32 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def words(seed, draw, n):
    """The uint32 words [n / 4, 4] behind the n elements of one draw of one stamp."""
    assert n > 0 and n % 4 == 0 and 0 <= draw <= 3 and 0 <= seed < 1 << 64
    q = np.arange(n // 4, dtype=np.uint64)
    ctr = np.stack([q & MASK, q >> np.uint64(32), np.full_like(q, draw), np.zeros_like(q)], axis=-1)
    return philox4x32(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))


def uniform(w):
    """u(w) = ((w >> 8) + 0.5) 2^-24 in float64: exact, inside (0, 1)."""
    return ((np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def normals(seed, draw, n, dtype=np.float32):
    """float32 [n]: elements 4q, 4q+1 from words (0, 1) of counter q as r cos t, r sin t; 4q+2, 4q+3 from words (2, 3)."""
    w = words(seed, draw, n)
    out = np.empty((n // 4, 4), dtype=np.float64)
    for j in (0, 2):
        r, t = np.sqrt(-2.0 * np.log(uniform(w[:, j]))), 2.0 * np.pi * uniform(w[:, j + 1])
        out[:, j], out[:, j + 1] = r * np.cos(t), r * np.sin(t)
    return out.reshape(n).astype(dtype)


def check_moments(z, what=""):
    """The bounds of a draw, stated for n = 2^20: |mean| <= 5e-3 (5 sigma of the mean), |var - 1| <= 1e-2 (7 sigma of the sample
    variance, sqrt(2 / n)); both are standard errors, so for another n they scale by sqrt(2^20 / n).  Every value finite and
    max |z| <= 5.9 at any n (24-bit u: sqrt(-2 ln 2^-25) = 5.887)."""
    z = np.asarray(z, dtype=np.float64)
    scale = np.sqrt(2.0 ** 20 / z.size)
    assert np.isfinite(z).all(), what
    assert np.abs(z).max() <= 5.9, (what, np.abs(z).max())
    assert abs(z.mean()) <= 5e-3 * scale, (what, z.mean())
    assert abs(z.var() - 1.0) <= 1e-2 * scale, (what, z.var())


def correlation(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.corrcoef(a, b)[0, 1])
