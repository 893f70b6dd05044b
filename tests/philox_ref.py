"""NumPy restatement of the counter-based noise generator (`so.DeviceRNG`), written from its specification and
independent of the engine: Philox4x32-10 in `uint64` arithmetic, the Box-Muller transform in `np.longdouble` with an
exactly reduced `sincospi`, rounded to Float64 once at the end.

Frame i (0-based, absolute) of the noise (seed, stream):
    p = i >> 1
    x0..x3 = Philox4x32-10(counter = (p lo, p hi, stream lo, stream hi), key = (seed lo, seed hi))
    u1 = ((x1:x0 >> 11) + 1) * 2^-53,  u2 = (x3:x2 >> 11) * 2^-53
    r = sqrt(-2 log u1);  frame i = r cospi(2 u2) for even i, r sinpi(2 u2) for odd i
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or integers) of 32-bit words, key: two; returns the four output words as uint64 arrays"""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & MASK for w in counter]
    k = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & MASK for w in key]
    for _ in range(10):
        p0 = M0 * c[0]  # < 2^64: both factors are below 2^32
        p1 = M1 * c[2]
        c = [(p1 >> S32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> S32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return c


def uniforms(seed, stream, pairs):
    """(u1, u2) of the pair indices `pairs`, as Float64 (both conversions are exact)"""
    p = np.asarray(pairs, dtype=np.uint64)
    seed, stream = np.uint64(seed), np.uint64(stream)
    x0, x1, x2, x3 = philox4x32_10((p & MASK, p >> S32, stream & MASK, stream >> S32), (seed & MASK, seed >> S32))
    a = ((x1 << S32) | x0) >> np.uint64(11)
    b = ((x3 << S32) | x2) >> np.uint64(11)
    u1 = (a + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = b.astype(np.float64) * 2.0 ** -53
    return u1, u2


def _sincospi(x):
    """sin(pi x), cos(pi x) of Float64 x in [0, 2) in long double, with an exact reduction to |t| <= 1/4"""
    k = np.rint(2.0 * x)
    t = (x - 0.5 * k).astype(np.longdouble)  # exact in Float64 already
    pi = np.longdouble("3.14159265358979323846264338327950288")
    s, c = np.sin(pi * t), np.cos(pi * t)
    q = k.astype(np.int64) & 3
    rs = np.where(q & 1, c, s)
    rc = np.where(q & 1, s, c)
    return np.where(q & 2, -rs, rs), np.where((q == 1) | (q == 2), -rc, rc)


def randn(seed, stream, start, n):
    """frames [start, start + n) of the noise (seed, stream) as Float64"""
    start, n = int(start), int(n)
    i = np.arange(start, start + n, dtype=np.uint64) if n else np.zeros(0, dtype=np.uint64)
    u1, u2 = uniforms(seed, stream, i >> np.uint64(1))
    r = np.sqrt(np.longdouble(-2.0) * np.log(u1.astype(np.longdouble)))
    s, c = _sincospi(2.0 * u2)
    z = np.where((i & np.uint64(1)).astype(bool), r * s, r * c)
    return z.astype(np.float64)
