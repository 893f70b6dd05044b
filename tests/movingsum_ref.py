"""The yardstick of `MovingSum(x, w)` / `MovingMean(x, w)` / `MovingRMS(x, w)` (include/sigops.h SO_NODE_MOVSUM;
csrc/k_movsum.hip): the window sum over ONE summation tree that depends on the absolute frame numbers, `back` and `ahead`
only, never on which frames are asked for.  Per channel, in Float64 (Float32 widens exactly; for the rms the addend is
x[k] * x[k], the product formed in Float64 and rounded once), with R = 16, B = 1024 and W = back + ahead + 1:

    padding  xp[k] = the addend for 0 <= k < N and -0.0 outside: -0.0 is the additive identity (v + -0.0 has the bits of v
             for every v, both zeros included), so padding equals clipping and a window of only -0.0 sums to -0.0
    W == 1   s[n] = xp[n], no addition
    segments S = min(B, the greatest power of two <= W - 1), from the nominal W; segment m is the frames [m S, (m + 1) S);
             runs are aligned groups of r = min(R, S) frames, L = S / r of them a segment
    P(k)     the prefix of k's segment up to k: the run summed left to right from its first frame; the L run totals through an
             inclusive Kogge-Stone scan, d = 1, 2, 4, .. < L: v[j] <- v[j - d] + v[j] for every j >= d at once; P(k) is the
             run prefix in run 0 and v[j - 1] + the run prefix in run j >= 1
    Q(k)     the mirror image: the run summed right to left from its last frame, the scan v[j] <- v[j] + v[j + d], Q(k) the
             run suffix in the last run and the run suffix + v[j + 1] before it
    window   lo = n - back, hi = n + ahead, a = floor(lo / S), b = floor(hi / S) (b > a always):
             s[n] = Q(lo) + P(hi) when b == a + 1, else (Q(lo) + M) + P(hi)
    M        the segments a + 1 .. b - 1: node (0, m) = t[m] = P((m + 1) S - 1), node (l, q) = node (l - 1, 2 q) +
             node (l - 1, 2 q + 1); M adds the canonical cover of [a + 1, b - 1] by maximal aligned nodes left to right: at
             p, the greatest l with 2^l | p and p + 2^l <= b, then p += 2^l.  For S < B that is the one node t[a + 1].

every + one rounded Float64 addition.  mean = s / cnt and rms = sqrt(q / cnt), cnt[n] = min(N - 1, n + ahead) -
max(0, n - back) + 1 as a Float64, q the same sum over the squares, every operation rounded once.

Error bound.  No partial sum is ever subtracted, so an addend's rounding errors are those of the additions it passes through:
at most R - 1 = 15 inside its run, log2(B / R) = 6 in the scan, l inside a node of level l, one for every further node of the
cover (a cover whose greatest level is lv has at most 2 lv + 2 nodes), and 2 to join Q, M and P.  With lv =
floor(log2((W - 1) / B)) for W - 1 >= B, else 0, that is at most K(W) = 24 + 3 lv additions, each with a relative error
of at most u = 2^-53, so |s - exact| <= ((1 + u)^K - 1) sum |xp| <= K u (1 + K u) sum |window|.  `math.fsum` is the exact sum
rounded once, at most u sum |window| from it: |s - fsum| <= (K(W) + 1)(1 + K u) * 2^-53 * sum |window| (`error_units`);
tests/test_movingsum_host.py measures 4.0 of these units at worst over 2^-60 .. 2^60.

Two forms: `movsum_loop`, plain loops over Python floats that follow the text above, and `movsum_1d`, the same tree in
NumPy array operations for the larger cases.  tests/test_movingsum_host.py holds the second to the first bit for bit; the
device is held to `movingsum_ref` bit for bit in tests/test_gpu_movingsum.py."""
import math
import re
from pathlib import Path

import numpy as np


def _constant(name):
    text = (Path(__file__).resolve().parent.parent / "signaloperators.jl_amd" / "csrc" / "kernels.h").read_text()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


R = 16      # frames of a run
B = 1024    # the longest segment
SUM, MEAN, RMS = 0, 1, 2


def kernel_constants():
    """(R, B, tile, halo) as the kernel has them (csrc/kernels.h kMsumRun, kMsumBlock, kMsumTile, kMsumHalo): the tests hold
    R and B to this file's; a workgroup's output frames, and the longest window less one that the one-launch form takes"""
    return _constant("kMsumRun"), _constant("kMsumBlock"), _constant("kMsumTile"), _constant("kMsumHalo")


def segment(W):
    """S of a window of W >= 2 frames"""
    return min(B, 1 << ((W - 1).bit_length() - 1))


def error_units(W):
    """the bound on |s - fsum(window)| in units of 2^-53 * sum |window| (the docstring's derivation)"""
    lv = ((W - 1) // B).bit_length() - 1 if W - 1 >= B else 0
    K = 24 + 3 * lv
    return (K + 1) * (1.0 + K * 2.0 ** -53)


def cover(a, b):
    """the canonical cover of the segments [a + 1, b - 1] by maximal aligned nodes, left to right: [(level, index)]"""
    out = []
    p = a + 1
    while p < b:
        l = 0
        while p % (2 << l) == 0 and p + (2 << l) <= b:
            l += 1
        out.append((l, p >> l))
        p += 1 << l
    return out


# ---- (a) the definition, one Python float after the other --------------------------------------------------------------
def movsum_loop(x, back, ahead):
    """one channel of addends (Float64) -> the window sums; plain loops over Python floats"""
    xs = [float(v) for v in np.asarray(x, dtype=np.float64)]
    N = len(xs)
    W = back + ahead + 1
    if W == 1:
        return np.array(xs, dtype=np.float64)
    S = segment(W)
    r = min(R, S)
    L = S // r

    def xp(k):
        return xs[k] if 0 <= k < N else -0.0

    segs = {}

    def seg(m):
        """(P, Q) of segment m as lists of S floats; a segment wholly outside the signal is all -0.0"""
        if m in segs:
            return segs[m]
        if (m + 1) * S <= 0 or m * S >= N:
            segs[m] = ([-0.0] * S, [-0.0] * S)
            return segs[m]
        f0 = m * S
        pre, suf = [0.0] * S, [0.0] * S
        for j in range(L):
            s = None
            for e in range(r):
                v = xp(f0 + j * r + e)
                s = v if s is None else s + v
                pre[j * r + e] = s
            s = None
            for e in range(r - 1, -1, -1):
                v = xp(f0 + j * r + e)
                s = v if s is None else v + s
                suf[j * r + e] = s
        v = [pre[j * r + r - 1] for j in range(L)]
        d = 1
        while d < L:
            v = [v[j] if j < d else v[j - d] + v[j] for j in range(L)]
            d *= 2
        P = [pre[i] if i < r else v[i // r - 1] + pre[i] for i in range(S)]
        v = [suf[j * r] for j in range(L)]
        d = 1
        while d < L:
            v = [v[j] if j + d >= L else v[j] + v[j + d] for j in range(L)]
            d *= 2
        Q = [suf[i] if i // r == L - 1 else suf[i] + v[i // r + 1] for i in range(S)]
        segs[m] = (P, Q)
        return segs[m]

    nodes = {}

    def node(l, q):
        if (l, q) not in nodes:
            if ((q + 1) << l) * S <= 0 or (q << l) * S >= N:
                nodes[(l, q)] = -0.0  # (a sum of -0.0 alone)
            elif l == 0:
                nodes[(l, q)] = seg(q)[0][S - 1]
            else:
                nodes[(l, q)] = node(l - 1, 2 * q) + node(l - 1, 2 * q + 1)
        return nodes[(l, q)]

    covers = {}
    y = [0.0] * N
    for n in range(N):
        lo, hi = n - back, n + ahead
        a, b = lo // S, hi // S
        assert b > a
        Qlo = seg(a)[1][lo - a * S]
        Phi = seg(b)[0][hi - b * S]
        if b == a + 1:
            y[n] = Qlo + Phi
            continue
        if (a, b) not in covers:
            M = None
            for (l, q) in cover(a, b):
                M = node(l, q) if M is None else M + node(l, q)
            covers[(a, b)] = M
        y[n] = (Qlo + covers[(a, b)]) + Phi
    return np.array(y, dtype=np.float64)


# ---- (b) the same tree in array operations ---------------------------------------------------------------------------------
def _prefix(seg, r):
    """seg: [segments][S] -> the prefix P of every segment"""
    ns, S = seg.shape
    L = S // r
    run = np.add.accumulate(seg.reshape(ns, L, r), axis=2)  # (sequential, left to right)
    v = run[:, :, -1].copy()
    d = 1
    while d < L:
        v[:, d:] = v[:, :-d].copy() + v[:, d:]
        d *= 2
    P = run.copy()
    P[:, 1:, :] = v[:, :-1, None] + run[:, 1:, :]
    return P.reshape(ns, S)


def movsum_1d(x, back, ahead):
    """one channel of addends (Float64) -> the window sums"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    N = x.size
    W = back + ahead + 1
    if W == 1 or N == 0:
        return x.copy()
    S = segment(W)
    r = min(R, S)
    # only the segments that hold a sample are formed; every other one is -0.0 throughout
    m1 = -(-N // S)
    seg = np.full(m1 * S, -0.0)
    seg[:N] = x
    seg = seg.reshape(m1, S)
    with np.errstate(all="ignore"):
        P = _prefix(seg, r)
        Q = _prefix(seg[:, ::-1], r)[:, ::-1]  # (the mirror image: + commutes bit for bit)
        n = np.arange(N)
        lo, hi = n - back, n + ahead
        a, b = lo // S, hi // S
        inside = lo >= 0
        Qlo = np.where(inside, Q.ravel()[np.where(inside, lo, 0)], -0.0)
        inside = hi < m1 * S
        Phi = np.where(inside, P.ravel()[np.where(inside, hi, 0)], -0.0)
        t = {0: P[:, -1].copy()}

        def node(l, q):
            if q < 0 or (q << l) >= m1:
                return np.float64(-0.0)
            if l not in t:
                prev = np.array([node(l - 1, k) for k in range(2 * (((m1 - 1) >> l) + 1))])
                t[l] = prev[0::2] + prev[1::2]
            return t[l][q]

        M = np.full(N, -0.0)
        mid = b - a > 1
        pairs = np.unique(np.stack([a[mid], b[mid]], axis=1), axis=0) if mid.any() else []
        for (ai, bi) in pairs:
            m = None
            for (l, q) in cover(int(ai), int(bi)):
                m = node(l, q) if m is None else m + node(l, q)
            M[(a == ai) & (b == bi)] = m
        # (Q + -0.0 has the bits of Q: where no whole segment lies in between this is Q + P)
        return (Qlo + M) + Phi


def counts(N, back, ahead):
    n = np.arange(N)
    return (np.minimum(N - 1, n + ahead) - np.maximum(0, n - back) + 1).astype(np.float64)


def _planar(x):
    x = np.asarray(x)
    return x.reshape(x.shape[0], -1).astype(np.float64)  # (Float32 widens exactly)


def movingsum_ref(x, back, ahead, op=SUM, one=movsum_1d):
    """frames x channels (or a vector) -> frames x channels Float64, planar; op: SUM, MEAN or RMS"""
    x = _planar(x)
    y = np.empty(x.shape, order="F")
    with np.errstate(all="ignore"):
        for c in range(x.shape[1]):
            v = np.ascontiguousarray(x[:, c])
            s = one(v * v if op == RMS else v, back, ahead)
            if op != SUM:
                s = s / counts(v.size, back, ahead)
            y[:, c] = np.sqrt(s) if op == RMS else s
    return y


def same_bits(a, b):
    """equal bit for bit, the sign of zero included; NaNs equal NaNs (their payloads are not compared)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(np.ascontiguousarray(a[ok]).view(np.int64), np.ascontiguousarray(b[ok]).view(np.int64))


def fsum_windows(x, back, ahead):
    """one channel -> (math.fsum of every clipped window, the sum of its magnitudes)"""
    v = [float(s) for s in x]
    N = len(v)
    ex, mag = np.empty(N), np.empty(N)
    for n in range(N):
        w = v[max(0, n - back):min(N - 1, n + ahead) + 1]
        ex[n] = math.fsum(w)
        mag[n] = math.fsum(abs(s) for s in w)
    return ex, mag


# ---- the inputs of the tests --------------------------------------------------------------------------------------------
TILE = 2048
# the smallest shapes that cross a run, a block and a tile, with ragged ends; the last two have several tiles and blocks
LENGTHS = [1, R - 1, R, R + 1, B - 1, B, B + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 77, 12 * B + 77]
SHORT_WINDOWS = [1, 2, 3, 16, 17, 18, 33, 480, 1024, 1025]        # the one-launch form and its last window
LONG_WINDOWS = [1026, 2049, 2050, 4097, 7 * 1024 + 5]              # (and N + 5): covers of one, two and three nodes, levels 0 .. 2
CHANNELS = [1, 3, 8]


def aheads(w):
    """causal, centred, fully ahead"""
    return sorted({0, (w - 1) // 2, w - 1})


def signal(N, C, dtype=np.float64, seed=0):
    """N frames x C channels of normal samples (planar)"""
    rng = np.random.default_rng(1000 * N + 10 * C + seed)
    return np.asfortranarray(rng.standard_normal((N, C)).astype(dtype))


def wide(N, C, seed=0):
    """magnitudes from 2^-60 to 2^60, both signs: the order of the additions shows in the bits"""
    rng = np.random.default_rng(7000 * N + 10 * C + seed)
    return np.asfortranarray(rng.standard_normal((N, C)) * np.exp2(rng.integers(-60, 61, (N, C)).astype(np.float64)))


def small_ints(N, C, seed=0):
    """small integers: every order of the additions is exact"""
    rng = np.random.default_rng(3000 * N + 10 * C + seed)
    return np.asfortranarray(rng.integers(-8, 9, (N, C)).astype(np.float64))


def planted(N, C, dtype=np.float64, seed=0):
    """normal samples with +-0 planted on both sides of run, segment, block and tile boundaries, one of +Inf, -Inf or NaN
    a channel at such a boundary (channel 1 has +Inf AND -Inf, a window's reach apart at most), and a channel of -0.0"""
    x = signal(N, C, dtype, seed + 1)
    marks = [m for m in (R - 1, R, 2 * R, B - 1, B, TILE - 1, TILE, 3 * B, 2 * TILE) if m < N]
    for c in range(C):
        for k, at in enumerate(marks):
            x[at, c] = (-0.0, 0.0)[(k + c) % 2]
        if marks and N > 3:
            at = marks[(len(marks) - 1 - c) % len(marks)]
            x[at, c] = (np.inf, -np.inf, np.nan)[c % 3]
            if c % 3 == 1 and at >= 3:
                x[at - 3, c] = np.inf
    if C >= 3:
        x[:, C - 1] = -0.0
    return x
