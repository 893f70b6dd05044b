"""The yardstick of `Recur2(a1, a2, b)`, `Resonator` and `Sweep` (include/sigops.h SO_NODE_RECUR2; csrc/k_recur2.hip): the
second-order scan

    y[0] = b[0]   y[1] = (a1[1] y[0] + a2[1] (+0.0)) + b[1]   y[n] = (a1[n] y[n-1] + a2[n] y[n-2]) + b[n]

over ONE tree that depends on the frame index only, never on how many frames are asked for.  Per channel, in Float64
(Float32 widens exactly); every product and every sum rounded on its own, nothing contracted into an FMA; a1[0] and a2[0]
multiply nothing.  With the constants of `Cumsum` (L = 16, W = 64, T = 1024, G = 16, CH = 16384), an element of the scan is
(M, v), M 2x2 and v a two-vector: the affine map s -> M s + v on the state s = (y[n], y[n-1]).

    join   of a later element with an earlier one, (M2, v2) o (M1, v1):
               M[i][j] = M2[i][0] M1[0][j] + M2[i][1] M1[1][j]      v[i] = (M2[i][0] v1[0] + M2[i][1] v1[1]) + v2[i]
           in DOUBLE-DOUBLE arithmetic: every entry of a joined element is an unevaluated sum high + low of two Float64,
           formed by error-free transformations that are themselves plain Float64 operations in a fixed order (below)
    apply  of an element to a state: s'[i] = (M[i][0] s[0] + M[i][1] s[1]) + v[i], formed as a double-double, its high word kept
    run    j of a tile: at its first frame M = [[a1, a2], [1, 0]], v = (b, +0.0); every further frame SHIFTS:
               row 0 <- a1 row 0 + a2 row 1 (three entries M00, M01, v0 -- and b added to v0 last), row 1 <- the old row 0
           (a literal 1 * x + 0 * y would turn an Inf in y into NaN), all in Float64, every product and sum rounded once; the
           run's total E_j is its last (M, v), low words 0
    tile   an inclusive Kogge-Stone scan over the totals: for d = 1, 2, .. 32 and every j >= d at once, E_j <- E_j o E_{j-d};
           the tile's total K is E_63
    chunk  G_0 = K_0, G_k = K_k o G_{k-1}, tile after tile (chunk-local): the chunk's own composite
    signal S_1 = the v of chunk 0's G_15; S_{c+1} = G_15 of chunk c applied to S_c: the state that enters chunk c + 1

    the state that enters tile k of chunk c:   k = 0: S_c (chunk 0: none);  k >= 1: K_{k-1} applied to the state that entered
                                               tile k - 1 (none entered it: the v of K_{k-1} alone): a state, not a composite,
                                               goes from tile to tile
    the state that enters run j of that tile:  j = 0: the tile's;  j >= 1: E_{j-1} applied to the tile's (none: its v alone)
    the outputs of a run: the recurrence itself, walked from the state (s0, s1) that entered it: y = (a1 s0 + a2 s1) + b,
           (s0, s1) <- (y, s0).  Run 0 of the signal has no state: y[0] = b[0] itself, and it goes on from (y[0], +0.0).

So inside a run the outputs are the sequential loop's own operations, and every carried state comes from composites.
With the joins in plain Float64 this definition missed the 1e-8 contract where poles lie within 0.003 rad of z = 1 (4.6e-8
against the loop's 4.5e-12): a join's products of entries ~ 1 / sin(theta) cancel, and the same rounded composite repeats
run after run.  Double-double joins bring the worst listed input to 7.9e-10 (tests/test_recur2_host.py).
"Its v alone" is not "applied to a zero state": M 0 + v would lose the sign of a -0.0 and make NaN of an Inf in M.

Here: in NumPy array operations (`recur2_ref`), restated as plain loops over Python floats (`recur2_tree_loop`), next to
the sequential loop (`recur2_loop`) and the same loop in extended precision (`recur2_loop_ext`, `np.longdouble`, the x87
80-bit type where `EXTENDED` is true) that the accuracy tests compare with, and the inputs the device tests read.  NaN
payloads are outside the contract; the sign of zero and the place of +-Inf and NaN are inside it.

Two known properties, pinned in tests/test_recur2_host.py:
  * joins are general products: an Inf that meets a zero entry of M (an exact zero, or a product of coefficients that
    underflowed) gives NaN where the loop keeps the Inf (`inf_example`: NaN from frame 2 L on);
  * coefficients that are unstable over long stretches overflow the products, and Inf * 0 gives NaN where the loop is
    still finite (`overflow_example`: NaN from frame T + 34 L on).
The operators are meant for stable coefficients; this file is the definition there too."""
import math

import numpy as np

from cumsum_ref import CH, G, L, T, W, kernel_constants, same_bits  # noqa: F401  (the tree's constants are Cumsum's)
from recur_ref import signal, wide  # noqa: F401  (the inputs b of the device tests are Recur's)

EXTENDED = np.finfo(np.longdouble).nmant == 63


# ---- elements ------------------------------------------------------------------------------------------------------------
# An element is a tuple of twelve arrays or Python floats, the same code serves both: (M00, M01, M10, M11, v0, v1), the high
# words, then their six low words.  An entry is the unevaluated sum high + low (a double-double): the joins' products of
# entries ~ 1 / sin(theta) cancel to results of that size again, and in plain Float64 that cancellation costs poles next to
# z = 1 four digits more than the loop loses (DESIGN.md "Recur2", accuracy).  The error-free transformations below are
# plain Float64 operations, each rounded once, in this order, nothing fused -- Dekker's product through Veltkamp's split,
# Knuth's sum -- so that NumPy and the device give the same bits; a low word that is not finite (an operand was, or the
# split overflowed) is replaced by 0.0, which leaves the high word what plain arithmetic gives.
SPLIT = 134217729.0  # 2^27 + 1


def fin(e):
    if isinstance(e, np.ndarray):
        return np.where(np.isfinite(e), e, 0.0)
    return e if math.isfinite(e) else 0.0


def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, fin((a - (s - bb)) + (b - bb))


def quick_two_sum(a, b):
    s = a + b
    return s, fin(b - (s - a))


def split(a):
    c = SPLIT * a
    h = c - (c - a)
    return h, a - h


def two_prod(a, b):
    p = a * b
    ah, al = split(a)
    bh, bl = split(b)
    return p, fin((((ah * bh - p) + ah * bl) + al * bh) + al * bl)


def dd_mul(xh, xl, yh, yl):
    p, e = two_prod(xh, yh)
    return quick_two_sum(p, fin(e + (xh * yl + xl * yh)))


def dd_mul_d(xh, xl, y):
    """a double-double times a Float64"""
    p, e = two_prod(xh, y)
    return quick_two_sum(p, fin(e + xl * y))


def dd_add(xh, xl, yh, yl):
    s, e = two_sum(xh, yh)
    return quick_two_sum(s, fin(e + (xl + yl)))


def _dot(ah, al, Ah, Al, bh, bl, Ch, Cl):
    """a A + b C"""
    return dd_add(*dd_mul(ah, al, Ah, Al), *dd_mul(bh, bl, Ch, Cl))


def join(e2, e1):
    """(M2, v2) o (M1, v1): the later element e2 after the earlier e1, every entry a double-double"""
    a, b, c, d, p, q, al, bl, cl, dl, pl, ql = e2
    A, B, C, D, P, Q, Al, Bl, Cl, Dl, Pl, Ql = e1
    m00 = _dot(a, al, A, Al, b, bl, C, Cl)
    m01 = _dot(a, al, B, Bl, b, bl, D, Dl)
    m10 = _dot(c, cl, A, Al, d, dl, C, Cl)
    m11 = _dot(c, cl, B, Bl, d, dl, D, Dl)
    v0 = dd_add(*_dot(a, al, P, Pl, b, bl, Q, Ql), p, pl)
    v1 = dd_add(*_dot(c, cl, P, Pl, d, dl, Q, Ql), q, ql)
    hi, lo = zip(m00, m01, m10, m11, v0, v1)
    return tuple(hi) + tuple(lo)


def apply(e, s):
    """the state (s0, s1) behind the element e: formed as double-doubles, the high words kept"""
    a, b, c, d, p, q, al, bl, cl, dl, pl, ql = e
    t0 = dd_add(*dd_add(*dd_mul_d(a, al, s[0]), *dd_mul_d(b, bl, s[1])), p, pl)
    t1 = dd_add(*dd_add(*dd_mul_d(c, cl, s[0]), *dd_mul_d(d, dl, s[1])), q, ql)
    return (t0[0], t1[0])


def enter(e, s):
    """the state behind e where s entered it; no state (None): the v of e alone (its high words)"""
    return (e[4], e[5]) if s is None else apply(e, s)


# ---- the definition, in array operations ----------------------------------------------------------------------------------
def _planar(x):
    x = np.asarray(x)
    return x.reshape(x.shape[0], -1).astype(np.float64)  # (Float32 widens exactly)


def coefficients(a, N, C):
    """`a` as the node takes it -- a number, one channel (broadcast) or C channels, at least N frames -- -> N x C Float64"""
    if np.ndim(a) == 0:
        return np.full((N, C), np.float64(a))
    a = _planar(a)[:N]
    assert a.shape[0] == N and a.shape[1] in (1, C)
    return np.broadcast_to(a, (N, C)) if a.shape[1] != C else a


def _tiles(x, nt):
    """N x C -> [C][nt][W][L], padded with zeros (a padded frame enters no frame that exists)"""
    N, C = x.shape
    p = np.zeros((nt * T, C))
    p[:N] = x
    return np.ascontiguousarray(p.T).reshape(C, nt, W, L)


def recur2_ref(a1, a2, b):
    """`b` frames x channels (or a vector), `a1`, `a2` numbers or arrays -> frames x channels Float64, planar"""
    b = _planar(b)
    N, C = b.shape
    nt = -(-N // T)
    A1, A2, B = _tiles(coefficients(a1, N, C), nt), _tiles(coefficients(a2, N, C), nt), _tiles(b, nt)
    with np.errstate(all="ignore"):
        # the runs' totals, every run of every tile at once
        m00, m01, v0 = A1[..., 0].copy(), A2[..., 0].copy(), B[..., 0].copy()
        m10, m11, v1 = np.ones_like(m00), np.zeros_like(m00), np.zeros_like(m00)
        for m in range(1, L):
            x1, x2 = A1[..., m], A2[..., m]
            n00, n01, nv0 = x1 * m00 + x2 * m10, x1 * m01 + x2 * m11, (x1 * v0 + x2 * v1) + B[..., m]
            m10, m11, v1 = m00, m01, v0
            m00, m01, v0 = n00, n01, nv0
        E = (m00, m01, m10, m11, v0, v1) + tuple(np.zeros_like(m00) for _ in range(6))
        d = 1
        while d < W:
            J = join(tuple(x[..., d:] for x in E), tuple(x[..., :-d] for x in E))
            E = tuple(np.concatenate((x[..., :d], y), axis=-1) for x, y in zip(E, J))
            d *= 2
        # the state that enters every tile: tiles and chunks one after the other
        s0, s1 = np.zeros((C, nt, W)), np.zeros((C, nt, W))  # the state that enters every run
        live = np.zeros((nt, W), dtype=bool)
        S = None  # entering the chunk
        for c0 in range(0, nt, G):
            Gk = None
            st = S  # entering the tile: the chunk's state, then tile after tile
            for k in range(c0, min(c0 + G, nt)):
                pre = tuple(x[:, k, :-1] for x in E)  # the exclusive prefixes of the runs 1 .. 63
                if st is not None:
                    s0[:, k, 0], s1[:, k, 0] = st
                    live[k, 0] = True
                    s0[:, k, 1:], s1[:, k, 1:] = apply(pre, (st[0][:, None], st[1][:, None]))
                else:
                    s0[:, k, 1:], s1[:, k, 1:] = pre[4], pre[5]
                live[k, 1:] = True
                K = tuple(x[:, k, W - 1] for x in E)
                st = enter(K, st)
                Gk = K if Gk is None else join(K, Gk)
            S = enter(Gk, S)
        # the outputs: the recurrence itself from the state that entered the run
        Y = np.empty((C, nt, W, L))
        for m in range(L):
            y = (A1[..., m] * s0 + A2[..., m] * s1) + B[..., m]
            if m == 0:
                y = np.where(live, y, B[..., 0])  # (run 0 of the signal: the sample itself)
                s1 = np.where(live, s0, 0.0)
            else:
                s1 = s0
            s0 = y
            Y[..., m] = y
    return np.asfortranarray(Y.reshape(C, nt * T)[:, :N].T)


# ---- the same tree, one Python float after the other ----------------------------------------------------------------------
def recur2_tree_loop(a1, a2, b):
    """one channel, plain loops over Python floats (IEEE doubles): nothing shared with the block form but join and apply"""
    a1 = [float(v) for v in np.asarray(a1, dtype=np.float64)]
    a2 = [float(v) for v in np.asarray(a2, dtype=np.float64)]
    b = [float(v) for v in np.asarray(b, dtype=np.float64)]
    n = len(b)
    y = [0.0] * n
    S = None
    for c0 in range(0, n, CH):
        Gk = None
        st = S
        for t0 in range(c0, min(c0 + CH, n), T):
            t1 = min(t0 + T, n)
            nr = -(-(t1 - t0) // L)
            E = []
            for j in range(nr):
                lo = t0 + L * j
                m00, m01, m10, m11, v0, v1 = a1[lo], a2[lo], 1.0, 0.0, b[lo], 0.0
                for i in range(lo + 1, min(lo + L, t1)):
                    n00, n01, nv0 = a1[i] * m00 + a2[i] * m10, a1[i] * m01 + a2[i] * m11, (a1[i] * v0 + a2[i] * v1) + b[i]
                    m10, m11, v1 = m00, m01, v0
                    m00, m01, v0 = n00, n01, nv0
                E.append((m00, m01, m10, m11, v0, v1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0))
            d = 1
            while d < W:
                E = [E[j] if j < d else join(E[j], E[j - d]) for j in range(nr)]
                d *= 2
            for j in range(nr):
                lo = t0 + L * j
                s = st if j == 0 else enter(E[j - 1], st)
                for i in range(lo, min(lo + L, t1)):
                    if s is None:
                        y[i] = b[i]
                        s = (y[i], 0.0)
                    else:
                        y[i] = (a1[i] * s[0] + a2[i] * s[1]) + b[i]
                        s = (y[i], s[0])
            st = enter(E[nr - 1], st)
            Gk = E[nr - 1] if Gk is None else join(E[nr - 1], Gk)  # (a ragged tile is the last: nothing reads these)
        S = enter(Gk, S)
    return np.array(y)


# ---- the sequential recurrence ---------------------------------------------------------------------------------------------
def recur2_loop(a1, a2, b):
    """one channel, one frame after the other"""
    a1 = [float(v) for v in np.asarray(a1, dtype=np.float64)]
    a2 = [float(v) for v in np.asarray(a2, dtype=np.float64)]
    b = [float(v) for v in np.asarray(b, dtype=np.float64)]
    y = [0.0] * len(b)
    for i in range(len(b)):
        if i == 0:
            y[0] = b[0]
        else:
            y[i] = (a1[i] * y[i - 1] + a2[i] * (y[i - 2] if i >= 2 else 0.0)) + b[i]
    return np.array(y)


def recur2_loop_ext(a1, a2, b):
    """the same loop in `np.longdouble` (80-bit where EXTENDED): what the accuracy of the tree AND of the loop is measured against"""
    a1, a2, b = (np.asarray(v, dtype=np.float64).astype(np.longdouble) for v in (a1, a2, b))
    y = np.zeros(len(b), dtype=np.longdouble)
    p1 = p2 = np.longdouble(0)
    for i in range(len(b)):
        v = b[i] if i == 0 else (a1[i] * p1 + a2[i] * p2) + b[i]
        y[i] = v
        p2, p1 = p1, v
    return y


# ---- the two pinned non-finite examples -------------------------------------------------------------------------------------
def inf_example():
    """-> (a1, a2, b): the constants (2^-70, 2^-140), b = 0 but for b[0] = 1 and an Inf at frame 3, 3 L frames.  The loop gives
    +Inf from frame 3 on.  So does the tree up to frame 2 L - 1; from frame 2 L = 32 on it gives NaN: the total of run 1 has
    M01 ~ 2^-1120, which underflows to 0, and the join with run 0's v = (Inf, Inf) multiplies that zero by Inf"""
    b = np.zeros(3 * L)
    b[0], b[3] = 1.0, np.inf
    return 2.0 ** -70, 2.0 ** -140, b


def overflow_example():
    """-> (a1, a2, b): the constants (4, -1) (poles 2 +- sqrt 3), b = 0 throughout, 2 T frames.  The loop gives +0.0 everywhere.
    So does the tree in tile 0, which no state enters (a prefix contributes its v alone); in tile 1 the prefixes are applied
    to the state (0, 0), and from run 34 on their M, ~ 3.73^(16 j), has passed 2^1024: Inf * 0 is NaN from frame
    T + 34 L = 1568 on"""
    return 4.0, -1.0, np.zeros(2 * T)


# ---- the inputs of the device tests ----------------------------------------------------------------------------------------
LENGTHS = [1, 2, 3, L - 1, L, L + 1, L + 2, T - 1, T, T + 1, T + 2, CH - 1, CH, CH + 1, CH + 2, 2 * CH + 1, 3 * CH + 77]
CHANNELS = [1, 3, 8]
COEFS = ["reson", "u1h"]


def coef(kind, N, C, seed=0):
    """-> (a1, a2), N x C each: stable resonator pairs (r in [0.5, 0.9995], theta in [0, pi]), or U[-1, 1] x U[-0.5, 0.5]"""
    rng = np.random.default_rng(3000 * N + 10 * C + seed + 100 * COEFS.index(kind))
    if kind == "reson":
        r, th = rng.uniform(0.5, 0.9995, (N, C)), rng.uniform(0.0, math.pi, (N, C))
        a1, a2 = 2.0 * r * np.cos(th), -(r * r)
    else:
        a1, a2 = rng.uniform(-1.0, 1.0, (N, C)), rng.uniform(-0.5, 0.5, (N, C))
    return np.asfortranarray(a1), np.asfortranarray(a2)


MARKS = tuple(m + k for m in (L - 1, L, T - 1, T, CH - 1, CH, 2 * CH) for k in (0, 1))


def planted(x, kinds=(np.inf, -np.inf, np.nan), zeros=True):
    """a copy of x with +-0 planted at run, tile and chunk boundaries and one frame after each and, per channel, ONE of
    `kinds` at a late mark, so that what lies before it stays finite; with three channels and more, the last one is all -0.0"""
    x = np.array(x, order="F")
    N, C = x.shape
    for c in range(C):
        if zeros:
            for k, at in enumerate(MARKS):
                if at + 1 < N:
                    x[at, c] = (-0.0, 0.0)[(k // 2 + c) % 2]
        late = [m for m in MARKS if m < N]
        if late and kinds:
            x[late[(len(late) - 1 - c) % len(late)], c] = kinds[c % len(kinds)]
    if zeros and C >= 3:
        x[:, C - 1] = -0.0
    return x


# ---- the wrappers' formulas ------------------------------------------------------------------------------------------------
def _fn(*vs):
    """`math` where every argument is a number (what the constructors run on the host), NumPy where one is an array"""
    return math if all(np.ndim(v) == 0 for v in vs) else np


def resonator_coefs(fc, bw, fs):
    """-> (a1, a2, g): `Resonator(x, fc, bw)` is `Recur2(a1, a2, g x)`; fc and bw numbers of Hz or arrays"""
    m = _fn(fc, bw)
    r = m.exp(-math.pi * bw / fs)
    th = 2.0 * math.pi * fc / fs
    return 2.0 * r * m.cos(th), -(r * r), (1.0 - r * r) * m.sin(th)


def sweep_coefs(kind, fc, q, fs):
    """-> (a1, a2, c0, c1, c2): `Sweep(x, kind, fc, q)` is `Recur2(a1, a2, (c0 x[n] + c1 x[n-1]) + c2 x[n-2])`, the
    audio-EQ-cookbook biquad with the coefficients of frame n on all taps; kind "lowpass", "highpass" or "bandpass\""""
    m = _fn(fc, q)
    w = 2.0 * math.pi * fc / fs
    cw = m.cos(w)
    alpha = m.sin(w) / (2.0 * q)
    a0 = 1.0 + alpha
    if kind == "lowpass":
        b0, b1 = (1.0 - cw) / 2.0, 1.0 - cw
        b2 = b0
    elif kind == "highpass":
        b0, b1 = (1.0 + cw) / 2.0, -(1.0 + cw)
        b2 = b0
    else:
        b0, b1, b2 = alpha, 0.0 * alpha, -alpha
    return 2.0 * cw / a0, -(1.0 - alpha) / a0, b0 / a0, b1 / a0, b2 / a0


def delayed(x, k):
    """x delayed by k whole frames, zeros in front, same length (frames x channels)"""
    x = np.asarray(x)
    y = np.zeros_like(x)
    if k < x.shape[0]:
        y[k:] = x[: x.shape[0] - k]
    return y


def sweep_input(x, c0, c1, c2):
    """the b of `Sweep`: (c0 x[n] + c1 x[n-1]) + c2 x[n-2], every operation rounded on its own"""
    x = _planar(x)
    bc = lambda c: c if np.ndim(c) == 0 else _planar(c)  # noqa: E731
    return (bc(c0) * x + bc(c1) * delayed(x, 1)) + bc(c2) * delayed(x, 2)
