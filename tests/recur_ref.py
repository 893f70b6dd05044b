"""The yardstick of `Recur(a, b)`, `OnePole`, `Smooth` and `PeakDecay` (include/sigops.h SO_NODE_RECUR; csrc/k_recur.hip): the
first-order scan y[n] = J(a[n], y[n-1], b[n]), y[0] = b[0], over ONE tree that depends on the frame index only, never on
how many frames are asked for.  Per channel, in Float64 (Float32 widens exactly).  With m = a * v rounded once,

    J(a, v, w)   op 0 (affine):    m + w, rounded once more (never one fused operation)
                 op 1 (max-decay): NaN if m or w is NaN, else m if m >= w, else w

and the constants of `Cumsum` (L = 16, W = 64, T = 1024, G = 16, CH = 16384), an element of the scan is a pair (product of
the a, value):

    run    j of a tile: p = a, r = b at the first frame itself; then p[n] = a[n] p[n-1], r[n] = J(a[n], r[n-1], b[n]);
           the run's totals (A_j, B_j) are its last (p, r)
    tile   an inclusive Kogge-Stone scan over the totals: for d = 1, 2, .. 32 and every j >= d at once,
           (A_j, B_j) <- (A_j A_{j-d}, J(A_j, B_{j-d}, B_j)); q = p, t = r in run 0, q = p A_{j-1}, t = J(p, B_{j-1}, r) in run j >= 1
    chunk  tile 0: u = t, Q = q; tile k >= 1: u = J(q, c, t), Q = q P, with (P, c) the last (Q, u) of the tile before
    signal chunk 0: y = u; chunk k >= 1: y = J(Q, C, u); C = u[last] after chunk 0, J(Q[last], C, u[last]) after each later one

-- in NumPy array operations (`recur_ref`), restated as plain loops over Python floats (`recur_tree_loop`), next to the
sequential loop y[n] = J(a[n], y[n-1], b[n]) (`recur_loop`) that the accuracy tests compare with, and the inputs the
device tests read.  NaN payloads are outside the contract; the sign of zero and the place of +-Inf and NaN are inside it.

Where |a| > 1 over long stretches a product of the a overflows, and the tree can then give Inf * 0 = NaN where the loop
stays finite (a = 2, b = 0: tests/test_recur_host.py pins it).  The operators are meant for |a| <= 1; this file is the
definition there too."""
import math

import numpy as np

from cumsum_ref import CH, G, L, T, W, kernel_constants, same_bits  # noqa: F401  (the tree's constants are Cumsum's)


# ---- J ---------------------------------------------------------------------------------------------------------------------
def join(op, a, v, w):
    """J over arrays (or scalars), every operation rounded on its own"""
    m = np.multiply(a, v)
    if op == 0:
        return np.add(m, w)
    bad = np.isnan(m) | np.isnan(w)
    return np.where(bad, np.nan, np.where(m >= w, m, w))


def join1(op, a, v, w):
    """J over Python floats"""
    m = a * v
    if op == 0:
        return m + w
    if m != m or w != w:
        return math.nan
    return m if m >= w else w


# ---- the definition, in array operations (one channel) -------------------------------------------------------------------
def tile_scan(op, a, b):
    """-> (q, t), tile-local"""
    n = b.size
    nr = -(-n // L)
    p, r = np.ones(nr * L), np.zeros(nr * L)  # (a ragged last run is padded: its totals enter no frame that exists)
    p[:n], r[:n] = a, b
    p, r = p.reshape(nr, L), r.reshape(nr, L)  # a row a run; p holds a until it is overwritten
    for m in range(1, L):
        r[:, m] = join(op, p[:, m], r[:, m - 1], r[:, m])
        p[:, m] = p[:, m] * p[:, m - 1]
    A, B = p[:, L - 1].copy(), r[:, L - 1].copy()
    d = 1
    while d < W:
        if d < nr:
            A0, B0 = A.copy(), B.copy()
            B[d:] = join(op, A0[d:], B0[:-d], B0[d:])
            A[d:] = A0[d:] * A0[:-d]
        d *= 2
    if nr > 1:
        r[1:] = join(op, p[1:], B[:-1, None], r[1:])
        p[1:] = p[1:] * A[:-1, None]
    return p.reshape(-1)[:n], r.reshape(-1)[:n]


def chunk_scan(op, a, b):
    """-> (Q, u), chunk-local"""
    Q, u = np.empty(b.size), np.empty(b.size)
    P = c = None
    for k in range(-(-b.size // T)):
        s = slice(T * k, T * k + T)
        q, t = tile_scan(op, a[s], b[s])
        if c is not None:
            t = join(op, q, c, t)
            q = q * P
        Q[s], u[s] = q, t
        P, c = q[-1], t[-1]
    return Q, u


def recur_1d(op, a, b):
    y = np.empty(b.size)
    C = None
    for k in range(-(-b.size // CH)):
        s = slice(CH * k, CH * k + CH)
        Q, u = chunk_scan(op, a[s], b[s])
        y[s] = u if C is None else join(op, Q, C, u)
        C = u[-1] if C is None else join(op, Q[-1], C, u[-1])
    return y


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


def recur_ref(a, b, op=0):
    """`b` frames x channels (or a vector), `a` a number or an array -> frames x channels Float64, planar"""
    b = _planar(b)
    a = coefficients(a, *b.shape)
    y = np.empty(b.shape, order="F")
    with np.errstate(all="ignore"):
        for c in range(b.shape[1]):
            y[:, c] = recur_1d(op, np.ascontiguousarray(a[:, c]), np.ascontiguousarray(b[:, c]))
    return y


# ---- the same tree, one Python float after the other ----------------------------------------------------------------------
def recur_tree_loop(a, b, op=0):
    """one channel, plain loops over Python floats (IEEE doubles): nothing shared with the block form but the tree"""
    a = [float(v) for v in np.asarray(a, dtype=np.float64)]
    b = [float(v) for v in np.asarray(b, dtype=np.float64)]
    n = len(b)
    y = [0.0] * n
    C = None
    for c0 in range(0, n, CH):
        P = c = None  # the last (Q, u) of the tile before, chunk-local
        Qlast = ulast = None
        for t0 in range(c0, min(c0 + CH, n), T):
            t1 = min(t0 + T, n)
            nr = -(-(t1 - t0) // L)
            p, r = [0.0] * (t1 - t0), [0.0] * (t1 - t0)
            A, B = [0.0] * nr, [0.0] * nr
            for j in range(nr):
                lo = t0 + L * j
                pp, rr = a[lo], b[lo]
                p[lo - t0], r[lo - t0] = pp, rr
                for i in range(lo + 1, min(lo + L, t1)):
                    rr = join1(op, a[i], rr, b[i])
                    pp = a[i] * pp
                    p[i - t0], r[i - t0] = pp, rr
                A[j], B[j] = pp, rr
            d = 1
            while d < W:
                A, B = ([A[j] if j < d else A[j] * A[j - d] for j in range(nr)],
                        [B[j] if j < d else join1(op, A[j], B[j - d], B[j]) for j in range(nr)])
                d *= 2
            for i in range(t0, t1):
                j = (i - t0) // L
                q, t = p[i - t0], r[i - t0]
                if j > 0:
                    t = join1(op, q, B[j - 1], t)
                    q = q * A[j - 1]
                if c is not None:
                    t = join1(op, q, c, t)
                    q = q * P
                y[i] = t if C is None else join1(op, q, C, t)
                Qlast, ulast = q, t
            P, c = Qlast, ulast
        C = ulast if C is None else join1(op, Qlast, C, ulast)
    return np.array(y)


# ---- the sequential recurrence ---------------------------------------------------------------------------------------------
def recur_loop(a, b, op=0):
    """one channel: y[0] = b[0], y[n] = J(a[n], y[n-1], b[n]), one frame after the other"""
    a = [float(v) for v in np.asarray(a, dtype=np.float64)]
    b = [float(v) for v in np.asarray(b, dtype=np.float64)]
    y = [0.0] * len(b)
    for i in range(len(b)):
        y[i] = b[i] if i == 0 else join1(op, a[i], y[i - 1], b[i])
    return np.array(y)


def magnitude_loop(a, b):
    """S[n] = |a[n]| S[n-1] + |b[n]|, S[0] = |b[0]|: what the error bound of op 0 is relative to"""
    return recur_loop(np.abs(a), np.abs(b), 0)


# ---- the inputs of the device tests ----------------------------------------------------------------------------------------
LENGTHS = [1, L - 1, L, L + 1, T - 1, T, T + 1, CH - 1, CH, CH + 1, 2 * CH + 1, 3 * CH + 77]
CHANNELS = [1, 3, 8]
COEFS = ["u01", "u11", "c999", "u099"]


def coef(kind, N, C, seed=0):
    """N x C coefficients: U[0,1], U[-1,1], the constant 0.999 as a row, U[0.99,1]"""
    rng = np.random.default_rng(3000 * N + 10 * C + seed + 100 * COEFS.index(kind))
    if kind == "u01":
        a = rng.uniform(0.0, 1.0, (N, C))
    elif kind == "u11":
        a = rng.uniform(-1.0, 1.0, (N, C))
    elif kind == "c999":
        a = np.full((N, C), 0.999)
    else:
        a = rng.uniform(0.99, 1.0, (N, C))
    return np.asfortranarray(a)


def signal(N, C, dtype=np.float64, seed=0):
    """N frames x C channels of normal samples (planar)"""
    rng = np.random.default_rng(1000 * N + 10 * C + seed)
    return np.asfortranarray(rng.standard_normal((N, C)).astype(dtype))


def wide(N, C, seed=0):
    """magnitudes from 2^-60 to 2^60, both signs: the order of the operations shows in the bits"""
    rng = np.random.default_rng(7000 * N + 10 * C + seed)
    return np.asfortranarray(rng.standard_normal((N, C)) * np.exp2(rng.integers(-60, 61, (N, C)).astype(np.float64)))


MARKS = (L - 1, L, T - 1, T, CH - 1, CH, 2 * CH)


def planted(x, kinds=(np.inf, -np.inf, np.nan), zeros=True):
    """a copy of x with +-0 planted at run, tile and chunk boundaries and, per channel, ONE of `kinds` at a late boundary, so
    that what lies before it stays finite; with three channels and more, the last one is all -0.0"""
    x = np.array(x, order="F")
    N, C = x.shape
    for c in range(C):
        if zeros:
            for k, at in enumerate(MARKS):
                if at + 1 < N:
                    x[at, c] = (-0.0, 0.0)[(k + c) % 2]
        late = [m for m in MARKS if m < N]
        if late and kinds:
            x[late[(len(late) - 1 - c) % len(late)], c] = kinds[c % len(kinds)]
    if zeros and C >= 3:
        x[:, C - 1] = -0.0
    return x
