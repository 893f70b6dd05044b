"""The definition of `SampleAt(x, pos, interp="cubic" | "sinc")` (include/sigops.h SO_NODE_SAMPLEAT, i1 = 1 | 2;
csrc/k_sample_at_fir.hip).  The device is held to this file bit for bit (tests/test_gpu_sampleat_interp.py); the two ways it
is written down here -- NumPy array operations, and loops over Python floats with one operation a line -- are held to each
other without a GPU (tests/test_sampleat_interp_host.py).

Shared by both kinds
    x, pos, the result's length, rate, channels and Float64 type, `relative` (p = float(n) + pos[n], one addition), the
    Float32 widening of either input: as for the linear node (tests/sampleat_ref.py).

    Without `wrap`, top = N - 1:  a NaN p gives NaN, p < 0 gives `left`, p > top gives `right`.  Otherwise j = floor(p),
    t = p - j (exact; a position of -0.0 counts as +0.0, so t is never a negative zero), and the kernel reads x[clamp(j + o, 0, N - 1)] for its offsets o: the table's two ends are
    replicated.  A table of ONE frame follows the linear node's one-knot rule instead: `left` for p < 0, `right` for p > 0,
    x[0] BY VALUE for any other p -- 0.0, -0.0 and NaN (a NaN position is neither left nor right of the knot).

    With `wrap`:  pm = np.remainder(p, N), in [0, N] (N itself where a tiny negative p rounds up to it) or NaN; a NaN pm gives
    NaN; j = floor(pm), t = pm - j, indices (j + o) mod N, a true modulo -- a table shorter than the kernel is gone round
    several times.  `left` and `right` are ignored.

    The device forms j from the position CLAMPED into the table (NaN -> 0), reads, computes, and selects left / right / NaN
    afterwards; the array form below does the same.  What the clamped lanes compute is thrown away, so it is no part of the
    definition.

"cubic": Catmull-Rom over fm = x[j-1], f0 = x[j], f1 = x[j+1], f2 = x[j+2]
    c1 = 0.5 * (f1 - fm)
    c2 = ((fm - 2.5 * f0) + 2.0 * f1) - 0.5 * f2
    c3 = 0.5 * (f2 - fm) + 1.5 * (f0 - f1)
    out = ((c3 * t + c2) * t + c1) * t + f0            every operation rounded on its own, in this order

"sinc": K = taps (even, 4 .. 64), P = 512 phases, the tables of `tap_table(K, cutoff)`: h, (P + 1) x K, and
    dh[ph] = h[ph + 1] - h[ph], P x K, BOTH built on the host and handed to the device as bytes (the device never subtracts
    two rows: for every K it reads h[ph] and dh[ph], from LDS for K <= 16 on large results, from global memory otherwise).
    u = t * 512.0 (exact), ph = floor(u), alpha = u - ph
    tap[k] = h[ph][k] + alpha * dh[ph][k]
    out = the sum over k = 0 .. K-1, left to right, of tap[k] * x[j - K/2 + 1 + k], begun with the first product (no 0 +)

No special cases beyond these: no knot shortcut, no NaN fall-backs.  A non-finite table value poisons every output whose
support holds it (0 * Inf is NaN).  An integer position over finite neighbours returns x[j] by value for "cubic" and for
"sinc" with cutoff == 1 (rows 0 and P are exact impulses) -- except that the sum turns a -0.0 into +0.0.
"""
import numpy as np

P = 512
N_TABLE = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 4097]
N_RESULT = [1, 2, 63, 64, 65, 1001]
N_CHANNELS = [1, 2, 3, 8]
#: (interp, keywords): taps 4, 16 and 64, one even count the kernel's four-tap steps leave two taps over for, both cutoffs
KINDS = [("cubic", {}), ("sinc", {}), ("sinc", {"taps": 4}), ("sinc", {"taps": 64}), ("sinc", {"taps": 10, "cutoff": 0.5}),
         ("sinc", {"taps": 16, "cutoff": 0.5})]


# ---- the host's tap tables -------------------------------------------------------------------------------------------
def beta_for(K):
    """the Kaiser window's shape: 96 dB of attenuation (0.1102 (A - 8.7)) from 16 taps on, 5.0 below"""
    return 0.1102 * (96 - 8.7) if K >= 16 else 5.0


def tap_table(K, cutoff=1.0):
    """(h, dh).  Row ph, tap k lies d = ph/P - (k - K/2 + 1) frames from the position;
    h = cutoff sinc(cutoff d) I0(beta sqrt(1 - (d / (K/2))^2)) / I0(beta), each row divided by its sum; with cutoff == 1
    rows 0 and P are set to the exact unit impulses (at k = K/2 - 1 and at k = K/2)."""
    c = np.float64(cutoff)
    d = np.arange(P + 1, dtype=np.float64)[:, None] / np.float64(P) - (np.arange(K, dtype=np.float64)[None, :] - np.float64(K // 2 - 1))
    w = d / np.float64(K // 2)
    beta = np.float64(beta_for(K))
    h = c * np.sinc(c * d) * (np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - w * w))) / np.i0(beta))
    h = h / h.sum(axis=1)[:, None]
    if c == 1.0:
        h[0] = 0.0
        h[0, K // 2 - 1] = 1.0
        h[P] = 0.0
        h[P, K // 2] = 1.0
    return np.ascontiguousarray(h), np.ascontiguousarray(h[1:] - h[:-1])


_TABLES = {}


def tables(K, cutoff):
    if (K, cutoff) not in _TABLES:
        _TABLES[K, cutoff] = tap_table(K, cutoff)
    return _TABLES[K, cutoff]


# ---- the array form --------------------------------------------------------------------------------------------------
def _column(f, p, left, right, wrap, interp, K, tabs):
    N = f.shape[0]
    with np.errstate(all="ignore"):
        if wrap:
            q = np.remainder(p, np.float64(N))
            pc = np.minimum(np.where(q > 0.0, q, 0.0), np.float64(N))
        else:
            if N == 1:
                return np.where(p < 0.0, left, np.where(p > 0.0, right, f[0]))
            q = p
            top = np.float64(N - 1)
            pc = np.minimum(np.where(p > 0.0, p, 0.0), top)
        j = np.floor(pc).astype(np.int64)
        t = pc - j.astype(np.float64)

        def at(o):
            return f[np.mod(j + o, N)] if wrap else f[np.clip(j + o, 0, N - 1)]

        if interp == "cubic":
            fm, f0, f1, f2 = at(-1), at(0), at(1), at(2)
            c1 = 0.5 * (f1 - fm)
            c2 = ((fm - 2.5 * f0) + 2.0 * f1) - 0.5 * f2
            c3 = 0.5 * (f2 - fm) + 1.5 * (f0 - f1)
            r = ((c3 * t + c2) * t + c1) * t + f0
        else:
            h, dh = tabs
            u = t * 512.0
            ph = np.floor(u).astype(np.int64)
            alpha = u - ph.astype(np.float64)
            r = None
            for k in range(K):
                tap = h[ph, k] + alpha * dh[ph, k]
                term = tap * at(k - (K // 2 - 1))
                r = term if r is None else r + term
        if not wrap:
            r = np.where(q > top, right, r)
            r = np.where(q < 0.0, left, r)
        return np.where(np.isnan(q), q, r)


def sampleat_interp(x, pos, interp, left=0.0, right=0.0, relative=False, wrap=False, taps=16, cutoff=1.0, base=0):
    """the definition, as array operations: out[n, c] for p = pos[n, c or 0] (n + pos with `relative`, n counted from `base`)"""
    assert interp in ("cubic", "sinc")
    x = np.asarray(x)
    x = x.reshape(x.shape[0], -1)
    pos = np.asarray(pos, dtype=np.float64)
    pos = pos.reshape(pos.shape[0], -1)
    out = np.empty((pos.shape[0], x.shape[1]), order="F")
    n = np.arange(base, base + pos.shape[0], dtype=np.float64)
    tabs = tables(taps, cutoff) if interp == "sinc" else None
    for c in range(x.shape[1]):
        p = pos[:, c if pos.shape[1] > 1 else 0]
        if relative:
            p = n + p
        out[:, c] = _column(x[:, c].astype(np.float64), p, np.float64(left), np.float64(right), wrap, interp, taps, tabs)
    return out


# ---- the loop form: Python floats, one operation a line --------------------------------------------------------------
def _one(f, N, p, left, right, wrap, interp, K, h, dh):
    nan = float("nan")
    if wrap:
        if p != p or p in (float("inf"), float("-inf")):
            return nan
        pm = float(np.remainder(np.float64(p), np.float64(N)))
        j = int(np.floor(pm))
        t = pm - float(j)
    else:
        if N == 1:
            return left if p < 0.0 else right if p > 0.0 else f[0]
        if p != p:
            return nan
        if p < 0.0:
            return left
        if p > float(N - 1):
            return right
        p = p if p > 0.0 else 0.0  # (a position of -0.0 is +0.0: t and alpha are never a negative zero)
        j = int(np.floor(p))
        t = p - float(j)

    def at(o):
        i = j + o
        if wrap:
            return f[i % N]
        return f[0 if i < 0 else N - 1 if i > N - 1 else i]

    if interp == "cubic":
        fm = at(-1)
        f0 = at(0)
        f1 = at(1)
        f2 = at(2)
        a = f1 - fm
        c1 = 0.5 * a
        b = 2.5 * f0
        b = fm - b
        e = 2.0 * f1
        b = b + e
        e = 0.5 * f2
        c2 = b - e
        a = f2 - fm
        a = 0.5 * a
        b = f0 - f1
        b = 1.5 * b
        c3 = a + b
        r = c3 * t
        r = r + c2
        r = r * t
        r = r + c1
        r = r * t
        r = r + f0
        return r
    u = t * 512.0
    ph = int(np.floor(u))
    alpha = u - float(ph)
    hr = h[ph]
    dr = dh[ph]
    r = None
    for k in range(K):
        tap = alpha * dr[k]
        tap = hr[k] + tap
        term = tap * at(k - (K // 2 - 1))
        r = term if r is None else r + term
    return r


def sampleat_interp_loops(x, pos, interp, left=0.0, right=0.0, relative=False, wrap=False, taps=16, cutoff=1.0, base=0):
    """the definition again, a frame at a time over Python floats"""
    x = np.asarray(x)
    x = x.reshape(x.shape[0], -1)
    pos = np.asarray(pos, dtype=np.float64)
    pos = pos.reshape(pos.shape[0], -1)
    N, C = x.shape
    out = np.empty((pos.shape[0], C), order="F")
    h, dh = (a.tolist() for a in tables(taps, cutoff)) if interp == "sinc" else (None, None)
    with np.errstate(all="ignore"):
        for c in range(C):
            f = x[:, c].astype(np.float64).tolist()
            col = pos[:, c if pos.shape[1] > 1 else 0].tolist()
            for n, p in enumerate(col):
                if relative:
                    p = float(base + n) + p
                out[n, c] = _one(f, N, p, float(left), float(right), wrap, interp, taps, h, dh)
    return out


def same_bits(a, b):
    """equal bit for bit, the sign of zero included; NaNs equal NaNs (their payloads are not compared)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.int64), b[ok].view(np.int64))


# ---- the inputs of the device tests ----------------------------------------------------------------------------------
def table(N, C, dtype=np.float64, seed=0, nonfinite=False):
    """a table of N frames x C channels (planar); `nonfinite`: +-Inf, NaN and -0.0 planted in the first 24 frames, with runs
    of finite values between them wide enough for a four-point kernel to fit"""
    rng = np.random.default_rng(1000 * N + 10 * C + seed)
    x = rng.standard_normal((N, C)).astype(dtype)
    if nonfinite:
        for c in range(C):
            pat = [-0.0, 1.5, -0.0, -0.0, 2.0, 0.5, np.inf, 1.0, 2.0, 3.0, -1.0, np.nan, 0.25, -0.0, 4.0, 1.0, 2.0, -np.inf, -0.0, 0.0]
            k = min(N, len(pat))
            at = (3 * c) % max(1, N - k + 1)
            x[at:at + k, c] = np.asarray(pat[:k], dtype=dtype)
    return np.asfortranarray(x)


def positions(N, L, C=1, dtype=np.float64, seed=0):
    """L positions x C channels for a table of N frames: integers, `top`, just inside both ends, negative, beyond `top`,
    +-0.0, NaN, +-Inf, +-1e300, the last phase k + 511.999/512, phase boundaries and midpoints first (as many as fit, a
    different rotation per channel), random positions in [-2, N + 2] behind them"""
    rng = np.random.default_rng(77 * N + 7 * L + C + seed)
    top = float(N - 1)
    special = [0.0, -0.0, top, np.nextafter(0.0, -1.0), np.nextafter(0.0, 1.0), np.nextafter(top, -np.inf), np.nextafter(top, np.inf),
               -1.0, float(N), -1e300, 1e300, np.inf, -np.inf, np.nan, 0.5, top - 0.5, top + 0.5, -0.5, 511.999 / 512, top - 1.0 + 511.999 / 512,
               1.0 / 512, 1.0 / 1024, np.nextafter(1.0, 0.0), -1e-20, float(N) - 1e-13]
    kn = np.arange(min(N, 80), dtype=np.float64)
    plant = np.asarray(special + list(kn) + list(kn + 0.5) + list(kn + 511.999 / 512) + list(kn + 37.0 / 512), dtype=np.float64)
    out = rng.uniform(-2.0, N + 2.0, size=(L, C))
    for c in range(C):
        rot = np.roll(plant, -5 * c)
        k = min(L, rot.size)
        out[:k, c] = rot[:k]
    with np.errstate(over="ignore"):  # (+-1e300 as Float32 positions: +-Inf)
        return np.asfortranarray(out.astype(dtype))
