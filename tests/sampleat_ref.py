"""The yardstick of `SampleAt(x, pos)` (include/sigops.h SO_NODE_SAMPLEAT; csrc/k_sample_at.hip): the two NumPy expressions
that define it, a NumPy restatement of the device's uniform-knot formula (j = floor(p), knot distance exactly 1.0), and the
tables and positions the device tests read -- shared, so that the restatement is held to NumPy on exactly those inputs
(tests/test_sampleat_host.py) and the device to both (tests/test_gpu_sampleat.py)."""
import numpy as np

N_TABLE = [1, 2, 3, 64, 65, 4097]
N_RESULT = [1, 2, 63, 64, 65, 1001]
N_CHANNELS = [1, 2, 3, 8]


# ---- the definition --------------------------------------------------------------------------------------------------
def sampleat_np(x, pos, left=0.0, right=0.0, relative=False, wrap=False, base=0):
    """out[n, c] = np.interp(p, arange(N), float64(x[:, c]), left, right) -- period=N with `wrap` -- at p = pos[n, c or 0],
    n + pos[n, c or 0] with `relative` (n counted from `base`)"""
    x = np.asarray(x)
    x = x.reshape(x.shape[0], -1)
    pos = np.asarray(pos, dtype=np.float64)
    pos = pos.reshape(pos.shape[0], -1)
    N, C = x.shape
    knots = np.arange(N, dtype=np.float64)
    out = np.empty((pos.shape[0], C), order="F")
    n = np.arange(base, base + pos.shape[0], dtype=np.float64)
    with np.errstate(all="ignore"):
        for c in range(C):
            p = pos[:, c if pos.shape[1] > 1 else 0]
            if relative:
                p = n + p
            f = x[:, c].astype(np.float64)
            out[:, c] = np.interp(p, knots, f, period=N) if wrap else np.interp(p, knots, f, left, right)
    return out


# ---- the device's formula, restated ------------------------------------------------------------------------------------
def _column(f, p, left, right, wrap):
    N = f.shape[0]
    with np.errstate(all="ignore"):
        if wrap:
            pm = np.remainder(p, np.float64(N))  # in [0, N], NaN for a NaN or infinite position
            pc = np.minimum(np.where(pm > 0.0, pm, 0.0), np.float64(N))
            j = pc.astype(np.int64)
            j0 = np.where(j >= N, 0, j)
            j1 = np.where(j0 + 1 >= N, 0, j0 + 1)
            q, edge = pm, None
        else:
            if N == 1:
                return np.where(p < 0.0, left, np.where(p > 0.0, right, f[0]))
            top = np.float64(N - 1)
            pc = np.minimum(np.where(p > 0.0, p, 0.0), top)
            j = np.minimum(pc.astype(np.int64), N - 2)
            j0, j1 = j, j + 1
            q, edge = p, top
        f0, f1 = f[j0], f[j1]
        xlo = j.astype(np.float64)
        s = f1 - f0
        r = s * (q - xlo) + f0
        r2 = s * (q - (xlo + 1.0)) + f1
        r2 = np.where(np.isnan(r2) & (f0 == f1), f0, r2)
        r = np.where(np.isnan(r), r2, r)
        r = np.where(q == xlo, f0, r)
        if edge is not None:
            r = np.where(q == edge, f1, r)
            r = np.where(q > edge, right, r)
            r = np.where(q < 0.0, left, r)
        return np.where(np.isnan(q), q, r)


def sampleat_restated(x, pos, left=0.0, right=0.0, relative=False, wrap=False, base=0):
    """what k_sample_at computes, operation for operation: no search, j = floor(p) clamped into the table, the slope
    f1 - f0, NumPy's two fall-backs where slope * distance + f0 is NaN"""
    x = np.asarray(x)
    x = x.reshape(x.shape[0], -1)
    pos = np.asarray(pos, dtype=np.float64)
    pos = pos.reshape(pos.shape[0], -1)
    out = np.empty((pos.shape[0], x.shape[1]), order="F")
    n = np.arange(base, base + pos.shape[0], dtype=np.float64)
    for c in range(x.shape[1]):
        p = pos[:, c if pos.shape[1] > 1 else 0]
        if relative:
            p = n + p
        out[:, c] = _column(x[:, c].astype(np.float64), p, np.float64(left), np.float64(right), wrap)
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
    """a table of N frames x C channels (planar); `nonfinite`: NaN, +-Inf and -0.0 planted so that both of NumPy's slope
    fall-backs are taken: a finite value next to an Inf (first fall-back from the finite side), two equal Infs side by
    side (the second), a NaN (no rescue)"""
    rng = np.random.default_rng(1000 * N + 10 * C + seed)
    x = rng.standard_normal((N, C)).astype(dtype)
    if nonfinite:
        for c in range(C):
            pat = [np.inf, np.inf, 1.5, -np.inf, -0.0, -0.0, np.nan, 2.0, np.inf, -np.inf]
            k = min(N, len(pat))
            at = (3 * c) % max(1, N - k + 1)
            x[at:at + k, c] = np.asarray(pat[:k], dtype=dtype)
    return np.asfortranarray(x)


def positions(N, L, C=1, dtype=np.float64, seed=0):
    """L positions x C channels for a table of N frames: every knot, +-0.0, N-1 and its neighbours, the neighbours of 0,
    -1, N, +-1e300, +-Inf, NaN and midpoints first (as many as fit, a different rotation per channel), random positions
    in [-2, N + 2] behind them"""
    rng = np.random.default_rng(77 * N + 7 * L + C + seed)
    top = float(N - 1)
    special = [0.0, -0.0, top, np.nextafter(0.0, -1.0), np.nextafter(0.0, 1.0), np.nextafter(top, -np.inf), np.nextafter(top, np.inf),
               -1.0, float(N), -1e300, 1e300, np.inf, -np.inf, np.nan, 0.5, top - 0.5, top + 0.5, -0.5]
    knots = list(np.arange(min(N, 80), dtype=np.float64)) + list(np.arange(min(N, 80), dtype=np.float64) + 0.5)
    plant = np.asarray(special + knots, dtype=np.float64)
    out = rng.uniform(-2.0, N + 2.0, size=(L, C))
    for c in range(C):
        rot = np.roll(plant, -5 * c)
        k = min(L, rot.size)
        out[:k, c] = rot[:k]
    with np.errstate(over="ignore"):  # (+-1e300 as Float32 positions: +-Inf)
        return np.asfortranarray(out.astype(dtype))
