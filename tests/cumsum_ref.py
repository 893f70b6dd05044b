"""The yardstick of `Cumsum(x)` (include/sigops.h SO_NODE_CUMSUM; csrc/k_cumsum.hip): ONE summation tree that depends on the
frame index only, never on how many frames are asked for.  Per channel, in Float64 (Float32 widens exactly), with
L = 16, W = 64, T = L W = 1024, G = 16, CH = T G = 16384:

    run    j of a tile: the frames [16 j, 16 j + 16) summed left to right from the first sample itself -> r, total R[j]
    tile   an inclusive Kogge-Stone scan v over R: for d = 1, 2, .. 32, v[j] <- v[j - d] + v[j] for every j >= d at once;
           t = r in run 0, v[j - 1] + r in run j >= 1
    chunk  tile 0 is its t, tile k >= 1 is c + t, c the last value just written
    signal chunk 0 is its chunk-local u, chunk k >= 1 is C + u; C = u[last] after chunk 0, C + u[last] after each later one

every + one rounded Float64 addition -- in NumPy array operations (`cumsum_ref`), restated as plain loops over Python
floats (`cumsum_loop`) -- and the inputs the device tests read.  The two forms are held to each other, to `np.cumsum`
where every order gives the same bits and to `math.fsum` in tests/test_cumsum_host.py; the device is held to
`cumsum_ref` bit for bit in tests/test_gpu_cumsum.py."""
import re
from pathlib import Path

import numpy as np


def _constant(name):
    text = (Path(__file__).resolve().parent.parent / "signaloperators.jl_amd" / "csrc" / "kernels.h").read_text()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


L = 16                # frames of a run
W = 64                # runs of a tile: the lanes of a wave
T = L * W             # frames of a tile
G = 16                # tiles of a chunk
CH = T * G            # frames of a chunk


def kernel_constants():
    """(L, G) as the kernel has them (csrc/kernels.h kCumsumRun, kCumsumTiles): the tests hold them to this file's"""
    return _constant("kCumsumRun"), _constant("kCumsumTiles")


# ---- the definition, in array operations (one channel) -------------------------------------------------------------------
def tile_scan(x):
    n = x.size
    y = np.empty(n)
    nr = -(-n // L)
    R = np.zeros(nr)
    for j in range(nr):
        r = np.add.accumulate(x[L * j:L * j + L])
        y[L * j:L * j + r.size] = r
        R[j] = r[-1]
    v = R.copy()
    d = 1
    while d < W:
        if d < nr:
            v[d:] = v[:-d].copy() + v[d:]
        d *= 2
    for j in range(1, nr):
        y[L * j:L * j + L] = v[j - 1] + y[L * j:L * j + L]
    return y


def chunk_scan(x):
    y = np.empty(x.size)
    c = None
    for k in range(-(-x.size // T)):
        t = tile_scan(x[T * k:T * k + T])
        t = t if c is None else c + t
        y[T * k:T * k + t.size] = t
        c = t[-1]
    return y


def cumsum_1d(x):
    y = np.empty(x.size)
    C = None
    for k in range(-(-x.size // CH)):
        u = chunk_scan(x[CH * k:CH * k + CH])
        y[CH * k:CH * k + u.size] = u if C is None else C + u
        C = u[-1] if C is None else C + u[-1]
    return y


def _planar(x):
    x = np.asarray(x)
    return x.reshape(x.shape[0], -1).astype(np.float64)  # (Float32 widens exactly)


def cumsum_ref(x):
    """frames x channels (or a vector) -> frames x channels Float64, planar"""
    x = _planar(x)
    y = np.empty(x.shape, order="F")
    with np.errstate(all="ignore"):
        for c in range(x.shape[1]):
            y[:, c] = cumsum_1d(np.ascontiguousarray(x[:, c]))
    return y


def integrate_ref(x, fs):
    return np.asfortranarray(cumsum_ref(x) * np.float64(1.0 / fs))


# ---- the same tree, one Python float after the other --------------------------------------------------------------------
def cumsum_loop(x):
    """one channel, plain loops over Python floats (IEEE doubles): nothing shared with the block form but the tree"""
    x = [float(v) for v in np.asarray(x, dtype=np.float64)]
    n = len(x)
    y = [0.0] * n
    C = None
    for c0 in range(0, n, CH):
        c = None  # the last value of the tile before, chunk-local
        ulast = None
        for t0 in range(c0, min(c0 + CH, n), T):
            t1 = min(t0 + T, n)
            nr = -(-(t1 - t0) // L)
            r = [0.0] * (t1 - t0)
            R = [0.0] * nr
            for j in range(nr):
                s = None
                for i in range(t0 + L * j, min(t0 + L * j + L, t1)):
                    s = x[i] if s is None else s + x[i]
                    r[i - t0] = s
                R[j] = s
            v = list(R)
            d = 1
            while d < W:
                v = [v[j] if j < d else v[j - d] + v[j] for j in range(nr)]
                d *= 2
            for i in range(t0, t1):
                j = (i - t0) // L
                t = r[i - t0] if j == 0 else v[j - 1] + r[i - t0]
                u = t if c is None else c + t
                y[i] = u if C is None else C + u
                ulast = u
            c = ulast
        C = ulast if C is None else C + ulast
    return np.array(y)


def same_bits(a, b):
    """equal bit for bit, the sign of zero included; NaNs equal NaNs (their payloads are not compared)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.int64), b[ok].view(np.int64))


# ---- the inputs of the device tests ----------------------------------------------------------------------------------------
# the smallest shapes that cross each level of the tree, with ragged ends at each level; 3 CH + 77 is the only one with
# more than one nonzero chunk carry behind another
LENGTHS = [1, L - 1, L, L + 1, T - 1, T, T + 1, CH - 1, CH, CH + 1, 2 * CH + 1, 3 * CH + 77]
CHANNELS = [1, 3, 8]
BOUNDARIES = sorted({b + o for b in (0, L, 2 * L, T - L, T, T + L, 2 * T, CH - T, CH, CH + L, CH + T, 2 * CH, 3 * CH) for o in (-1, 0, 1) if b + o >= 0})


def signal(N, C, dtype=np.float64, seed=0):
    """N frames x C channels of normal samples (planar)"""
    rng = np.random.default_rng(1000 * N + 10 * C + seed)
    return np.asfortranarray(rng.standard_normal((N, C)).astype(dtype))


def wide(N, C, seed=0):
    """magnitudes from 2^-60 to 2^60, both signs: the order of the additions shows in the bits"""
    rng = np.random.default_rng(7000 * N + 10 * C + seed)
    return np.asfortranarray(rng.standard_normal((N, C)) * np.exp2(rng.integers(-60, 61, (N, C)).astype(np.float64)))


def huge(N, C, seed=0):
    """values near 1e308 of both signs: partial sums overflow to +-Inf (and Inf - Inf to NaN) where the tree says"""
    rng = np.random.default_rng(9000 * N + 10 * C + seed)
    return np.asfortranarray(rng.uniform(-1.0, 1.0, (N, C)) * 1e308)


def planted(N, C, dtype=np.float64, seed=0):
    """normal samples with +-0, +-Inf and NaN planted at run, tile and chunk boundaries (a channel has ONE of +Inf, -Inf or
    NaN late, so that what lies before it stays finite, and zeros of both signs early), and a channel of all -0.0"""
    x = signal(N, C, dtype, seed + 1)
    marks = (L - 1, L, T - 1, T, CH - 1, CH, 2 * CH)
    for c in range(C):
        for k, at in enumerate(marks):
            if at + 1 < N:
                x[at, c] = (-0.0, 0.0)[(k + c) % 2]
        late = [m for m in marks if m < N]
        if late:
            at = late[(len(late) - 1 - c) % len(late)]
            x[at, c] = (np.inf, -np.inf, np.nan)[c % 3]
    if C >= 3:
        x[:, C - 1] = -0.0
    return x
