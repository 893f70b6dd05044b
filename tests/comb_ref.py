"""The yardstick of `Comb(x, d, g)` / `Allpass(x, d, g)` (include/sigops.h SO_NODE_COMB; csrc/k_comb.hip): the definition

    xd = x[n-D] if n >= D else +0.0          yd = y[n-D] if n >= D else +0.0
    y[n] = (b0*x[n] + bD*xd) + a*yd

in NumPy, per channel, every product and every sum rounded on its own in Float64, a term whose coefficient is exactly 0.0
left out -- in blocks of D frames with separately rounded array operations (`comb_ref`), restated as a scalar sequential
loop (`comb_loop`) -- and the inputs the device tests read.  The two forms are held to each other, to closed forms and to
`scipy.signal.lfilter` without a GPU in tests/test_comb_host.py; the device is held to `comb_ref` bit for bit in
tests/test_gpu_comb.py."""
import re
from pathlib import Path

import numpy as np


def unroll():
    """the number of steps whose loads the kernel issues ahead (csrc/kernels.h kCombUnroll)"""
    text = (Path(__file__).resolve().parent.parent / "signaloperators.jl_amd" / "csrc" / "kernels.h").read_text()
    return int(re.search(r"constexpr int kCombUnroll = (\d+);", text).group(1))


def _planar(x):
    x = np.asarray(x)
    return x.reshape(x.shape[0], -1).astype(np.float64)  # (Float32 widens exactly)


# ---- the definition, in blocks of D frames -----------------------------------------------------------------------------
def comb_ref(x, D, b0, bD, a):
    x = _planar(x)
    N, C = x.shape
    D = int(D)
    assert D >= 1
    b0, bD, a = np.float64(b0), np.float64(bD), np.float64(a)
    y = np.empty((N, C), order="F")
    with np.errstate(all="ignore"):
        for c in range(C):
            xp = np.zeros(D)  # x and y before frame 0: +0.0
            yp = np.zeros(D)
            for s in range(0, N, D):
                k = min(D, N - s)
                xb = x[s:s + k, c]
                t = b0 * xb
                if bD != 0.0:
                    t = t + bD * xp[:k]
                if a != 0.0:
                    t = t + a * yp[:k]
                y[s:s + k, c] = t
                xp, yp = xb, t
    return y


def comb(x, D, g, feedforward=0.0, direct=1.0):
    return comb_ref(x, D, direct, feedforward, g)


def allpass(x, D, g):
    return comb_ref(x, D, -g, 1.0, g)


# ---- the same, one frame after the other -------------------------------------------------------------------------------
def comb_loop(x, D, b0, bD, a):
    x = _planar(x)
    N, C = x.shape
    b0, bD, a = np.float64(b0), np.float64(bD), np.float64(a)
    zero = np.float64(0.0)
    y = np.empty((N, C), order="F")
    with np.errstate(all="ignore"):
        for c in range(C):
            for n in range(N):
                xd = x[n - D, c] if n >= D else zero
                yd = y[n - D, c] if n >= D else zero
                t = b0 * x[n, c]
                if bD != 0.0:
                    t = t + bD * xd
                if a != 0.0:
                    t = t + a * yd
                y[n, c] = t
    return y


def same_bits(a, b):
    """equal bit for bit, the sign of zero included; NaNs equal NaNs (their payloads are not compared)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.int64), b[ok].view(np.int64))


# ---- the inputs of the device tests ------------------------------------------------------------------------------------
DELAYS = [1, 2, 63, 64, 65, 255, 256, 257, 513, 1000]
CHANNELS = [1, 3, 8]
# (name, b0, bD, a): the plain comb, the allpass, all three terms, a == 0, both zero, g < 0, g = 1
FORMS = [("comb", 1.0, 0.0, 0.7), ("allpass", -0.6, 1.0, 0.6), ("three terms", 0.9, -0.35, 0.5), ("a == 0", 0.8, 0.45, 0.0),
         ("both zero", -1.25, 0.0, 0.0), ("g < 0", 1.0, 0.0, -0.8), ("g = 1", 1.0, 0.0, 1.0)]


def lengths(D, U):
    """around the first recursion and around the ends of the kernel's unrolled loop (U steps)"""
    ns = [1, D - 1, D, D + 1, 2 * D, 2 * D + 1, U * D - 1, U * D, U * D + 1, (U + 1) * D + 1, (2 * U + 1) * D + 3]
    return sorted({n for n in ns if n >= 1})


def signal(N, C, dtype=np.float64, seed=0):
    """N frames x C channels of normal samples (planar)"""
    rng = np.random.default_rng(1000 * N + 10 * C + seed)
    return np.asfortranarray(rng.standard_normal((N, C)).astype(dtype))


def planted(N, C, D, dtype=np.float64, seed=0):
    """normal samples with +-0, +-Inf and NaN planted: zeros of both signs at the start of a class and later, an Inf exactly
    D frames before a finite sample (what the omitted-term rule exists for: 0 * Inf never arises in a plain comb), a -Inf
    in another class that meets the +Inf's class nowhere, a NaN in a third"""
    x = signal(N, C, dtype, seed + 1)
    for c in range(C):
        at = [(0 + c) % N, (3 + c) % N, (2 * D + 1 + c) % N, (5 * D + 2 + c) % N, (3 * D + 5 + c) % N, (D + 7 + c) % N, (4 * D + 9 + c) % N]
        for i, v in zip(at, (-0.0, 0.0, np.inf, -0.0, -np.inf, np.nan, 0.0)):
            x[i, c] = v
    return x
