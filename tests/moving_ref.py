"""The yardstick of `MovingMax(x, w)` / `MovingMin(x, w)` (include/sigops.h SO_NODE_MOVING; csrc/k_moving.hip).  Per channel,
with `back >= 0` and `ahead >= 0` whole frames and W = back + ahead + 1:

    y[n] = MAX over { x[k] : max(0, n - back) <= k <= min(N - 1, n + ahead) }

The window is clipped to the signal, never padded.  If any sample of the clipped window is NaN, y[n] is NaN (payload
unspecified); otherwise y[n] is a bit copy of the greatest sample under -Inf < ... < -0.0 < +0.0 < ... < +Inf.  The minimum
is the mirror image (-0.0 beats +0.0, NaN propagates), stated on its own here.  The result has the type of x.

Two forms: `moving_loop`, the scalar loop with plain Python comparisons, and `moving_ref`, an O(N) NumPy form (van Herk /
Gil-Werman over a monotone integer key) for the larger cases.  tests/test_moving_host.py holds the second to the first; the
device is held to `moving_ref` bit for bit in tests/test_gpu_moving.py."""
import math
import re
from pathlib import Path

import numpy as np


def _constant(name):
    text = (Path(__file__).resolve().parent.parent / "signaloperators.jl_amd" / "csrc" / "kernels.h").read_text()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def kernel_constants():
    """(T, H) as the kernel has them (csrc/kernels.h kMovTile, kMovHalo): a workgroup's output frames, and the longest
    window less one that the one-launch form takes"""
    return _constant("kMovTile"), _constant("kMovHalo")


# ---- (a) the definition, one Python float after the other --------------------------------------------------------------
def _beats_max(a, b):
    """does a beat b for the maximum?  (neither is NaN)"""
    if a == 0.0 and b == 0.0:
        return math.copysign(1.0, a) > math.copysign(1.0, b)  # +0.0 beats -0.0
    return a > b


def _beats_min(a, b):
    if a == 0.0 and b == 0.0:
        return math.copysign(1.0, a) < math.copysign(1.0, b)  # -0.0 beats +0.0
    return a < b


def moving_loop(x, back, ahead, is_min=False):
    """one channel (a vector of Float32 or Float64) -> a vector of the same type"""
    x = np.asarray(x)
    assert x.ndim == 1 and x.dtype in (np.float32, np.float64) and back >= 0 and ahead >= 0
    N = x.size
    v = [float(s) for s in x]  # (a Float32 widens exactly, and the order is the same)
    y = np.empty(N, x.dtype)
    beats = _beats_min if is_min else _beats_max
    for n in range(N):
        lo, hi = max(0, n - back), min(N - 1, n + ahead)
        best = lo
        nan = False
        for k in range(lo, hi + 1):
            if v[k] != v[k]:
                nan = True
                break
            if beats(v[k], v[best]):
                best = k
        y[n] = np.nan if nan else x[best]  # a bit copy of the winner
    return y


# ---- (b) O(N): van Herk / Gil-Werman over a monotone integer key ------------------------------------------------------
def _keys(x):
    """the bits as a signed integer that orders like the samples: a non-negative float's bits, INT_MIN - bits - 1 for a
    negative one, INT_MAX for NaN"""
    it = np.int32 if x.dtype == np.float32 else np.int64
    info = np.iinfo(it)
    b = np.ascontiguousarray(x).view(it)
    k = np.where(b >= 0, b, info.min - b - 1)  # (no overflow: b < 0)
    return np.where(np.isnan(x), info.max, k).astype(it)


def _unkeys(k, dtype):
    it = k.dtype
    info = np.iinfo(it)
    b = np.where(k >= 0, k, info.min - k - 1).astype(it)
    y = b.view(dtype).copy()
    y[k == info.max] = np.nan
    return y


def _moving_max_keys(k, back, ahead):
    N = k.size
    it = k.dtype
    lo = np.iinfo(it).min
    back, ahead = min(back, N), min(ahead, N)  # (a longer reach is clipped anyway)
    W = back + ahead + 1
    rows = -(-(N + back + ahead) // W)
    p = np.full(rows * W, lo, it)
    p[back:back + N] = k
    p = p.reshape(rows, W)
    prefix = np.maximum.accumulate(p, axis=1).ravel()
    suffix = np.maximum.accumulate(p[:, ::-1], axis=1)[:, ::-1].ravel()
    n = np.arange(N)
    return np.maximum(suffix[n], prefix[n + W - 1])  # the window of frame n is p[n .. n + W - 1]


def moving_1d(x, back, ahead, is_min=False):
    x = np.asarray(x)
    assert x.ndim == 1 and x.dtype in (np.float32, np.float64) and back >= 0 and ahead >= 0
    if x.size == 0:
        return x.copy()
    if not is_min:
        return _unkeys(_moving_max_keys(_keys(x), back, ahead), x.dtype)
    # the minimum on its own: the least key, with NaN made the least of all
    k = _keys(x)
    info = np.iinfo(k.dtype)
    nan = k == info.max
    # reverse the order (k -> -1 - k is monotone decreasing and cannot overflow), NaN to the top again
    r = np.where(nan, info.max, -1 - np.where(nan, 0, k)).astype(k.dtype)
    m = _moving_max_keys(r, back, ahead)
    out_nan = m == info.max
    kk = (-1 - np.where(out_nan, 0, m)).astype(k.dtype)
    y = _unkeys(kk, x.dtype)
    y[out_nan] = np.nan
    return y


def moving_ref(x, back, ahead, is_min=False):
    """frames x channels (or a vector) -> frames x channels of the same type, planar"""
    x = np.asarray(x)
    x2 = x.reshape(x.shape[0], -1)
    y = np.empty(x2.shape, x2.dtype, order="F")
    for c in range(x2.shape[1]):
        y[:, c] = moving_1d(np.ascontiguousarray(x2[:, c]), back, ahead, is_min)
    return y


def same_bits(a, b):
    """equal bit for bit, the sign of zero included; NaNs equal NaNs (their payloads are not compared)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    it = np.int32 if a.dtype == np.float32 else np.int64
    return np.array_equal(np.ascontiguousarray(a[ok]).view(it), np.ascontiguousarray(b[ok]).view(it))


# ---- the inputs of the tests --------------------------------------------------------------------------------------------
def halves(N, C, dtype=np.float64, seed=0):
    """normal samples rounded to halves: ties are common (planar)"""
    rng = np.random.default_rng(1000 * N + 10 * C + seed)
    return np.asfortranarray((np.round(rng.standard_normal((N, C)) * 2) / 2).astype(dtype))


def tied(N, dtype=np.float64, seed=0):
    """one channel with many ties, zeros of both signs, both infinities and one NaN (where N allows)"""
    rng = np.random.default_rng(77 * N + seed)
    x = rng.integers(-2, 3, N).astype(dtype)
    x[rng.random(N) < 0.2] = -0.0
    if N >= 7:
        x[N // 5] = np.inf
        x[N // 2] = -np.inf
        x[(3 * N) // 4] = np.nan
    return x


def spikes(N, C, T, seed=0):
    """small noise with one spike a block of T frames at a random offset, a different height each: a wrong block index shows"""
    rng = np.random.default_rng(5000 * N + 10 * C + seed)
    x = rng.uniform(-0.25, 0.25, (N, C))
    for c in range(C):
        for b in range(-(-N // T)):
            at = b * T + int(rng.integers(0, min(T, N - b * T)))
            x[at, c] = 10.0 + b + 0.5 * c
    return np.asfortranarray(x)
