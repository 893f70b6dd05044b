"""The yardstick of `MovingMedian(x, w)` / `MovingQuantile(x, w, q)` (include/sigops.h SO_NODE_MOVRANK; csrc/k_movrank.hip).
Per channel, with `back >= 0` and `ahead >= 0` whole frames, W = back + ahead + 1 and a number q in [0, 1], frame n of a
signal of N frames looks at

    lo = max(0, n - back),  hi = min(N - 1, n + ahead),  m = hi - lo + 1

samples: the window is clipped to the signal, never padded.  Order them -Inf < ... < -0.0 < +0.0 < ... < +Inf (the order of
`moving_ref._keys`: the two zeros are distinct and ordered).  y[n] is a BIT COPY of the sample of rank

    r(m) = floor(q * (m - 1)),   counted from 0,

the product ONE Float64 multiplication and the floor exact.  The result has the sample type of x.  If any sample of the
clipped window is NaN, y[n] is NaN (payload unspecified).  `MovingMedian` is q = 0.5: the middle sample of an odd count, the
LOWER of the two middle samples of an even one -- always a sample of the window, never an average.  q = 0 is `MovingMin`,
q = 1 is `MovingMax`, W = 1 is x itself.  Equal samples have equal bits, so how ties are broken never shows.

Two forms: `movrank_loop`, Python floats and `sorted`, and `movrank_ref`, vectorised (a padded `sliding_window_view` of the
integer keys, `np.sort` along the window, a gather).  tests/test_movingmedian_host.py holds the second to the first; the
device is held to `movrank_ref` bit for bit in tests/test_gpu_movingmedian.py."""
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from moving_ref import _constant, _keys, _unkeys, halves, same_bits, spikes, tied  # noqa: F401  (the shared inputs)


def kernel_constants():
    """(T, H) as the kernel has them (csrc/kernels.h kRankTile, kRankHalo): a workgroup's output frames, and the longest
    window less one that is built"""
    return _constant("kRankTile"), _constant("kRankHalo")


def rank_of(q, m):
    """r(m): one Float64 product, an exact floor"""
    return int(np.floor(np.float64(q) * np.float64(m - 1)))


# ---- (a) the definition, one Python float after the other --------------------------------------------------------------
def _order(v):
    """a sort key for a Python float that is no NaN: by value, and -0.0 before +0.0"""
    return (v, math.copysign(1.0, v))


def movrank_loop(x, back, ahead, q):
    """one channel (a vector of Float32 or Float64) -> a vector of the same type"""
    x = np.asarray(x)
    assert x.ndim == 1 and x.dtype in (np.float32, np.float64) and back >= 0 and ahead >= 0 and 0.0 <= q <= 1.0
    N = x.size
    v = [float(s) for s in x]  # (a Float32 widens exactly, and the order is the same)
    y = np.empty(N, x.dtype)
    for n in range(N):
        lo, hi = max(0, n - back), min(N - 1, n + ahead)
        if any(v[k] != v[k] for k in range(lo, hi + 1)):
            y[n] = np.nan
            continue
        ranked = sorted(range(lo, hi + 1), key=lambda k: _order(v[k]))
        y[n] = x[ranked[rank_of(q, hi - lo + 1)]]  # a bit copy of the sample
    return y


# ---- (b) vectorised: sort every window of the integer keys -----------------------------------------------------------------
def movrank_1d(x, back, ahead, q):
    x = np.asarray(x)
    assert x.ndim == 1 and x.dtype in (np.float32, np.float64) and back >= 0 and ahead >= 0 and 0.0 <= q <= 1.0
    N = x.size
    if N == 0:
        return x.copy()
    back, ahead = min(back, N), min(ahead, N)  # (a longer reach is clipped anyway)
    W = back + ahead + 1
    k = _keys(x)
    info = np.iinfo(k.dtype)
    # the least integer (no sample's key) in front of the signal, the greatest behind it: the front pads rank below every
    # sample of a window and the back pads above, so the sample of rank r is entry r + (front pads) of the sorted window
    p = np.concatenate([np.full(back, info.min, k.dtype), k, np.full(ahead, info.max, k.dtype)])
    rows = np.sort(sliding_window_view(p, W), axis=1)
    n = np.arange(N)
    lo, hi = np.maximum(0, n - back), np.minimum(N - 1, n + ahead)
    r = np.floor(np.float64(q) * (hi - lo).astype(np.float64)).astype(np.int64)  # r(m), m - 1 = hi - lo
    y = _unkeys(rows[n, r + np.maximum(0, back - n)], x.dtype)
    nans = np.concatenate([[0], np.cumsum(np.isnan(x))])
    y[nans[hi + 1] - nans[lo] > 0] = np.nan
    return y


def movrank_ref(x, back, ahead, q):
    """frames x channels (or a vector) -> frames x channels of the same type, planar"""
    x = np.asarray(x)
    x2 = x.reshape(x.shape[0], -1)
    y = np.empty(x2.shape, x2.dtype, order="F")
    for c in range(x2.shape[1]):
        y[:, c] = movrank_1d(np.ascontiguousarray(x2[:, c]), back, ahead, q)
    return y
