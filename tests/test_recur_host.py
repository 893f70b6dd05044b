"""`Recur(a, b)`, `OnePole`, `Smooth` and `PeakDecay` above the C-ABI (signals.py, lowering.py): the NumPy definition the device
is held to (tests/recur_ref.py) checked against its scalar restatement, against itself on every prefix, against
`cumsum_ref` for `a = 1`, and against the sequential loop within derived bounds; length, rate and channel algebra,
currying, the `ToFramerate` rules, every refusal and the lowered node.  No GPU needed."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import _capi as K
from sigops_amd import engine, sharding
from sigops_amd import lowering as LW
from cumsum_ref import cumsum_ref
from recur_ref import (CH, COEFS, G, L, LENGTHS, T, W, coef, kernel_constants, magnitude_loop, planted, recur_1d, recur_loop, recur_ref,
                       recur_tree_loop, same_bits, signal, wide)

FS = 10 * so.kHz
CUTS = [T - 1, T, T + 1, CH - 1, CH, CH + 1, 2 * CH, 2 * CH + 3]
U = 2.0 ** -53


def _x(n=100, c=2, dtype=np.float64, fs=FS):
    return so.Signal(np.asfortranarray(np.arange(n * c, dtype=dtype).reshape(c, n).T), fs)


def _inputs(op, N, seed=0):
    """one channel of coefficients and samples in the range the op is meant for"""
    rng = np.random.default_rng(100 * N + seed + op)
    if op == 0:
        return rng.uniform(-1.0, 1.0, N), rng.standard_normal(N)
    return rng.uniform(0.0, 1.0, N), np.abs(rng.standard_normal(N))


# ---- 1. the reference ------------------------------------------------------------------------------------------------
def test_the_constants_are_the_kernels():
    assert kernel_constants() == (L, G) and (L, W, T, G, CH) == (16, 64, 1024, 16, 16384)
    assert LENGTHS == [1, 15, 16, 17, 1023, 1024, 1025, 16383, 16384, 16385, 2 * 16384 + 1, 3 * 16384 + 77]
    text = (Path(__file__).resolve().parent.parent / "signaloperators.jl_amd" / "csrc" / "k_recur.hip").read_text()
    assert "kRecurWaves = kCumsumTiles" in text and "kCumsumRun" in text  # the kernel takes the tree's constants from kernels.h


@pytest.mark.parametrize("op", [0, 1])
def test_the_block_form_equals_the_scalar_loops_bit_for_bit(op):
    for N in list(range(1, 301)) + CUTS:
        a, b = _inputs(op, N)
        assert same_bits(recur_1d(op, a, b), recur_tree_loop(a, b, op)), (op, N)
    for N in (T + L + 3, 2 * CH + 3):  # wide magnitudes, planted zeros, infinities and NaNs
        a = coef("u11", N, 3)
        b = planted(wide(N, 3))
        with np.errstate(all="ignore"):
            y = recur_ref(a, b, op)
            for c in range(3):
                assert same_bits(y[:, c], recur_tree_loop(a[:, c], b[:, c], op)), (op, N, c)
    b32 = signal(CH + 77, 1, np.float32)
    a32 = coef("u01", CH + 77, 1).astype(np.float32)
    assert same_bits(recur_ref(a32, b32, op)[:, 0], recur_tree_loop(a32[:, 0].astype(np.float64), b32[:, 0].astype(np.float64), op))


@pytest.mark.parametrize("op", [0, 1])
def test_a_prefix_does_not_depend_on_what_follows(op):
    """the tree depends on the frame index only: the scan of a shorter signal is the prefix of a longer one's"""
    N = 2 * CH + 3
    a, b = coef("u11" if op == 0 else "u01", N, 1), wide(N, 1)
    whole = recur_ref(a, b, op)
    for m in [1, L - 1, L, L + 1, 300] + CUTS:
        assert same_bits(recur_ref(a[:m], b[:m], op), whole[:m]), (op, m)


def test_a_coefficient_of_one_is_cumsum_bit_for_bit():
    for N in (1, L + 1, T + 5, CH + T + 3, 3 * CH + 77):
        x = wide(N, 2)  # 2^-60 .. 2^60
        x[min(5, N - 1), 0] = -0.0
        x[:, 1] = np.where(np.arange(N) < min(40, N), -0.0, x[:, 1])  # a run of -0.0 at the start: the sum stays -0.0 there
        with np.errstate(all="ignore"):
            want = cumsum_ref(x)
            assert same_bits(recur_ref(1.0, x), want), N
            assert same_bits(recur_ref(np.ones((N, 1)), x), want), N
        if N > 1:
            assert np.signbit(want[0, 1]) and want[0, 1] == 0


@pytest.mark.parametrize("op", [0, 1])
def test_a_constant_equals_a_row_of_that_constant(op):
    for N in (L + 1, CH + T + 3):
        b = signal(N, 3)
        for a in (0.999, 0.5, -0.75, 0.0, 1.0):
            row = np.full((N, 1), a)
            assert same_bits(recur_ref(a, b, op), recur_ref(row, b, op)), (op, N, a)
            assert same_bits(recur_ref(a, b, op), recur_ref(np.full((N, 3), a), b, op)), (op, N, a)


@pytest.mark.parametrize("kind", COEFS + ["c99999"])
def test_accuracy_of_op_0_against_the_sequential_loop(kind):
    """|tree - loop| <= (gamma(Kt) + gamma(Kl)) S[n], S[n] = |a[n]| S[n-1] + |b[n]|, gamma(K) = K u / (1 - K u), u = 2^-53.
    In exact arithmetic y[n] = sum over k of b[k] times the product of a[k+1 .. n], and both computations form exactly these
    terms, each operation with a relative error of at most u, so a term's relative error is gamma(the rounded operations it
    passes through) (Higham, Accuracy and Stability, lemma 3.1) and the errors sum to that times sum |term| = S[n].
    The loop: term k passes through n - k products and n - k sums: Kl = 2 (N - 1).
    The tree: the product of the n - k coefficients is assembled from disjoint partial products (p, A, q, P, Q) and applied
    to the value one J at a time, which takes n - k multiplications at most however they are grouped; the value passes
    through at most 15 sums in its run, 6 Kogge-Stone steps, 1 to reach the tile's values, 15 tile carries and 1 to apply
    the chunk carry, then one per further chunk: 38 + chunks sums, rounded up to Cumsum's 40 + chunks, and one more product
    per J where the multiplier was itself rounded when it was stored: Kt = (N - 1) + 2 (40 + chunks).
    S is computed by the same loop in floating point: its own error, gamma(2 N) relative, is below 1e-11 and covered by
    the factor 1.0001.  The observed worst ratio |tree - loop| / (u S) is printed: a few units."""
    N = 2 * CH + 1500
    a = np.full(N, 0.99999) if kind == "c99999" else coef(kind, N, 1)[:, 0]
    b = signal(N, 1)[:, 0]
    tree, loop, S = recur_1d(0, a, b), recur_loop(a, b, 0), magnitude_loop(a, b)
    Kt, Kl = (N - 1) + 2 * (40 + -(-N // CH)), 2 * (N - 1)
    bound = (Kt * U / (1 - Kt * U) + Kl * U / (1 - Kl * U)) * 1.0001
    err = np.abs(tree - loop)
    print(f"{kind}: worst |tree - loop| = {np.max(err / (U * S)):.2f} u S (the bound: {Kt + Kl})")
    assert (err <= bound * S).all()


@pytest.mark.parametrize("r", [0.0, 0.5, 0.9995, 0.999999, 1.0, "u01", "u099"])
def test_accuracy_of_op_1_against_the_sequential_loop(r):
    """for r in [0, 1] and x >= 0: y[n] is the greatest of the candidates x[k] times the product of r[k+1 .. n], all >= 0.
    Each candidate is formed with a relative error of gamma(Kt) in the tree and gamma(Kl) in the loop (the counts of
    test_accuracy_of_op_0..., with a comparison, which rounds nothing, where that test has a sum: Kt = (N - 1) + (40 +
    chunks), Kl = N - 1), and max is monotone: the greatest of perturbed candidates lies within the same relative distance
    of the exact maximum.  So |tree - loop| <= (gamma(Kt) + gamma(Kl)) (1 + gamma(Kl)) loop.  Observed: up to about 200 u."""
    N = 2 * CH + 1500
    a = coef(r, N, 1)[:, 0] if isinstance(r, str) else np.full(N, r)
    x = np.abs(signal(N, 1)[:, 0])
    tree, loop = recur_1d(1, a, x), recur_loop(a, x, 1)
    Kt, Kl = (N - 1) + 40 + -(-N // CH), N - 1
    bound = (Kt * U / (1 - Kt * U) + Kl * U / (1 - Kl * U)) * (1 + 2 * Kl * U)
    rel = np.abs(tree - loop) / loop
    print(f"r = {r}: worst |tree - loop| / loop = {np.max(rel) / U:.1f} u (the bound: {Kt + Kl})")
    assert (loop > 0).all() and (rel <= bound).all()
    if r in (0.0, 1.0):  # nothing is rounded: x itself, and the running maximum
        assert same_bits(tree, loop) and same_bits(tree, x if r == 0.0 else np.maximum.accumulate(x))


def test_the_sign_of_zero():
    for N in (1, L + 1, T + 1, CH + T + L + 1):
        neg, pos = np.full((N, 1), -0.0), np.zeros((N, 1))
        # op 0: (+a)(-0) + (-0) = -0 stays; a negative coefficient turns the product to +0 and (+0) + (-0) = +0
        y = recur_ref(0.5, neg)
        assert np.signbit(y).all() and not y.any(), N
        assert not np.signbit(recur_ref(0.5, pos)).any()
        y = recur_ref(-0.5, neg)  # (-a)(-0) = +0, (+0) + (-0) = +0; (-a)(+0) = -0, (-0) + (-0) = -0: the sign alternates
        assert not y.any() and np.array_equal(np.signbit(y[:, 0]), np.arange(N) % 2 == 0), N
        # op 1: m >= w takes the product on a tie, whatever the signs of the zeros
        y = recur_ref(0.5, neg, 1)
        assert np.signbit(y).all() and not y.any()
        y = recur_ref(-0.5, neg, 1)  # the product on a tie: +0, -0, +0, ... again
        assert not y.any() and np.array_equal(np.signbit(y[:, 0]), np.arange(N) % 2 == 0), N
        for op in (0, 1):
            assert same_bits(recur_ref(-0.5, neg, op)[:, 0], recur_loop(np.full(N, -0.5), neg[:, 0], op))
    b = np.full(40, -0.0)
    b[20] = 0.0
    y = recur_ref(1.0, b)[:, 0]
    assert np.signbit(y[:20]).all() and not np.signbit(y[20:]).any()
    y = recur_ref(0.0, np.array([1.0, -0.0, 3.0, -0.0]))[:, 0]  # a = 0 is b itself but for the zero's sign: 0 * y + (-0) = +0
    assert same_bits(y, np.array([1.0, 0.0, 3.0, 0.0]))
    y = recur_ref(0.0, np.array([1.0, -0.0, 3.0, -0.0]), 1)[:, 0]  # max-decay: m = +0 >= -0
    assert same_bits(y, np.array([1.0, 0.0, 3.0, 0.0]))


@pytest.mark.parametrize("op", [0, 1])
def test_infinities_and_nans_appear_where_the_tree_says(op):
    """(a = 0.999: its products stay above the smallest number over these lengths; see the next test for when they do not)"""
    for N, i, j in ((100, 17, 40), (3 * T, T - 1, T), (2 * CH + 5, CH - 1, CH + T + 3), (2 * CH + 5, 3, 2 * CH)):
        a, b = np.full(N, 0.999), np.abs(signal(N, 1)[:, 0]) + 0.1
        b[i] = np.inf
        b[j] = -np.inf
        with np.errstate(all="ignore"):
            y = recur_ref(a, b, op)[:, 0]
        assert np.isfinite(y[:i]).all() and (y[i:j] == np.inf).all(), (op, N, i, j)
        if op == 0:  # Inf + (-Inf)
            assert np.isnan(y[j:]).all()
        else:  # the greater of +Inf and -Inf
            assert (y[j:] == np.inf).all()
    for N, k in ((50, 0), (3 * T, T + L), (CH + 9, CH - 1), (2 * CH + 5, CH + 1)):
        for where in "ab":
            a, b = np.full(N, 0.999), np.abs(signal(N, 1)[:, 0]) + 0.1
            (a if where == "a" else b)[k] = np.nan
            first = N if (where, k) == ("a", 0) else k  # (a[0] multiplies nothing: there is no y[-1])
            with np.errstate(all="ignore"):
                y = recur_ref(a, b, op)[:, 0]
            assert np.isfinite(y[:first]).all() and np.isnan(y[first:]).all(), (op, N, k, where)
    # an infinite coefficient: Inf * y is Inf (y > 0), and Inf * 0 is NaN
    a, b = np.full(64, 0.5), np.ones(64)
    a[20] = np.inf
    with np.errstate(all="ignore"):
        y = recur_ref(a, b, op)[:, 0]
    assert np.isfinite(y[:20]).all() and (y[20:] == np.inf).all()
    # a coefficient of 0 forgets what lies before it, a NaN included only through 0 * NaN = NaN
    a, b = np.full(64, 0.5), np.ones(64)
    b[10] = np.nan
    a[30] = 0.0
    with np.errstate(all="ignore"):
        y = recur_ref(a, b, op)[:, 0]
    assert np.isnan(y[10:]).all()


@pytest.mark.parametrize("op", [0, 1])
def test_an_infinity_becomes_nan_once_the_product_behind_it_underflows(op):
    """the other side of forming the products of the a on their own: 0.5^1075 is 0, so an Inf carried over more frames than
    that meets 0 * Inf = NaN where the loop keeps Inf.  Inside a chunk the carries meet p (at most 16 factors) and q (at
    most 1024, 2^-1024 > 0), so the Inf of frame 3 survives chunk 0; in chunk 1 the carry C meets Q, the product from the
    chunk's first frame on, which is 0 from the chunk's frame 1074 on.  The reference is the definition here too."""
    N = CH + 2 * T
    a, b = np.full(N, 0.5), np.ones(N)
    b[3] = np.inf
    with np.errstate(all="ignore"):
        tree = recur_ref(a, b, op)[:, 0]
    loop = recur_loop(a, b, op)
    assert (loop[3:] == np.inf).all()
    first = CH + 1074
    assert np.isfinite(tree[:3]).all() and (tree[3:first] == np.inf).all() and np.isnan(tree[first:]).all()
    with np.errstate(all="ignore"):
        assert same_bits(tree, recur_tree_loop(a, b, op))


def test_coefficients_above_one_can_overflow_where_a_loop_stays_finite():
    """the documented property: the products of the a are formed on their own, so a = 2 over 1024 frames is Inf, and
    Inf * 0 = NaN at the last frame of the second tile, where the loop's 2 * 0 + 0 stays 0.  The operators are meant for
    |a| <= 1; the reference is the definition here too."""
    N = 3000
    a, b = np.full(N, 2.0), np.zeros(N)
    with np.errstate(all="ignore"):
        tree = recur_ref(a, b)[:, 0]
    loop = recur_loop(a, b)
    assert not loop.any() and not tree[:2 * T - 1].any()
    assert np.isnan(tree[2 * T - 1:]).all()
    assert same_bits(tree, recur_tree_loop(a, b))


# ---- 2. the wrappers against their definitions -------------------------------------------------------------------------
def _fields(y):
    """(a, op, the coefficient signal, b) of a RecurSignal"""
    assert isinstance(y, so.RecurSignal) and y.evaltrait == "computed"
    return y.a, y.op, y.coef, y.signal


def _number(k):
    while isinstance(k, so.MapSignal):  # (`Uniform` spreads the number over the channels of x)
        assert len(k.signals) == 1
        k = k.signals[0]
    assert isinstance(k, so.NumberSig) and k.dtype == np.float64 and not k.dB
    return k.val


def test_onepole_smooth_and_peakdecay_are_their_one_line_definitions():
    x = _x(100, 2, np.float32, fs=44.1 * so.kHz)
    a, op, coef_, b = _fields(so.OnePole(x, 1 * so.kHz))
    want = math.exp(-2.0 * math.pi * 1000.0 / 44_100.0)
    assert (a, op, coef_) == (want, 0, None) and isinstance(b, so.MapSignal) and b.fn == so.signals.MUL
    assert b.signals[0] is x and _number(b.signals[1]) == 1.0 - want
    assert so.OnePole(x, 1000.0).a == want  # a bare number is Hz
    a, op, coef_, b = _fields(so.Smooth(x, 5 * so.ms))
    want = math.exp(-1.0 / (0.005 * 44_100.0))
    assert (a, op, coef_) == (want, 0, None) and b.signals[0] is x and _number(b.signals[1]) == 1.0 - want
    assert so.Smooth(x, 0.005).a == want  # a bare number is seconds
    a, op, coef_, b = _fields(so.Smooth(x, 0))
    assert (a, op) == (0.0, 0) and _number(b.signals[1]) == 1.0  # tau = 0: a = 0, x itself
    a, op, coef_, b = _fields(so.PeakDecay(x, 50 * so.ms))
    assert (a, op, coef_) == (math.exp(-1.0 / (0.05 * 44_100.0)), 1, None) and b is x
    assert so.PeakDecay(x, 0).a == 0.0 and so.PeakDecay(x, r=0.25).a == 0.25 and so.PeakDecay(x, r=1).a == 1.0
    # the values the device is held to
    data = signal(500, 2)
    a = math.exp(-2.0 * math.pi * 100.0 / 10_000.0)
    y = recur_ref(a, np.asfortranarray(data * (1.0 - a)))
    assert abs(y[-1, 0] - recur_loop(np.full(500, a), data[:, 0] * (1.0 - a))[-1]) < 1e-12
    step = recur_ref(a, np.full((2000, 1), 1.0 - a))  # unit gain at DC: the step response tends to 1
    assert abs(step[-1, 0] - 1.0) < 1e-12 and (np.diff(step[:200, 0]) > 0).all() and step.max() < 1.0 + 1e-12
    peak = recur_ref(0.9, np.abs(data), 1)
    assert (peak >= np.abs(data)).all() and np.allclose(peak[:, 0], recur_loop(np.full(500, 0.9), np.abs(data[:, 0]), 1), rtol=1e-13, atol=0)


def test_a_signal_fc_builds_traced_maps():
    x = _x(100, 2, fs=FS)
    fc = so.Signal(np.full((100, 1), 300.0), FS)
    for y, arg in ((so.OnePole(x, fc), 300.0), (so.Smooth(x, so.Signal(np.full((100, 1), 0.01), FS)), 0.01)):
        a, op, coef_, b = _fields(y)
        assert a is None and op == 0 and isinstance(coef_, so.MapSignal) and isinstance(coef_.fn, so.signals.ExprFn) and coef_.nch == 1
        assert so.nframes(b) == 100 and b.nch == 2 and so.nframes(y) == 100 and y.children == (coef_, b)
        want = math.exp(-2.0 * math.pi * arg / 10_000.0) if arg == 300.0 else math.exp(-1.0 / (arg * 10_000.0))
        got = coef_.fn.fn(np.array([arg])) if hasattr(coef_.fn, "fn") else None
        assert got is None or abs(float(np.asarray(got).ravel()[0]) - want) < 1e-15
    inf = so.Signal(np.sin, FS, ω=2 * so.Hz)  # an infinite control signal: the node keeps the length of x
    y = so.OnePole(x, so.OperateOn(so.elementwise(lambda v: 500.0 + 100.0 * v), inf))
    assert so.nframes(y) == 100 and so.signals.isknowninf(so.nframes(y.coef))


# ---- 3. algebra ------------------------------------------------------------------------------------------------------
def test_length_rate_channels_and_type():
    b = _x(100, 3, np.float32, fs=44.1 * so.kHz)
    y = so.Recur(0.5, b)
    assert isinstance(y, so.RecurSignal) and y.signal is b and y.children == (b,) and (y.a, y.op, y.coef) == (0.5, 0, None)
    assert so.nframes(y) == 100 and so.nchannels(y) == 3 and so.framerate(y) == 44_100.0
    assert so.sampletype(y) == np.float64 and so.duration(y) == 100 / 44_100.0
    a1 = so.Signal(np.full((150, 1), 0.5, dtype=np.float32), 44.1 * so.kHz)  # one channel, longer than b
    y = so.Recur(a1, b)
    assert y.coef is a1 and y.a is None and y.children == (a1, b) and so.nframes(y) == 100 and y.nch == 3
    a3 = so.Signal(np.full((100, 3), 0.5), 44.1 * so.kHz)
    assert so.Recur(a3, b).coef is a3
    ainf = so.Signal(np.sin, 44.1 * so.kHz, ω=5 * so.Hz)  # infinite
    assert so.nframes(so.Recur(ainf, b)) == 100
    assert so.Recur(so.Signal(np.full((100, 1), 0.5)), b).coef.fs == 44_100.0  # a without a rate takes b's
    assert so.Recur(a1, _x(100, 3, fs=None)).signal.fs == 44_100.0  # b without a rate takes a's
    assert so.Recur(0.5, _x(fs=None)).fs is None
    assert so.nframes(so.Recur(0.5, b | so.Filt(so.Lowpass, 1 * so.kHz))) == 100  # a computed child


def test_currying_and_piping():
    x = _x()
    y = x | so.Recur(0.5)
    assert isinstance(y, so.RecurSignal) and y.signal is x and y.a == 0.5
    z = np.zeros((100, 2)) | so.Recur(0.5)  # a bare array on the left
    assert isinstance(z, so.RecurSignal) and z.nch == 2
    assert so.nframes(so.pipe(x, so.Recur(0.5), so.Recur(0.25), so.Until(10 * so.frames))) == 10
    for made in (x | so.OnePole(1 * so.kHz), x | so.Smooth(1 * so.ms), x | so.PeakDecay(1 * so.ms), x | so.PeakDecay(r=0.5)):
        assert isinstance(made, so.RecurSignal) and so.nframes(made) == 100 and made.nch == 2
    assert (x | so.PeakDecay(1 * so.ms)).op == 1 and (x | so.PeakDecay(r=0.5)).signal is x
    assert (x | so.OnePole(1 * so.kHz)).a == so.OnePole(x, 1 * so.kHz).a


def test_toframerate():
    y = so.Recur(so.Signal(np.full((100, 1), 0.5)), _x(fs=None))  # no rate: it is handed to both inputs
    z = so.ToFramerate(y, 8 * so.kHz)
    assert isinstance(z, so.RecurSignal) and z.fs == 8000.0 and z.signal.fs == 8000.0 and z.coef.fs == 8000.0 and so.nframes(z) == 100
    z = so.ToFramerate(so.PeakDecay(_x(fs=None), r=0.5), 8 * so.kHz)
    assert isinstance(z, so.RecurSignal) and (z.a, z.op, z.fs, z.signal.fs) == (0.5, 1, 8000.0, 8000.0)
    y = so.Recur(0.5, _x())  # a rate: resampled like any computed signal
    z = so.ToFramerate(y, 20 * so.kHz)
    assert isinstance(z, so.FilteredSignal) and isinstance(z.fn, so.ResamplerFn) and z.signal is y
    assert z.fs == 20_000.0 and so.nframes(z) == 200
    assert so.ToFramerate(y, FS) is y


# ---- 4. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_name_the_construct():
    x = _x()
    sine = so.Signal(np.sin, FS, ω=5 * so.Hz)
    short = so.Signal(np.full((50, 1), 0.5), FS)
    cases = [
        (lambda: so.Recur(0.5, sine), "Recur", "use `Until`"),
        (lambda: sine | so.Recur(0.5), "Recur", "use `Until`"),
        (lambda: so.Recur(0.5, so.Signal(np.zeros(10)) | so.Filt(so.Lowpass, 1 * so.kHz)), "Recur", "use `Until`"),  # unknown: no rate
        (lambda: so.OnePole(sine, 1 * so.kHz), "OnePole", "use `Until`"),
        (lambda: so.OnePole(sine, so.Signal(np.full((100, 1), 300.0), FS)), "OnePole", "use `Until`"),
        (lambda: so.Smooth(sine, 1 * so.ms), "Smooth", "use `Until`"),
        (lambda: so.PeakDecay(sine, 1 * so.ms), "PeakDecay", "use `Until`"),
        (lambda: so.Recur(0.5, so.Signal(np.arange(10), FS)), "Recur", "Float32 or Float64"),
        (lambda: so.Recur(so.Signal(np.arange(100), FS), x), "Recur", "Float32 or Float64"),
        (lambda: so.OnePole(so.Signal(np.arange(10), FS), 1 * so.kHz), "OnePole", "Float32 or Float64"),
        (lambda: so.Smooth(so.Signal(np.arange(10), FS), 1 * so.ms), "Smooth", "Float32 or Float64"),
        (lambda: so.PeakDecay(so.Signal(np.arange(10), FS), 1 * so.ms), "PeakDecay", "Float32 or Float64"),
        (lambda: so.Recur(short, x), "Recur", "at least as long as b"),
        (lambda: so.PeakDecay(x, r=short), "PeakDecay", "at least as long as b"),
        (lambda: so.OnePole(x, so.Signal(np.full((50, 1), 300.0), FS)), "OnePole", "at least as long as b"),
        (lambda: so.Recur(so.Signal(np.full((100, 3), 0.5), FS), x), "Recur", "3 channels; 1 or b's 2"),
        (lambda: so.Recur(so.Signal(np.full((100, 1), 0.5), 8 * so.kHz), x), "Recur", "use `ToFramerate`"),
        (lambda: so.OnePole(x, so.Signal(np.full((100, 1), 300.0), 8 * so.kHz)), "OnePole", "use `ToFramerate`"),
        (lambda: so.Recur(math.inf, x), "Recur", "finite number"),
        (lambda: so.Recur(math.nan, x), "Recur", "finite number"),
        (lambda: so.Recur("half", x), "Recur", "a number or a signal"),
        (lambda: so.OnePole(_x(fs=None), 1 * so.kHz), "OnePole", "needs the frame rate of x"),
        (lambda: so.OnePole(_x(fs=None), so.Signal(np.full((100, 1), 300.0))), "OnePole", "needs the frame rate of x"),
        (lambda: so.Smooth(_x(fs=None), 1 * so.ms), "Smooth", "needs the frame rate of x"),
        (lambda: so.PeakDecay(_x(fs=None), 1 * so.ms), "PeakDecay", "needs the frame rate of x"),
        (lambda: so.OnePole(x, -1 * so.Hz), "OnePole", ">= 0"),
        (lambda: so.OnePole(x, math.inf), "OnePole", ">= 0"),
        (lambda: so.OnePole(x, 1 * so.ms), "OnePole", "not a frequency"),
        (lambda: so.Smooth(x, -1 * so.ms), "Smooth", ">= 0"),
        (lambda: so.Smooth(x, 5 * so.Hz), "Smooth", "not a time"),
        (lambda: so.PeakDecay(x, -1 * so.ms), "PeakDecay", ">= 0"),
        (lambda: so.PeakDecay(x, r=1.5), "PeakDecay", "[0, 1]"),
        (lambda: so.PeakDecay(x, r=-0.1), "PeakDecay", "[0, 1]"),
        (lambda: so.PeakDecay(x, r=math.nan), "PeakDecay", "[0, 1]"),
        (lambda: so.PeakDecay(x, 1 * so.ms, r=0.5), "PeakDecay", "one of them"),
        (lambda: so.PeakDecay(x, short), "PeakDecay", "`r=`"),
        (lambda: engine._streamable(so.Recur(0.5, x) | so.Filt(so.Lowpass, 1 * so.kHz)), "BlockStream: Recur", "not streamable"),
        (lambda: engine._streamable(so.Mix(so.PeakDecay(x, r=0.5), 1.0)), "BlockStream: Recur", "not streamable"),
        (lambda: sharding.shard_time(so.Recur(0.5, x), 0, 2), "Recur", "Recur / OnePole / Smooth / PeakDecay over several GPUs is not built"),
        (lambda: sharding.shard_channels(so.Mix(so.Smooth(x, 1 * so.ms), 1.0), 0, 2), "Recur", "over several GPUs is not built"),
        (lambda: sharding.shard_append(so.Append(so.OnePole(x, 1 * so.kHz), x), 0, 2), "Recur", "over several GPUs is not built"),
    ]
    for make, name, words in cases:
        with pytest.raises(so.ErrorException) as e:
            make()
        assert name in str(e.value) and "Recur" in str(e.value) and words in str(e.value), str(e.value)
    assert (so.Recur, "Recur / OnePole / Smooth / PeakDecay") not in sharding._FROM_FRAME_0
    assert (so.RecurSignal, "Recur / OnePole / Smooth / PeakDecay") in sharding._FROM_FRAME_0


# ---- 5. the lowered node ---------------------------------------------------------------------------------------------
def test_the_lowered_node_in_both_forms():
    assert K.NODE_RECUR == 17 and K.NODE_MOVSUM == 16
    text = (Path(__file__).resolve().parent.parent / "include" / "sigops.h").read_text()
    assert re.search(r"SO_NODE_RECUR = 17\b", text) and re.search(r"SO_NODE_MOVSUM = 16,", text)
    assert re.search(r"\*  RECUR +one child: child 0 = b, d0 = the constant a", text)
    b = _x(100, 2, np.float32)
    for op, tree in ((0, so.Recur(0.75, b)), (1, so.PeakDecay(b, r=0.75))):
        lw = LW.lower(tree)
        nd = lw.nodes[lw.root]
        assert nd.kind == K.NODE_RECUR and nd.n_children == 1 and nd.nch == 2 and nd.dtype == K.SO_F64 and nd.nframes == 100 and nd.fs == 10_000.0
        cb = lw.nodes[nd.children[0]]
        assert cb.kind == K.NODE_ARRAY and cb.l0 == 100 and cb.dtype == K.SO_F32 and cb.nch == 2
        assert (nd.i0, nd.d0) == (op, 0.75)
        assert (nd.i1, nd.i2, nd.i3, nd.l0, nd.l1, nd.s0, nd.s1, nd.d1, nd.d2, nd.d3) == (0,) * 10 and not nd.p0 and not nd.p1
    a = so.Signal(np.full((150, 1), 0.5), FS)
    for op, tree in ((0, so.Recur(a, b)), (1, so.PeakDecay(b, r=a))):
        lw = LW.lower(tree)
        nd = lw.nodes[lw.root]
        assert nd.kind == K.NODE_RECUR and nd.n_children == 2 and nd.nch == 2 and nd.dtype == K.SO_F64 and nd.nframes == 100
        ca, cb = lw.nodes[nd.children[0]], lw.nodes[nd.children[1]]
        assert ca.kind == K.NODE_ARRAY and ca.l0 == 150 and ca.dtype == K.SO_F64 and ca.nch == 1
        assert cb.kind == K.NODE_ARRAY and cb.l0 == 100 and cb.dtype == K.SO_F32 and cb.nch == 2
        assert (nd.i0, nd.d0) == (op, 0.0)


def test_demand_sizes_both_children_from_frame_0():
    a, b = so.Signal(np.full((150, 1), 0.5), FS), _x(100, 2)
    tree = so.Recur(a, b)
    need = {}
    LW._demand(tree | so.Until(10 * so.frames), 10, need)
    assert need[id(a)] == (10, 0) and need[id(b)] == (10, 0)
    need = {}
    LW._demand(tree | so.After(5 * so.frames) | so.Until(10 * so.frames), 10, need)
    assert need[id(a)] == (15, 0) and need[id(b)] == (15, 0)  # the skipped frames are computed too: the skip is not handed on
    need = {}
    LW._demand(so.Recur(0.5, b) | so.After(5 * so.frames), 95, need)
    assert need[id(b)] == (100, 0)
