"""Expression programs at the interpreter's limits (csrc/planner.cpp legalise / materialise; csrc/kcommon.h run_program):
deeper than kStackDepth = 4, more than kMaxFrameSlots = 4 per-frame values, nested selects, programs that double per
level, odd geometry, and seeded random programs.  Every closure here is built from exact operations only (correctly
rounded, tests/eop_ref.py EXACT_*), so the gate is bit equality with the closure applied to the NumPy arrays -- for any
composition, in Float64 and Float32, through the interpreter (SIGOPS_RTC=0) and hipRTC (SIGOPS_RTC=1).  `-` and `/` are
used throughout: an operand-order slip shows."""
import re

import numpy as np
import pytest

import eop_ref as R
import sigops_amd as so
from test_gpu_elementwise_ops import FS, run

pytestmark = pytest.mark.gpu
DTYPES = [np.float64, np.float32]
SEED = 20240818


def data(rng, n, nch, dt, nans=True):
    """small multiples of 1/2 (comparisons come out both ways, `==` included), some ±0, and NaNs"""
    x = rng.integers(-6, 7, (n, nch)) / 2.0
    x[rng.random((n, nch)) < 0.05] = -0.0
    if nans:
        x[rng.random((n, nch)) < 0.03] = np.nan
    return np.asfortranarray(x.astype(dt))


def smooth(rng, n, nch, dt):
    return np.asfortranarray((rng.standard_normal((n, nch)) * 2).astype(dt))


def want_of(fn, *xs):
    with np.errstate(all="ignore"):
        return np.asarray(fn(*xs))


def check(tree, want, what, steps0=None, rtc=True, dtype=None):
    """the tree through the interpreter and (rtc) hipRTC: bit-equal to `want`; steps0: a predicate on the interpreter's steps"""
    got, names = run(tree, 0, dtype)
    assert set(names) == {"k_pointwise"}, names
    if steps0 is not None:
        assert steps0(names), (what, names)
    R.check_exact(what, got, np.asfortranarray(want))
    if rtc:
        got, names = run(tree, 1, dtype)
        assert names == ["k_pointwise_rtc"], (what, names)
        R.check_exact(what + " (hipRTC)", got, np.asfortranarray(want))


# ---- depth ------------------------------------------------------------------------------------------------------------
def ladder(d):
    """a0 - (a1 / (a2 - (a3 / ...))) over d operands: stack depth d"""
    def f(*a):
        r = a[d - 1]
        for k in range(d - 2, -1, -1):
            r = a[k] - r if k % 2 == 0 else a[k] / r
        return r
    return f


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("d", range(2, 9))
def test_depth_ladder(d, dt):
    rng = np.random.default_rng(SEED + d)
    xs = [smooth(rng, 3000, 2, dt) for _ in range(d)]
    tree = so.OperateOn(so.elementwise(ladder(d)), *[so.Signal(x, FS) for x in xs])
    # beyond kStackDepth the interpreter's plan materialises a sub-expression first (and does not raise "too deep")
    check(tree, want_of(ladder(d), *xs), f"ladder {d}", (lambda s: len(s) > 1) if d > 4 else (lambda s: len(s) == 1))


# ---- select -----------------------------------------------------------------------------------------------------------
SELECTS = [
    lambda a, b, c, d, e, f, g: np.where(np.where(np.where(a < b, c, d) > e, f, g) <= c, a - g, b / f),       # in the condition
    lambda a, b, c, d, e, f, g: np.where(a < b, np.where(c >= d, np.where(e != f, g - a, b / c), d - e), f / g),  # in the true branch
    lambda a, b, c, d, e, f, g: np.where(a > b, c / d, np.where(e == f, g - a, np.where(b <= c, d / e, f - g))),  # in the false branch
    lambda a, b, c, d, e, f, g: np.where(np.where(a >= b, c, d), np.where(e, f - g, g / f), np.where(f < g, a / b, b - a)),  # all three; bare values as conditions
]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("k", range(len(SELECTS)))
def test_select_nests(k, dt):
    rng = np.random.default_rng(SEED + 10 + k)
    xs = [data(rng, 4000, 2, dt) for _ in range(7)]
    tree = so.OperateOn(so.elementwise(SELECTS[k]), *[so.Signal(x, FS) for x in xs])
    check(tree, want_of(SELECTS[k], *xs), f"select nest {k}")


# ---- per-frame slots --------------------------------------------------------------------------------------------------
def timefn(k):
    return lambda t: np.floor(k * t) - t / k


def slot_tree(x, fns, n):
    """((x * f1 + f2) * f3 + f4) ...: a slot taken for another changes the value"""
    r = so.Signal(x, FS)
    for i, f in enumerate(fns):
        s = so.Signal(so.elementwise(f), FS)
        r = so.Amplify(r, s) if i % 2 == 0 else so.Mix(r, s)
    return r | so.Until(n * so.frames)


def slot_want(x, fns, n):
    t = ((np.arange(n, dtype=np.float64) + 1) / 10000.0).reshape(-1, 1)  # frame i (from 1) is at i / fs
    r = x
    for i, f in enumerate(fns):
        r = r * f(t) if i % 2 == 0 else r + f(t)
    return r


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("m", range(1, 7))
def test_frame_slot_ladder(m, dt):
    n = 5000
    x = smooth(np.random.default_rng(SEED + 20 + m), n, 2, dt)
    fns = [timefn(k) for k in range(2, 2 + m)]
    check(slot_tree(x, fns, n), slot_want(x, fns, n), f"{m} time functions")


@pytest.mark.parametrize("dt", DTYPES)
def test_one_time_function_used_twice(dt):
    n = 5000
    x = smooth(np.random.default_rng(SEED + 30), n, 2, dt)
    s = so.Signal(so.elementwise(timefn(3)), FS)
    tree = so.Mix(so.Amplify(so.Signal(x, FS), s), s) | so.Until(n * so.frames)
    check(tree, slot_want(x, [timefn(3), timefn(3)], n), "one time function twice")
    f = so.elementwise(lambda t: (np.floor(3 * t) - t / 3) / (2 - (np.floor(3 * t) - t / 3)))  # ... and inside one closure
    t = ((np.arange(n, dtype=np.float64) + 1) / 10000.0).reshape(-1, 1)
    check(so.Amplify(so.Signal(x, FS), so.Signal(f, FS)) | so.Until(n * so.frames), x * want_of(f.fn, t), "a closure's value twice")


# ---- shared sub-expressions: the tracer emits a tree ------------------------------------------------------------------
def repeated(levels, c=1.5):
    def f(x):
        y = x
        for _ in range(levels):
            y = y * y - c
        return y
    return f


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("levels", [5, 8, 9, 10])
def test_programs_that_double_per_level(levels, dt):
    x = np.asfortranarray(np.random.default_rng(SEED + levels).uniform(-1, 1, (2000, 2)).astype(dt))
    f = so.elementwise(repeated(levels))
    (prog,), _ = f.program([dt])
    assert len(prog[0]) >= 4 * 2 ** levels - 3
    check(so.OperateOn(f, so.Signal(x, FS)), want_of(repeated(levels), x), f"{levels} levels", rtc=levels == 5)  # (hipRTC takes 23 s over the 1021 operations of 8 levels)


def test_a_program_beyond_65536_operations_is_refused_at_plan_creation():
    x = np.zeros((64, 1))
    f = so.elementwise(repeated(15))
    (prog,), _ = f.program([np.float64])
    assert len(prog[0]) > 65536 >= len(so.elementwise(repeated(14)).program([np.float64])[0][0][0])
    with pytest.raises(so.ErrorException, match="longer than 65536 operations"):
        run(so.OperateOn(f, so.Signal(x, FS)), 0)


# ---- geometry ---------------------------------------------------------------------------------------------------------
GEO = [
    lambda a, b, c: a - (b / (c - (a / (b - c)))),                                                              # depth 5
    lambda a, b, c: np.where(a < b, np.where(b >= c, a - c, b / a), np.where(c != a, c / b, a - b)),
    lambda a, b, c: ((a * a - b) * (a * a - b) - c) / (b - a),
]
GEO_FNS = [so.elementwise(f) for f in GEO]  # (one marked object each: one trace, one hipRTC kernel per signature)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("k", range(len(GEO)))
def test_channel_counts_and_lengths(k, dt):
    rng = np.random.default_rng(SEED + 40 + k)
    for nch, n in [(1, 4097), (2, 257), (3, 256), (5, 255), (8, 4097), (1, 1), (2, 1), (3, 2), (8, 2), (5, 257), (2, 256)]:
        xs = [data(rng, n, nch, dt) for _ in range(3)]
        check(so.OperateOn(GEO_FNS[k], *[so.Signal(x, FS) for x in xs]), want_of(GEO[k], *xs), f"closure {k}, {n} x {nch}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("k", range(len(GEO)))
def test_leaves_that_start_at_an_odd_element(k, dt):
    """x[1:], x[3:]: the pair loads' alignment test (run_program, OP_LOAD) -- host arrays and device tensors"""
    import torch

    rng = np.random.default_rng(SEED + 50 + k)
    n = 4100
    for nch in (1, 2):
        full = [data(rng, n, nch, dt) for _ in range(3)]
        for offs in ((1, 0, 3), (3, 1, 1), (0, 1, 2)):
            m = n - 3
            xs = [x[o:o + m] for x, o in zip(full, offs)]
            want = want_of(GEO[k], *xs)
            check(so.OperateOn(GEO_FNS[k], *[so.Signal(x, FS) for x in xs]), want, f"closure {k}, offsets {offs}")
            dev = [torch.from_numpy(np.ascontiguousarray(x.T)).cuda().t()[o:o + m] for x, o in zip(full, offs)]
            check(so.OperateOn(GEO_FNS[k], *[so.Signal(x, FS) for x in dev]), want, f"closure {k}, device, offsets {offs}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("k", range(len(GEO)))
def test_windows_result_types_and_padding(k, dt):
    rng = np.random.default_rng(SEED + 60 + k)
    n = 3001
    xs = [data(rng, n, 2, dt) for _ in range(3)]
    tree = so.OperateOn(GEO_FNS[k], *[so.Signal(x, FS) for x in xs])
    want = want_of(GEO[k], *xs)
    check(tree | so.After(3 * so.frames) | so.Until(1001 * so.frames), want[3:1004], f"closure {k}, After | Until")
    check(tree | so.After(1235 * so.frames) | so.Until(1 * so.frames), want[1235:1236], f"closure {k}, one frame")
    if dt == np.float64:  # a Float32 result requested from a Float64 closure: one rounding at the store
        check(tree, want.astype(np.float32), f"closure {k}, Float32 result", dtype=np.float32)
    # operands of different lengths: the shorter ones are padded with zeros
    cut = [n, n - 7, n - 1000]
    padded = [np.vstack([x[:c], np.zeros((n - c, 2), dtype=dt)]) for x, c in zip(xs, cut)]
    tree = so.OperateOn(GEO_FNS[k], *[so.Signal(np.asfortranarray(x[:c]), FS) for x, c in zip(xs, cut)])
    check(tree, want_of(GEO[k], *padded), f"closure {k}, zero padding")


# ---- seeded random programs -------------------------------------------------------------------------------------------
UN = ["-{0}", "abs({0})", "np.sqrt({0})", "np.square({0})", "np.reciprocal({0})", "np.floor({0})", "np.ceil({0})", "np.trunc({0})",
      "np.rint({0})", "np.sign({0})"]
BIN = ["({0} + {1})", "({0} - {1})", "({0} * {1})", "({0} / {1})", "np.fmod({0}, {1})", "({0} % {1})"]
CMP = ["<", "<=", ">", ">=", "==", "!="]
CONSTS = ["0.5", "-1.25", "3.0", "0.1", "2.0", "-0.75", "np.float32(0.3)", "np.float64(1.7)", "7.0"]
# (minimum / maximum / fmin / fmax against a non-zero constant only: NumPy's answer for the pair (+0, -0) depends on its
#  build; copysign takes its sign from an operand or a constant: a computed NaN's sign differs between processors)
MINMAX = ["np.minimum({0}, {1})", "np.maximum({0}, {1})", "np.fmin({0}, {1})", "np.fmax({1}, {0})"]


def has_operand(e):
    return re.search(r"\ba\d\b", e) is not None


def random_tree(rng, depth, nargs):
    def leaf():
        return f"a{rng.integers(nargs)}" if rng.random() < 0.75 else str(rng.choice(CONSTS))

    def arg():
        return f"a{rng.integers(nargs)}"

    def gen(d):
        if d == 0 or rng.random() < 0.12:
            return leaf()
        r = rng.random()
        if r < 0.22:
            return str(rng.choice(UN)).format(gen(d - 1))
        if r < 0.62:
            a, b = gen(d - 1), gen(rng.integers(d))
            return str(rng.choice(BIN)).format(*((a, b) if rng.random() < 0.5 else (b, a)))
        if r < 0.72:
            return str(rng.choice(MINMAX)).format(gen(d - 1), str(rng.choice(CONSTS[:6])))
        if r < 0.8:
            return f"np.copysign({gen(d - 1)}, {arg() if rng.random() < 0.7 else rng.choice(CONSTS[:6])})"
        lhs = gen(rng.integers(d))
        c = f"({lhs if has_operand(lhs) else arg()} {rng.choice(CMP)} {gen(rng.integers(d))})"  # (a condition of constants alone is no select)
        return f"np.where({c}, {gen(d - 1)}, {gen(rng.integers(d))})"

    for _ in range(100):
        e = gen(depth)
        if has_operand(e):
            return e
    raise AssertionError("no tree with an operand")


NTREES = 200


@pytest.mark.parametrize("block", range(10))
def test_seeded_random_programs(block):
    """200 random trees over the exact operations (arity 1-4, Float32 / Float64 operands, constants, depth <= 7): all of
    them through the interpreter, every tenth through hipRTC as well"""
    for i in range(block * NTREES // 10, (block + 1) * NTREES // 10):
        rng = np.random.default_rng([SEED, i])
        nargs = int(rng.integers(1, 5))
        dts = [np.float32 if rng.random() < 0.5 else np.float64 for _ in range(nargs)]
        xs = [data(rng, 1500, 2, dt, nans=False) if rng.random() < 0.5 else smooth(rng, 1500, 2, dt) for dt in dts]
        while True:
            expr = random_tree(rng, int(rng.integers(2, 8)), nargs)
            fn = eval("lambda " + ", ".join(f"a{k}" for k in range(nargs)) + ": " + expr, {"np": np})  # noqa: S307
            try:
                want = want_of(fn, *xs)
                break
            except ZeroDivisionError:  # Python's own arithmetic on two constants: not a program
                continue
        what = f"seed ({SEED}, {i}): {[np.dtype(d).name for d in dts]} {expr}"
        if want.dtype.kind != "f":
            want = want.astype(np.float64)
        try:
            check(so.OperateOn(so.elementwise(fn), *[so.Signal(x, FS) for x in xs]), want, what, rtc=i % 10 == 0)
        except Exception:
            print("FAILED " + what)
            raise
