"""Every operation of expression programs (csrc/kmath.h: 30 unary functions, 14 binary ones, 6 comparisons, select) on
the device, one by one and element by element, in Float64 and Float32, through the interpreter's math instantiation
(SIGOPS_RTC=0, step k_pointwise) and through hipRTC (SIGOPS_RTC=1, step k_pointwise_rtc), against tests/eop_ref.py: bit
equality with NumPy for the exact operations, an mpmath reference rounded once for the transcendental ones, over grids
of specials, type limits, ties, domain edges, overflow thresholds and huge arguments.  tests/test_eop_reference.py runs
NumPy through the same gates without a device.

One plan evaluates a whole group of operations (a `bychannel=False` closure that returns a tuple: one output channel,
i.e. one piece, per operation; at most 32 pieces go to hipRTC), so the file costs 6 hipRTC compiles.  Run with -s for
the worst error per (operation, type, path) in ulps of the reference (profiles/r08/elementwise_ops_ulp.txt)."""
import contextlib
import functools
import os

import numpy as np
import pytest

import eop_ref as R
import sigops_amd as so
from sigops_amd import _capi as K
from sigops_amd.engine import Plan

pytestmark = pytest.mark.gpu
FS = 10 * so.kHz
DTYPES = [np.float64, np.float32]
GROUPS = {"un": list(K.UN), "bin": list(K.BIN) + ["select"], "cmp": list(K.CMP)}
OPS = [(g, n) for g, names in GROUPS.items() for n in names]
STEP = {0: "k_pointwise", 1: "k_pointwise_rtc"}


@contextlib.contextmanager
def rtc_mode(v):
    old = os.environ.get("SIGOPS_RTC")
    os.environ["SIGOPS_RTC"] = str(v)
    try:
        yield
    finally:
        if old is None:
            del os.environ["SIGOPS_RTC"]
        else:
            os.environ["SIGOPS_RTC"] = old


def run(tree, rtc, dtype=None):
    """(result, step names) of `tree` sunk with SIGOPS_RTC=`rtc`"""
    n = int(so.nframes(tree))
    res = np.zeros((n, tree.nch), dtype=dtype or tree.dtype, order="F")
    with rtc_mode(rtc):
        p = Plan(so.ToChannels(tree, res.shape[1]), res.shape, res.dtype, (1, res.shape[0]), False)
        try:
            p.set_profiling(True)
            p.execute(res.ctypes.data)
            names = [s["name"] for s in p.steps()]
        finally:
            p.close()
    return res, names


def condition(dt):
    """select's first operand: every class of value NumPy's truth test tells apart (±0 false; NaN, Inf, subnormals true)"""
    a, _ = R.grid2(dt)
    c = np.resize(np.asarray([0.0, 1.0, -0.0, np.nan, -2.5, 0.0, np.inf, np.finfo(dt).smallest_subnormal, -0.0, 3.0, 0.0], dtype=dt), a.size)
    return c


def closure(group):
    names = GROUPS[group]
    if group == "un":
        return lambda fr: tuple(R.np_fn(n)(fr[0]) for n in names)
    return lambda fr: tuple(np.where(fr[2], fr[0], fr[1]) if n == "select" else R.np_fn(n)(fr[0], fr[1]) for n in names)


def operands(group, dt):
    if group == "un":
        return np.asfortranarray(R.grid(dt).reshape(-1, 1))
    a, b = R.grid2(dt)
    return np.asfortranarray(np.stack([a, b, condition(dt)], axis=1))


@functools.lru_cache(maxsize=None)
def device(group, dt, rtc):
    tree = so.OperateOn(so.elementwise(closure(group)), so.Signal(operands(group, dt), FS), bychannel=False)
    return run(tree, rtc)


def expected_dtype(group, dt):
    return np.dtype(np.float64) if group == "cmp" else np.dtype(dt)  # (a Boolean result is stored as Float64)


def test_every_operation_is_covered():
    """the parametrisation below is exactly the ids of _capi.UN / BIN / CMP and select: an operation added later
    cannot go untested -- and the groups' closures really trace to those ids"""
    assert {n for g, n in OPS} == set(K.UN) | set(K.BIN) | set(K.CMP) | {"select"}
    assert len(OPS) == 30 + 14 + 6 + 1 == len(K.UN) + len(K.BIN) + len(K.CMP) + 1
    seen = {"un": set(), "bin": set(), "cmp": set(), "select": 0}
    for g in GROUPS:
        progs, _ = so.elementwise(closure(g)).program([np.float64], bychannel=False, nch=[1 if g == "un" else 3])
        assert len(progs) == len(GROUPS[g]) <= 32  # (one piece each; more than 32 pieces do not go to hipRTC)
        for code, _ in progs:
            ops = [(int(o), int(a)) for o, a in code if int(o) in (K.EOP["un"], K.EOP["bin"], K.EOP["cmp"], K.EOP["select"])]
            assert len(ops) == 1, "one operation per output channel"
            (o, a), = ops
            if o == K.EOP["select"]:
                seen["select"] += 1
            else:
                seen[{K.EOP["un"]: "un", K.EOP["bin"]: "bin", K.EOP["cmp"]: "cmp"}[o]].add(a)
    assert seen["un"] == set(K.UN.values()) and seen["bin"] == set(K.BIN.values()) and seen["cmp"] == set(K.CMP.values())
    assert seen["select"] == 1


@pytest.mark.parametrize("rtc", [0, 1])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("group,name", OPS)
def test_operation(group, name, dt, rtc):
    got, names = device(group, dt, rtc)
    assert names == [STEP[rtc]], names  # which path produced the values
    assert got.dtype == expected_dtype(group, dt)
    col = got[:, GROUPS[group].index(name)]
    if name == "select":
        a, b = R.grid2(dt)
        res = R.check_exact(name, col, np.where(condition(dt), a, b), (condition(dt), a, b))
    else:
        res = R.check_on_grid(name, col, dt)
    print(f"device {name:<10} {np.dtype(dt).name} {STEP[rtc]:<15}: worst {res['ulp']:.0f} ulp, {res['excluded']:.2%} of {col.size} excluded")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("group", list(GROUPS))
def test_the_two_paths_agree_bit_for_bit(group, dt):
    a, b = device(group, dt, 0)[0], device(group, dt, 1)[0]
    it = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    same = (a.view(it) == b.view(it)) | (np.isnan(a) & np.isnan(b))
    bad = np.argwhere(~same)
    assert not len(bad), [(GROUPS[group][c], operands(group, dt)[r].tolist(), a[r, c], b[r, c]) for r, c in bad[:6]]


# ---------------------------------------------------------------------------------------------------------------------
# Float32 rules: where "the Float64 function, then one rounding" is not the whole story
def _both(tree):
    a, na = run(tree, 0)
    b, nb = run(tree, 1)
    assert na == ["k_pointwise"] and nb == ["k_pointwise_rtc"], (na, nb)
    assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
    return a


def test_float32_results_beyond_the_range_are_infinite():
    """exp(89) and square(1e20) are finite Float64 values; the ROUND32 behind the operation makes them Inf"""
    x = np.asfortranarray(np.array([[89.0, 1e20, -1e20, 88.0, 1e19]], dtype=np.float32).T)
    got = _both(so.OperateOn(so.elementwise(lambda fr: (np.exp(fr[0]), np.square(fr[0]), np.exp(fr[0]) * 0.5)), so.Signal(x, FS), bychannel=False))
    assert got.dtype == np.float32
    with np.errstate(all="ignore"):
        R.check_close("exp", got[:, 0], *R.ref_unary("exp", x[:, 0], np.float32, edges=True), (x[:, 0],))
        R.check_exact("square", got[:, 1], np.square(x[:, 0]))
        assert got[0, 0] == np.inf and got[1, 1] == got[2, 1] == np.inf               # e^89 = 4.5e38, 1e40: beyond 3.4e38
        assert np.isfinite(got[3, 0]) and np.isfinite(got[4, 1]) and got[3, 0] > 1e38  # e^88, 1e38: just inside
        assert got[0, 2] == np.inf  # (rounded BEFORE the product: e^89 / 2 would fit)


def test_float32_subnormal_results_are_kept():
    """a result in Float32's subnormal range is that subnormal, not zero: x * 1e-30 * 1e-10 in Float32"""
    x = np.asfortranarray(np.array([[1.0, 3.0, -7.5, 1e-3, 1e6, 1e-6]], dtype=np.float32).T)
    fn = lambda v: v * 1e-30 * 1e-10  # noqa: E731
    got = _both(so.OperateOn(so.elementwise(fn), so.Signal(x, FS)))
    want = fn(x)
    assert want.dtype == np.float32 and ((want != 0) & (np.abs(want) < np.finfo(np.float32).tiny)).sum() >= 4
    R.check_exact("mul", got, want)


def test_mixed_operands_round_where_numpy_rounds():
    """(Float32, Float64) operands: the Float32 part of the closure rounds to Float32, the rest does not"""
    rng = np.random.default_rng(21)
    n = 5000
    x = np.asfortranarray(np.abs(rng.standard_normal((n, 1))).astype(np.float32) * 3)
    y = np.asfortranarray(rng.standard_normal((n, 1)))
    sigs = [so.Signal(x, FS), so.Signal(y, FS)]
    # exact operations: bit-equal to the traced program's NumPy evaluation, and to NumPy on the arrays
    fn = lambda a, b: np.sqrt(a) * b - a / 3  # noqa: E731
    f = so.elementwise(fn)
    got = _both(so.OperateOn(f, *sigs))
    (prog,), odt = f.program([np.float32, np.float64])
    assert odt == np.float64 and got.dtype == np.float64
    assert (prog[0][:, 0] == K.EOP["round32"]).sum() == 2  # sqrt(a) and a / 3, not the product or the difference
    R.check_exact("mixed", got[:, 0], R.run_program(prog[0], prog[1], [x[:, 0], y[:, 0]]))
    R.check_exact("mixed", got[:, 0], fn(x[:, 0], y[:, 0]))
    # tanh(x) * y: tanh is rounded to Float32 before the Float64 product -- with y a power of two, got / y IS that Float32
    y2 = np.asfortranarray(rng.choice([0.5, 2.0, -4.0, 0.125, -1.0], (n, 1)))
    fn = lambda a, b: np.tanh(a) * b  # noqa: E731
    got = _both(so.OperateOn(so.elementwise(fn), so.Signal(x, FS), so.Signal(y2, FS)))
    t = got / y2
    assert got.dtype == np.float64 and np.array_equal(t.astype(np.float32).astype(np.float64), t)
    ref, edge = R.ref_unary("tanh", x[:, 0], np.float32, edges=True)
    R.check_close("tanh", t[:, 0].astype(np.float32), ref, edge, (x[:, 0],))
