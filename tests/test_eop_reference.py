"""The reference of the device tests, tested without a device (tests/eop_ref.py): NumPy's own ufuncs go through the very
comparison tests/test_gpu_elementwise_ops.py applies to the device, over the same grids, and pass -- with no more than
1 % of any grid excluded.  Run with -s for NumPy's worst error per function, in ulps of the reference."""
import math

import mpmath
import numpy as np
import pytest

import eop_ref as R
from sigops_amd import _capi as K

DTYPES = [np.float64, np.float32]
ALL = list(K.UN) + list(K.BIN) + list(K.CMP)
WORST = {}


def test_the_classes_partition_the_operations():
    assert sorted(R.EXACT_UN + R.TRANS_UN) == sorted(K.UN)
    assert sorted(R.EXACT_BIN + R.TRANS_BIN) == sorted(K.BIN)
    assert len(R.TRANS_UN) == 20


@pytest.mark.parametrize("dt", DTYPES)
def test_grids_are_fixed_and_hold_what_they_promise(dt):
    fi = np.finfo(dt)
    g = R.grid(dt)
    a, b = R.grid2(dt)
    assert g.dtype == dt and a.dtype == dt and b.dtype == dt and a.shape == b.shape
    assert 300 <= g.size <= 5000 and 300 <= a.size <= 5000
    assert R.grid(dt) is g and not g.flags.writeable
    for v in (0.0, 1.0, -1.0, 0.5, 1.5, 2.5, -2.5, fi.tiny, fi.max, -fi.max, fi.eps, fi.smallest_subnormal, 1 + fi.eps,
              np.nextafter(dt(1), dt(0)), np.nextafter(dt(1), dt(2)), dt(1e22), dt(math.log(float(fi.max)))):
        assert (g == dt(v)).any(), v
    assert np.isnan(g).any() and np.isposinf(g).any() and np.isneginf(g).any()
    assert ((g == 0) & np.signbit(g)).any() and ((g == 0) & ~np.signbit(g)).any()
    assert ((g != 0) & (np.abs(g) < fi.tiny)).any()                      # a subnormal
    assert (np.abs(g[np.isfinite(g)]) > 1e30).any() and ((g != 0) & (np.abs(g) < 1e-30)).any()
    for sa in (False, True):  # all four signed-zero pairs; (Inf, NaN); a negative base with a fractional exponent
        for sb in (False, True):
            assert ((a == 0) & (b == 0) & (np.signbit(a) == sa) & (np.signbit(b) == sb)).any()
    assert (np.isinf(a) & np.isnan(b)).any() and (np.isnan(a) & np.isinf(b)).any()
    assert ((a < 0) & (b == 0.5)).any() and ((a == 0) & (b < 0)).any() and ((a == 1) & np.isnan(b)).any()
    with np.errstate(all="ignore"):
        assert (np.isfinite(a) & np.isfinite(b) & (b != 0) & (np.abs(a / b) > 2.0 ** 53)).any()  # fmod: a huge quotient


def test_one_rounding_to_each_format():
    with mpmath.workprec(R.PREC):
        two = mpmath.mpf(2)
        for dt, p, emin, emax in ((np.float32, 24, -126, 127), (np.float64, 53, -1022, 1023)):
            tiny_sub = two ** (emin - p + 1)
            assert R._round_once(two ** emax * (2 - two ** -p), dt) == (math.inf, True)            # the overflow threshold: a tie, to even
            assert R._round_once(two ** emax * (2 - two ** -p) * (1 - two ** -100), dt) == (float(np.finfo(dt).max), True)
            assert R._round_once(-two ** (emax + 3), dt) == (-math.inf, False)
            assert R._round_once(tiny_sub / 2, dt) == (0.0, True)                                  # a tie, to even
            assert R._round_once(tiny_sub / 2 * (1 + two ** -100), dt) == (float(np.finfo(dt).smallest_subnormal), False)
            v, e = R._round_once(-tiny_sub / 1024, dt)
            assert v == 0.0 and math.copysign(1, v) == -1 and not e
            assert R._round_once(tiny_sub * 5 / 2, dt) == (2 * float(np.finfo(dt).smallest_subnormal), False)  # a subnormal tie
            assert R._round_once(1 + two ** -p, dt) == (1.0, False) and R._round_once(1 + 3 * two ** -p, dt) == (1 + 2.0 ** (2 - p), False)
            assert R._round_once(mpmath.mpf(1) / 3, dt)[0] == float(dt(1) / dt(3))


def test_reference_rules():
    f32, f64 = np.float32, np.float64
    # Float32: one rounding of the exact value of the STORED argument; overflow -> Inf; a subnormal stays a subnormal
    assert R.ref_unary("exp", f32([89.0]), f32)[0] == np.inf and R.ref_unary("exp", f64([89.0]), f64)[0] == math.exp(89.0)
    r = R.ref_unary("exp", f32([-100.0]), f32)
    assert r.dtype == f32 and 0 < r[0] < np.finfo(f32).tiny
    assert R.ref_unary("exp", f64([-1e300, 1e300, -800.0]), f64).tolist() == [0.0, np.inf, 0.0]
    assert R.ref_unary("expm1", f64([-1e300, 1e-300]), f64).tolist() == [-1.0, 1e-300]
    assert R.ref_unary("sin", f64([1e22]), f64)[0] == -0.8522008497671888  # (the classic: Ng, "Argument reduction for huge arguments")
    assert np.signbit(R.ref_unary("sin", f64([-0.0]), f64)[0]) and R.ref_unary("log", f64([1.0]), f64)[0] == 0.0
    # outside the domain / specials: NumPy's class
    assert np.isnan(R.ref_unary("arccosh", f64([0.5]), f64)[0]) and R.ref_unary("arctanh", f64([-1.0]), f64)[0] == -np.inf
    assert R.ref_unary("log1p", f64([-1.0]), f64)[0] == -np.inf and np.isnan(R.ref_unary("log", f64([-2.0]), f64)[0])
    # pow: C99 Annex F
    a = f64([-2.0, -2.0, -2.0, 0.0, -0.0, 1.0, np.nan, -8.0, 2.0, 2.0])
    b = f64([3.0, 2.0, 0.5, -1.0, -3.0, np.nan, 0.0, -1.0, 1024.0, -1080.0])
    r = R.ref_binary("pow", a, b, f64)
    assert r[:2].tolist() == [-8.0, 4.0] and np.isnan(r[2]) and r[3] == np.inf and r[4] == -np.inf
    assert r[5:].tolist() == [1.0, 1.0, -0.125, np.inf, 0.0]
    assert R.ref_binary("hypot", f64([np.inf, 1e200]), f64([np.nan, 1e200]), f64).tolist() == [np.inf, math.hypot(1e200, 1e200)]
    assert R.ref_binary("arctan2", f64([0.0, -0.0]), f64([-0.0, -0.0]), f64).tolist() == [math.pi, -math.pi]
    assert R.ref_binary("lt", f64([1.0, np.nan]), f64([2.0, 2.0]), f64).tolist() == [1.0, 0.0]


def test_the_comparisons_notice_what_they_should():
    f64 = np.float64
    x = np.array([1.0, 0.0, np.nan, np.inf])
    R.check_exact("neg", x.copy(), x)
    for wrong in ([1.0, -0.0, np.nan, np.inf], [np.nextafter(1.0, 2), 0.0, np.nan, np.inf], [1.0, 0.0, 0.0, np.inf]):
        with pytest.raises(AssertionError):
            R.check_exact("neg", f64(wrong), x)
    a, b = f64([0.0, -0.0, 1.0]), f64([-0.0, 0.0, 2.0])
    R.check_exact("minimum", f64([0.0, 0.0, 1.0]), f64([-0.0, -0.0, 1.0]), (a, b))  # (+0, -0): by value
    with pytest.raises(AssertionError):
        R.check_exact("sub", f64([0.0, 0.0, 1.0]), f64([-0.0, -0.0, 1.0]), (a, b))
    ref = f64([1.0, 0.0, np.nan, np.inf, 5e-324 * 7])
    none = np.zeros(5, dtype=bool)
    assert R.check_close("exp", f64([1 + 4e-13, 0.0, np.nan, np.inf, 5e-324 * 8]), ref, none)["ulp"] > 1000
    for wrong in ([1 + 2e-12, 0.0, np.nan, np.inf, 5e-324 * 7], [1.0, -0.0, np.nan, np.inf, 5e-324 * 7], [1.0, 5e-324, np.nan, np.inf, 5e-324 * 7],
                  [1.0, 0.0, np.inf, np.inf, 5e-324 * 7], [1.0, 0.0, np.nan, -np.inf, 5e-324 * 7], [1.0, 0.0, np.nan, 1e308, 5e-324 * 7],
                  [1.0, 0.0, np.nan, np.inf, 5e-324 * 9]):
        with pytest.raises(AssertionError):
            R.check_close("exp", f64(wrong), ref, none)
    edge = np.array([True, False, False, False, False])
    with pytest.raises(AssertionError, match="excluded"):
        R.check_close("exp", ref.copy(), ref, edge)  # 20 % excluded


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", ALL)
def test_numpy_passes_the_device_gate(name, dt):
    args = [R.grid(dt)] if name in K.UN else list(R.grid2(dt))
    with np.errstate(all="ignore"):
        got = np.asarray(R.np_fn(name)(*args))
    if got.dtype == np.bool_:
        got = got.astype(np.float64)
    res = R.check_on_grid(name, got, dt)
    assert res["excluded"] <= R.MAX_EXCLUDED
    WORST[(name, np.dtype(dt).name)] = res
    print(f"numpy {name:<10} {np.dtype(dt).name}: worst {res['ulp']:.3f} ulp, {res['excluded']:.2%} of {got.size} excluded")
