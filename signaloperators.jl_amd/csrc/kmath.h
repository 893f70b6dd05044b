// Device implementation of the operations of expression programs (include/sigops.h so_eop_t: SO_UN_*, SO_BIN_*,
// SO_CMP_*, select) -- the traced elementwise closures of `OperateOn(fn, xs...)`, `Signal(fn)` and custom ramp shapes
// (reference src/mapsignal.jl:131-145, src/functions.jl:53-60, src/ramps.jl:60-72).  Used by the interpreter's math
// instantiation (kcommon.h, run_program<..., MATH = true>) and, as TEXT embedded by build.py into rtc_embed.inc, by the
// hipRTC kernels of steps that contain such an operation (rtc.cpp): both call these very functions, so the two paths
// give the same values bit for bit.  Self-contained: no standard headers, no SO_* constants.
//
// Semantics are NumPy's ufuncs on Float64: minimum / maximum propagate NaN, fmin / fmax ignore it, remainder has the
// sign of the divisor (npy_divmod), sign(±0) = +0, rint rounds half to even, a zero result has the sign C99 gives it
// (expm1(-0) = log1p(-0) = -0).  minimum / maximum / fmin / fmax of the pair (+0, -0) return the SECOND operand (NumPy's
// answer there depends on how it was built).  Every value is a Float64 (booleans are 0.0 / 1.0); Float32 closures round
// with an explicit ROUND32 after each operation, so Float32 results overflow to ±Inf and keep their subnormals as
// Float32 arithmetic does.  Checked function by function on the device: tests/test_gpu_elementwise_ops.py.
#pragma once

namespace so {

// (function id, name): the ids are include/sigops.h's so_un_t / so_bin_t / so_cmp_t
#define SO_UN_LIST(X)                                                                                              \
    X(0, neg) X(1, abs) X(2, sqrt) X(3, cbrt) X(4, square) X(5, reciprocal) X(6, exp) X(7, exp2) X(8, expm1)      \
    X(9, log) X(10, log2) X(11, log10) X(12, log1p) X(13, sin) X(14, cos) X(15, tan) X(16, arcsin) X(17, arccos)  \
    X(18, arctan) X(19, sinh) X(20, cosh) X(21, tanh) X(22, arcsinh) X(23, arccosh) X(24, arctanh) X(25, floor)   \
    X(26, ceil) X(27, trunc) X(28, rint) X(29, sign)
#define SO_BIN_LIST(X)                                                                                             \
    X(0, add) X(1, sub) X(2, mul) X(3, div) X(4, pow) X(5, remainder) X(6, fmod) X(7, minimum) X(8, maximum)      \
    X(9, fmin) X(10, fmax) X(11, arctan2) X(12, hypot) X(13, copysign)
#define SO_CMP_LIST(X) X(0, lt) X(1, le) X(2, gt) X(3, ge) X(4, eq) X(5, ne)

#define SO_MF __device__ __forceinline__ double
SO_MF so_m_neg(double x) { return -x; }
SO_MF so_m_abs(double x) { return __builtin_fabs(x); }
SO_MF so_m_sqrt(double x) { return ::sqrt(x); }
SO_MF so_m_cbrt(double x) { return ::cbrt(x); }
SO_MF so_m_square(double x) { return x * x; }
SO_MF so_m_reciprocal(double x) { return 1.0 / x; }
SO_MF so_m_exp(double x) { return ::exp(x); }
SO_MF so_m_exp2(double x) { return ::exp2(x); }
SO_MF so_m_expm1(double x) { return x == 0.0 ? x : ::expm1(x); }  // (the library's expm1(-0) is +0; C99 and NumPy: -0)
SO_MF so_m_log(double x) { return ::log(x); }
SO_MF so_m_log2(double x) { return ::log2(x); }
SO_MF so_m_log10(double x) { return ::log10(x); }
SO_MF so_m_log1p(double x) { return x == 0.0 ? x : ::log1p(x); }  // (as expm1: log1p(-0) = -0)
SO_MF so_m_sin(double x) { return ::sin(x); }
SO_MF so_m_cos(double x) { return ::cos(x); }
SO_MF so_m_tan(double x) { return ::tan(x); }
SO_MF so_m_arcsin(double x) { return ::asin(x); }
SO_MF so_m_arccos(double x) { return ::acos(x); }
SO_MF so_m_arctan(double x) { return ::atan(x); }
SO_MF so_m_sinh(double x) { return ::sinh(x); }
SO_MF so_m_cosh(double x) { return ::cosh(x); }
SO_MF so_m_tanh(double x) { return ::tanh(x); }
SO_MF so_m_arcsinh(double x) { return ::asinh(x); }
SO_MF so_m_arccosh(double x) { return ::acosh(x); }
SO_MF so_m_arctanh(double x) { return ::atanh(x); }
SO_MF so_m_floor(double x) { return ::floor(x); }
SO_MF so_m_ceil(double x) { return ::ceil(x); }
SO_MF so_m_trunc(double x) { return ::trunc(x); }
SO_MF so_m_rint(double x) { return ::rint(x); }
SO_MF so_m_sign(double x) { return x > 0.0 ? 1.0 : x < 0.0 ? -1.0 : x == 0.0 ? 0.0 : x; }

SO_MF so_m_add(double a, double b) { return a + b; }
SO_MF so_m_sub(double a, double b) { return a - b; }
SO_MF so_m_mul(double a, double b) { return a * b; }
SO_MF so_m_div(double a, double b) { return a / b; }
SO_MF so_m_pow(double a, double b) { return ::pow(a, b); }
SO_MF so_m_fmod(double a, double b) { return ::fmod(a, b); }
SO_MF so_m_remainder(double a, double b) {  // npy_divmod's modulus (Python `%` on floats)
    double m = ::fmod(a, b);
    if (b == 0.0) return m;
    if (m != 0.0) {
        if ((b < 0.0) != (m < 0.0)) m = m + b;
    } else m = __builtin_copysign(0.0, b);
    return m;
}
SO_MF so_m_minimum(double a, double b) { return a != a ? a : b != b ? b : (a < b ? a : b); }
SO_MF so_m_maximum(double a, double b) { return a != a ? a : b != b ? b : (a > b ? a : b); }
SO_MF so_m_fmin(double a, double b) { return a != a ? b : b != b ? a : (a < b ? a : b); }
SO_MF so_m_fmax(double a, double b) { return a != a ? b : b != b ? a : (a > b ? a : b); }
SO_MF so_m_arctan2(double a, double b) { return ::atan2(a, b); }
SO_MF so_m_hypot(double a, double b) { return ::hypot(a, b); }
SO_MF so_m_copysign(double a, double b) { return __builtin_copysign(a, b); }

SO_MF so_c_lt(double a, double b) { return a < b ? 1.0 : 0.0; }
SO_MF so_c_le(double a, double b) { return a <= b ? 1.0 : 0.0; }
SO_MF so_c_gt(double a, double b) { return a > b ? 1.0 : 0.0; }
SO_MF so_c_ge(double a, double b) { return a >= b ? 1.0 : 0.0; }
SO_MF so_c_eq(double a, double b) { return a == b ? 1.0 : 0.0; }
SO_MF so_c_ne(double a, double b) { return a != b ? 1.0 : 0.0; }

SO_MF so_select(double c, double a, double b) { return c != 0.0 ? a : b; }

// SO_EOP_INTERP: NumPy's `np.interp(x, xp, fp, left, right)` over a table `t` in device memory, laid out as the C-ABI
// lays it into a node's constants (include/sigops.h): t[0] = n, t[1] = left, t[2] = right, then xp[n] (strictly
// increasing: the planner checks) and fp[n].  The values are NumPy's, operation for operation (arr_interp of
// numpy/_core/src/multiarray/compiled_base.c): a NaN x is returned as it is (a table of ONE knot has no such rule in
// NumPy: there a NaN x is neither left nor right of the knot and gives fp[0]); outside the table left / right; on a knot
// that knot's fp; otherwise slope * (x - xp[j]) + fp[j] with the slope computed per sample, and NumPy's two fall-backs
// where that is NaN (an infinite fp).
// The search returns the one j with xp[j] <= x < xp[j + 1] for ANY strictly increasing xp.  It starts from the linear
// guess (x - xp[0]) * (n - 1) / (xp[n - 1] - xp[0]) -- which only chooses where the search starts: every decision is a
// comparison against xp --, gallops from there in doubling steps until x is bracketed, then bisects.  A uniform table
// costs two reads of xp (the guess is the answer or next to it), any other at most ~2 log2 n.  All table reads are plain
// loads; a table of up to a few megabytes stays in L2.
SO_MF so_interp(const double* __restrict__ t, double x) {
    const int n = (int)t[0];
    const double* __restrict__ xp = t + 3;
    const double* __restrict__ fp = xp + n;
    const double x0 = xp[0];
    if (n == 1) return x < x0 ? t[1] : x > x0 ? t[2] : fp[0];
    if (x != x) return x;
    const double xl = xp[n - 1];
    if (x < x0) return t[1];
    if (x > xl) return t[2];
    if (x == xl) return fp[n - 1];
    // here xp[0] <= x < xp[n - 1]
    const double g = (x - x0) * (double)(n - 1) / (xl - x0);
    int lo = g >= 0.0 && g < (double)(n - 1) ? (int)g : g >= (double)(n - 1) ? n - 2 : 0;  // (a NaN guess: 0)
    int hi;
    double xlo = xp[lo], xhi = xl;
    if (xlo <= x) {  // the answer is at lo or above: gallop up until xp[hi] > x (xp[n - 1] is)
        int step = 1;
        hi = lo + 1;
        while (hi < n - 1) {
            const double v = xp[hi];
            if (v > x) {
                xhi = v;
                break;
            }
            lo = hi;
            xlo = v;
            step += step;
            hi = lo + step < n - 1 ? lo + step : n - 1;
        }
    } else {  // below lo: gallop down until xp[lo] <= x (xp[0] is)
        int step = 1;
        hi = lo;
        xhi = xlo;
        lo = hi - 1;
        for (;;) {
            xlo = xp[lo];
            if (xlo <= x) break;
            hi = lo;
            xhi = xlo;
            step += step;
            lo = hi - step > 0 ? hi - step : 0;
        }
    }
    while (hi - lo > 1) {  // xp[lo] <= x < xp[hi]
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        const double v = xp[mid];
        if (v <= x) {
            lo = mid;
            xlo = v;
        } else {
            hi = mid;
            xhi = v;
        }
    }
    const double f0 = fp[lo];
    if (x == xlo) return f0;
    const double f1 = fp[lo + 1];
    const double s = (f1 - f0) / (xhi - xlo);
    double r = s * (x - xlo) + f0;
    if (r != r) {
        r = s * (x - xhi) + f1;
        if (r != r && f0 == f1) r = f0;
    }
    return r;
}
#undef SO_MF

}  // namespace so
