"""Reference side of the expression-program tests (include/sigops.h so_eop_t; csrc/kmath.h):

  * `run_program`: a NumPy evaluator of the so_eop_t format (what the tracer's programs mean);
  * `ref_unary` / `ref_binary`: the value every operation must have.  Exact operations (`EXACT_*`) are NumPy's own
    result, to be met bit for bit.  For the transcendental ones (`TRANS_*`) a finite, non-zero argument inside the
    function's domain is evaluated by mpmath at 200 bits on the STORED value (Float32 / Float64 widened exactly) and
    rounded ONCE to the type -- overflow gives ±Inf, underflow a subnormal or a signed zero; everything else (NaN, ±Inf,
    ±0, arguments outside the domain, C99 Annex F cases of pow / arctan2 / hypot) has NumPy's class and sign;
  * `grid` / `grid2`: the fixed, seeded inputs -- specials, type limits, ties, domain edges, overflow / underflow
    thresholds of both types, large trigonometric arguments, magnitudes over ±40 decades, and the pairs binary
    functions go wrong on;
  * `check_exact` / `check_close`: the two comparisons.  tests/test_eop_reference.py runs NumPy itself through them (the
    reference and the comparison are tested without a device); tests/test_gpu_elementwise_ops.py runs the device.
"""
import functools
import math

import mpmath
import numpy as np

from sigops_amd import _capi as K

UN_NAMES = {v: k for k, v in K.UN.items()}
BIN_NAMES = {v: k for k, v in K.BIN.items()}
CMP_NAMES = {v: k for k, v in K.CMP.items()}
NP_UN = {"neg": np.negative, "abs": np.absolute, "square": np.square, "reciprocal": np.reciprocal}
NP_BIN = {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.true_divide, "pow": np.power}
NP_CMP = {"lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal, "eq": np.equal,
          "ne": np.not_equal}

EXACT_UN = ["neg", "abs", "sqrt", "square", "reciprocal", "floor", "ceil", "trunc", "rint", "sign"]
EXACT_BIN = ["add", "sub", "mul", "div", "fmod", "remainder", "fmin", "fmax", "minimum", "maximum", "copysign"]
TRANS_UN = ["cbrt", "exp", "exp2", "expm1", "log", "log2", "log10", "log1p", "sin", "cos", "tan", "arcsin", "arccos",
            "arctan", "sinh", "cosh", "tanh", "arcsinh", "arccosh", "arctanh"]
TRANS_BIN = ["pow", "arctan2", "hypot"]
MINMAX = ("minimum", "maximum", "fmin", "fmax")
TOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 1e-6}  # the project's parity contract (README "Parity")
MAX_EXCLUDED = 0.01
PREC = 200  # bits


def np_fn(name):
    """the NumPy ufunc of an operation name of _capi.UN / BIN / CMP"""
    for table in (NP_UN, NP_BIN, NP_CMP):
        if name in table:
            return table[name]
    return getattr(np, name)


def run_program(code, consts, args):
    """a NumPy evaluator of the so_eop_t format: every value Float64; an operation followed by ROUND32 is applied in
    Float32 (what the recorded type says), then widened"""
    st = []
    code = [tuple(int(v) for v in row) for row in code]
    for i, (op, arg) in enumerate(code):
        f32 = i + 1 < len(code) and code[i + 1][0] == K.EOP["round32"]
        cast = (lambda v: np.asarray(v, dtype=np.float32)) if f32 else (lambda v: v)
        with np.errstate(all="ignore"):
            if op == K.EOP["arg"]:
                st.append(np.asarray(args[arg], dtype=np.float64))
            elif op == K.EOP["const"]:
                st.append(np.full(len(args[0]), consts[arg]))
            elif op == K.EOP["un"]:
                n = UN_NAMES[arg]
                st[-1] = np.asarray(NP_UN.get(n, getattr(np, n, None))(cast(st[-1])), dtype=np.float64)
            elif op in (K.EOP["bin"], K.EOP["cmp"]):
                b = st.pop()
                a = st.pop()
                fn = NP_CMP[CMP_NAMES[arg]] if op == K.EOP["cmp"] else NP_BIN.get(BIN_NAMES[arg], getattr(np, BIN_NAMES[arg], None))
                st.append(np.asarray(fn(cast(a), cast(b)), dtype=np.float64))
            elif op == K.EOP["select"]:
                b = st.pop()
                a = st.pop()
                c = st.pop()
                st.append(np.where(c != 0, a, b))
            elif op == K.EOP["round32"]:
                st[-1] = st[-1].astype(np.float32).astype(np.float64)
            else:
                raise AssertionError(f"unknown code {op}")
    assert len(st) == 1
    return st[0]


# ---------------------------------------------------------------------------------------------------------------------
# one rounding of an exact (200-bit) value to a binary format
_FMT = {np.dtype(np.float32): (24, -126, 127), np.dtype(np.float64): (53, -1022, 1023)}
_FAR = 1e4  # |argument| beyond which exp / sinh / cosh / tanh are decided without evaluating them (2^±14427)


def _round_once(v, dtype):
    """(value, edge) of the mpf `v` rounded to nearest-even in `dtype`, as a Python float (exact: every Float32 is a
    Float64).  edge: the exact value lies within one ulp of the overflow threshold, or in the upper half of the interval
    that rounds to zero (a quarter to a half of the smallest subnormal) -- there one rounding more or less may tip the
    class.  (Just above that boundary the reference is a subnormal, and check_close's absolute allowance applies.)"""
    p, emin, emax = _FMT[np.dtype(dtype)]
    sign, man, exp, bc = v._mpf_
    if man == 0:
        return 0.0, False
    e = exp + bc - 1  # 2^e <= |v| < 2^(e+1)
    q = max(e - (p - 1), emin - (p - 1))  # exponent of the last place kept
    sh = q - exp
    if sh <= 0:
        m = man << -sh
    else:
        m = man >> sh
        rem = man - (m << sh)
        half = 1 << (sh - 1)
        if rem > half or (rem == half and (m & 1)):
            m += 1
    edge = False
    if e >= emax or e <= emin - p + 2:
        a = abs(v)
        with mpmath.workprec(PREC + 64):
            tiny = mpmath.ldexp(1, emin - p + 1)
            ulp = mpmath.ldexp(1, emax - p + 1)
            thr = mpmath.ldexp(2, emax) - ulp / 2  # largest finite + half an ulp
            edge = bool(abs(a - thr) <= ulp) or bool(tiny / 4 <= a <= tiny / 2)
    val = math.inf if m.bit_length() + q - 1 > emax else math.ldexp(float(m), q)
    return (-val if sign else val), edge


def _expm1(x):
    with mpmath.workprec(PREC + 32 + max(0, -mpmath.frexp(x)[1])):
        return mpmath.exp(x) - 1


def _log1p(x):
    with mpmath.workprec(PREC + 32 + max(0, -mpmath.frexp(x)[1])):
        return mpmath.log(1 + x)


_MP_UN = {
    "cbrt": lambda x: mpmath.sign(x) * mpmath.cbrt(abs(x)), "exp": mpmath.exp, "exp2": lambda x: mpmath.power(2, x),
    "expm1": _expm1, "log": mpmath.log, "log2": lambda x: mpmath.log(x, 2), "log10": mpmath.log10, "log1p": _log1p,
    "sin": mpmath.sin, "cos": mpmath.cos, "tan": mpmath.tan, "arcsin": mpmath.asin, "arccos": mpmath.acos,
    "arctan": mpmath.atan, "sinh": mpmath.sinh, "cosh": mpmath.cosh, "tanh": mpmath.tanh, "arcsinh": mpmath.asinh,
    "arccosh": mpmath.acosh, "arctanh": mpmath.atanh,
}
# where the mathematical function is defined and finite, for a finite non-zero argument (else: NumPy's class and sign)
_DOMAIN = {
    "log": lambda x: x > 0, "log2": lambda x: x > 0, "log10": lambda x: x > 0, "log1p": lambda x: x > -1,
    "arcsin": lambda x: abs(x) <= 1, "arccos": lambda x: abs(x) <= 1, "arccosh": lambda x: x >= 1,
    "arctanh": lambda x: abs(x) < 1,
}


def _far(name, x):
    """results that need no evaluation: the argument is so large that the function has long overflowed / saturated"""
    if abs(x) <= _FAR:
        return None
    if name in ("exp", "exp2"):
        return math.inf if x > 0 else 0.0
    if name == "expm1":
        return math.inf if x > 0 else -1.0
    if name == "sinh":
        return math.copysign(math.inf, x)
    if name == "cosh":
        return math.inf
    if name == "tanh":
        return math.copysign(1.0, x)
    return None


def _pow(a, b, dtype):
    """pow of finite non-zero a, b: (value, edge), or None where NumPy's class applies (negative base, fractional b)"""
    neg = False
    if a < 0:
        if b != math.floor(b):
            return None
        neg = abs(b) < 2.0 ** 53 and int(b) % 2 == 1
        a = -a
    t = math.log2(a) * b  # the result's exponent, roughly: far outside every format -> no evaluation
    if abs(t) > _FAR and not math.isinf(t):
        v, edge = (math.inf if t > 0 else 0.0), False
    elif math.isinf(t):
        v, edge = (math.inf if t > 0 else 0.0), False
    else:
        v, edge = _round_once(mpmath.power(mpmath.mpf(a), mpmath.mpf(b)), dtype)
    return (-v if neg else v), edge


def _reference(name, args, dtype):
    dtype = np.dtype(dtype)
    args = [np.ascontiguousarray(a, dtype=dtype) for a in args]
    with np.errstate(all="ignore"):
        host = np.asarray(np_fn(name)(*args))
    edge = np.zeros(host.shape, dtype=bool)
    if name not in TRANS_UN and name not in TRANS_BIN:
        return (host.astype(np.float64) if host.dtype == np.bool_ else host), edge
    out = host.copy()
    with mpmath.workprec(PREC):
        for i in range(len(out)):
            xs = [float(a[i]) for a in args]
            if not all(math.isfinite(x) and x != 0.0 for x in xs):
                continue
            if name in _MP_UN:
                if not _DOMAIN.get(name, lambda x: True)(xs[0]):
                    continue
                v = _far(name, xs[0])
                r = (v, False) if v is not None else _round_once(_MP_UN[name](mpmath.mpf(xs[0])), dtype)
            elif name == "pow":
                r = _pow(xs[0], xs[1], dtype)
                if r is None:
                    continue
            elif name == "arctan2":
                r = _round_once(mpmath.atan2(mpmath.mpf(xs[0]), mpmath.mpf(xs[1])), dtype)
            else:  # hypot
                a, b = mpmath.mpf(xs[0]), mpmath.mpf(xs[1])
                with mpmath.workprec(PREC + 64):
                    r = _round_once(mpmath.sqrt(a * a + b * b), dtype)
            out[i], edge[i] = r
    return out, edge


def ref_unary(name, x, dtype, edges=False):
    """the expected value of unary operation `name` on `x` in `dtype` (module docstring); edges=True: also the mask of
    inputs whose exact result lies at the overflow threshold / zero's rounding boundary"""
    r = _reference(name, [x], dtype)
    return r if edges else r[0]


def ref_binary(name, a, b, dtype, edges=False):
    """as ref_unary, for a binary operation or a comparison (comparisons: 0.0 / 1.0 as Float64)"""
    r = _reference(name, [a, b], dtype)
    return r if edges else r[0]


# ---------------------------------------------------------------------------------------------------------------------
# inputs
def _cast(v, dtype):
    with np.errstate(all="ignore"):
        return np.asarray(v, dtype=np.float64).astype(dtype)


def _specials(dtype):
    fi = np.finfo(dtype)
    eps = float(fi.eps)
    return [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 0.5, -0.5, 2.0, 1e-300, -3.5,
            float(fi.tiny), -float(fi.tiny), float(fi.smallest_subnormal), -float(fi.smallest_subnormal) * 5,
            float(fi.tiny) / 8, float(fi.max), -float(fi.max), eps, 1 + eps, 1 - eps, -1 + eps, -1 - eps]


@functools.lru_cache(maxsize=None)
def _grid(dtype):
    dtype = np.dtype(dtype)
    fi = np.finfo(dtype)
    p = fi.nmant + 1
    rng = np.random.default_rng(20240816)
    v = list(_specials(dtype))
    # ties of rint, and the last magnitudes that still have a fractional part
    for t in (0.5, 1.5, 2.5, 3.5, 2.0 ** (p - 2) + 0.5, 2.0 ** (p - 1) - 0.5, 2.0 ** (p - 1) + 1, 2.0 ** p, 2.0 ** 52 - 0.5,
              2.0 ** 23 - 0.5, 0.49999999999999994, 0.5000001):
        v += [t, -t]
    # just inside and just outside the domain edges at ±1 (arcsin, arccos, arccosh, arctanh, log1p) and at 0
    one = np.ones((), dtype)
    for s in (1, -1):
        v += [float(np.nextafter(s * one, 0 * one)), float(np.nextafter(s * one, 2 * s * one)), s * (1 - 3 * float(fi.eps)),
              s * (1 + 3 * float(fi.eps)), s * 0.999, s * 1.001]
    # overflow / underflow thresholds of exp, exp2, expm1, sinh, cosh in both types
    thr = []
    for f in (np.finfo(np.float32), np.finfo(np.float64)):
        mx, tn, sub = float(f.max), float(f.tiny), float(f.smallest_subnormal)
        thr += [math.log(mx), math.log(tn), math.log(sub), math.log(sub) - math.log(2), math.log(mx) + math.log(2), math.log2(mx),
                math.log2(tn), math.log2(sub), math.log2(sub) - 1, float(f.maxexp), float(f.minexp)]
    thr += [89.0, 710.0, -104.0, -746.0, 37.5, -37.5, 17.5, -17.5]  # (expm1 -> -1, tanh -> ±1 in either type)
    for t in thr:
        for k in (-64, -3, -1, 0, 1, 3, 64):
            v += [t * (1 + k * float(fi.eps)), -t * (1 + k * float(fi.eps))]
        v += [t - 1, t + 1, math.floor(t), math.ceil(t)]
    # large trigonometric arguments
    v += [1e22, -1e22, 1e15, 1e10, 3e38, 1e300]
    for k in range(0, 64, 3):
        for c in (math.pi, math.pi / 2):
            x = _cast(c * 2.0 ** k, dtype)
            v += [float(x), float(np.nextafter(x, np.inf * one)), float(np.nextafter(x, -np.inf * one)), -float(x)]
    v += list(rng.uniform(-1e6, 1e6, 200))
    # magnitudes over ±40 decades (as far as the type reaches), both signs
    hi = min(40.0, math.floor(math.log10(float(fi.max))))
    v += list(10.0 ** rng.uniform(-40, hi, 300) * rng.choice([-1.0, 1.0], 300))
    # what the other tests draw
    v += list(rng.standard_normal(300) * 3) + list(rng.standard_normal(100) * 2) + list(rng.uniform(-1, 1, 200))
    out = _cast(v, dtype)
    out.setflags(write=False)
    return out


def grid(dtype):
    """the unary inputs in `dtype` (read-only; the same array on every call)"""
    return _grid(np.dtype(dtype))


@functools.lru_cache(maxsize=None)
def _grid2(dtype):
    dtype = np.dtype(dtype)
    fi = np.finfo(dtype)
    rng = np.random.default_rng(20240817)
    mx, tn, sub = float(fi.max), float(fi.tiny), float(fi.smallest_subnormal)
    # (the largest finite value enters the cross product halved: hypot(max, anything small) sits AT the overflow threshold,
    #  which is the one place a case may exclude; the pairs with max itself are listed below)
    s = [v / 2 if abs(v) == mx else v for v in _specials(dtype)] + [3.0, -2.0, 1.5, 2.5, -1.5, 1e30, -1e-30, 7.0]
    pairs = [(a, b) for a in s for b in s]  # every special against every special (all signed-zero pairs, (Inf, NaN), ...)
    pairs += [(mx, 1.0), (mx, -mx), (-mx, np.nan), (mx, np.inf), (-mx, 0.0), (mx, -0.0), (1.0, mx), (-2.0, -mx), (mx, 0.5)]
    pairs += list(zip(rng.standard_normal(300) * 3, rng.standard_normal(300) * 3))
    pairs += list(zip(rng.uniform(0, 30, 100), rng.uniform(-20, 20, 100)))
    pairs += list(zip(10.0 ** rng.uniform(-30, 30, 100) * rng.choice([-1.0, 1.0], 100),
                      10.0 ** rng.uniform(-30, 30, 100) * rng.choice([-1.0, 1.0], 100)))
    # pow: negative bases with integer and non-integer exponents, ±0 bases with negative exponents, 1 and 0 against NaN,
    # results at the limits of either type
    for base in (-2.0, -0.5, -1.0, -3.5, -1e10, -tn):
        pairs += [(base, e) for e in (-5.0, -4.0, -3.0, -2.0, -1.0, 1.0, 2.0, 3.0, 4.0, 5.0, 0.5, -0.5, 2.5, 1e-3, 2.0 ** 53,
                                      2.0 ** 53 + 2, 2.0 ** 24 + 1, 1e300, -1e300)]
    pairs += [(z, e) for z in (0.0, -0.0) for e in (-1.0, -2.0, -3.0, -0.5, -np.inf, -2.5, -1e30, 1.0, 2.0, 3.0, 0.5, np.inf)]
    pairs += [(1.0, np.nan), (np.nan, 0.0), (np.nan, -0.0), (-1.0, np.inf), (-1.0, -np.inf), (1.0, np.inf), (np.nan, 1.0)]
    pairs += [(2.0, e) for e in (1023.0, 1024.0, -1074.0, -1075.0, -1076.0, 127.0, 128.0, -149.0, -150.0, -151.0, 0.5, -1022.5)]
    pairs += [(10.0, 308.0), (10.0, 309.0), (10.0, 38.0), (10.0, 39.0), (10.0, -45.0), (10.0, -46.0), (10.0, -323.0),
              (10.0, -324.0), (0.5, 1074.0), (0.5, 149.0), (1 + float(fi.eps), 1 / float(fi.eps)), (1 - float(fi.eps), -2 / float(fi.eps))]
    # fmod / remainder: quotients beyond 2^53, every sign combination, results that are exactly zero
    for a, b in ((mx * 0.75, 3.0), (mx / 2, 7.0), (mx / 4, 0.1), (2.0 ** 100, 3.0), (1e30, 1.5), (1e20, 0.1), (1e18, tn * 3), (mx * 0.75, sub * 3),
                 (6.0, 3.0), (7.5, 2.5), (2.0 ** 60, 2.0), (5.0, 3.0), (3.0, 5.0), (0.3, 0.1), (1.0, 0.1), (5.5, 0.25), (tn, sub),
                 (1e10, 1.0), (3.0, np.inf), (3.0, 3.0)):
        pairs += [(sa * a, sb * b) for sa in (1, -1) for sb in (1, -1)]
    # hypot: squares that overflow or underflow although the result does not; exact results in the subnormal range
    pairs += [(mx / 2, mx / 2), (mx, mx), (mx / 2, -mx / 3), (1e200, 1e200), (1e-200, 1e-200), (1e30, 1e30), (1e-30, 1e-30),
              (tn, tn), (sub, sub), (3 * sub, 4 * sub), (-3 * tn, 4 * tn), (mx, 3.0), (np.inf, np.nan), (np.nan, -np.inf)]
    # arctan2: results that underflow, quadrants at extreme ratios
    pairs += [(tn, mx / 2), (-tn, mx / 2), (sub, 1e10), (tn, -mx / 2), (-sub, -1.0), (mx / 2, tn), (1.0, -sub), (mx, -mx), (-mx, mx)]
    a = _cast([q[0] for q in pairs], dtype)
    b = _cast([q[1] for q in pairs], dtype)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def grid2(dtype):
    """the binary inputs in `dtype`: two read-only arrays of one length"""
    return _grid2(np.dtype(dtype))


# ---------------------------------------------------------------------------------------------------------------------
# comparisons
def _show(bad, cols, k=6):
    idx = np.flatnonzero(bad)[:k]
    return "; ".join("(" + ", ".join(repr(c[i].item()) for c in cols) + ")" for i in idx) + f"  [{int(bad.sum())} of {bad.size}]"


def check_exact(name, got, want, args=()):
    """bit equality (sign of zero included; NaNs by isnan).  One stated exception: minimum / maximum / fmin / fmax of the
    pair (+0, -0), where NumPy's own answer depends on how it was built -- those pairs are compared by value."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    it = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    ok = (got.view(it) == want.view(it)) | (np.isnan(got) & np.isnan(want))
    if name in MINMAX:
        a, b = args
        ok |= (a == 0) & (b == 0) & (np.signbit(a) != np.signbit(b)) & (got == want)
    assert ok.all(), f"{name} {got.dtype}: (inputs..., got, want) " + _show(~ok, list(args) + [got, want])
    return {"ulp": 0.0, "excluded": 0.0}


def check_close(name, got, ref, edge, args=()):
    """the transcendental gate, element by element: the same NaNs, the same ±Inf, the same sign on a zero result,
    |got - ref| <= tol |ref| elsewhere.  Where the reference is subnormal the bound is one spacing at that magnitude,
    absolutely, once that is the larger of the two (a subnormal just below the smallest normal is spaced as finely as a
    normal, relatively, and keeps the relative bound: NumPy's own Float32 exp2 is 2 spacings off there).  Inputs marked
    `edge` (at most MAX_EXCLUDED of them) are left out.  Returns the worst error in units of the reference's spacing (a
    whole number: both values are numbers of the type) and the excluded share."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (name, got.shape, ref.shape, got.dtype, ref.dtype)
    tol, tiny = TOL[ref.dtype], np.finfo(ref.dtype).tiny
    share = float(edge.mean())
    assert share <= MAX_EXCLUDED, f"{name} {ref.dtype}: {share:.2%} of the inputs excluded"
    cols = list(args) + [got, ref]
    keep = ~edge
    bad = keep & (np.isnan(got) != np.isnan(ref))
    assert not bad.any(), f"{name} {ref.dtype}: NaN sets differ " + _show(bad, cols)
    bad = keep & ((np.isinf(got) != np.isinf(ref)) | (np.isinf(ref) & (np.signbit(got) != np.signbit(ref))))
    assert not bad.any(), f"{name} {ref.dtype}: Inf sets differ " + _show(bad, cols)
    bad = keep & (ref == 0) & ((got != 0) | (np.signbit(got) != np.signbit(ref)))
    assert not bad.any(), f"{name} {ref.dtype}: zero results differ " + _show(bad, cols)
    fin = keep & np.isfinite(ref) & (ref != 0)
    g, r = got[fin].astype(np.float64), ref[fin].astype(np.float64)
    err = np.abs(g - r)
    mag = np.minimum(np.abs(ref[fin]), np.nextafter(np.finfo(ref.dtype).max, 0))  # (the largest finite: the spacing below it)
    spacing = np.spacing(mag).astype(np.float64)
    allowed = np.where(np.abs(r) < tiny, np.maximum(spacing, tol * np.abs(r)), tol * np.abs(r))
    bad = np.zeros(ref.shape, dtype=bool)
    bad[np.flatnonzero(fin)[err > allowed]] = True
    worst = float((err / spacing).max()) if err.size else 0.0
    assert not bad.any(), f"{name} {ref.dtype}: beyond {tol:g} (worst {worst:.2f} ulp) " + _show(bad, cols)
    return {"ulp": worst, "excluded": share}


@functools.lru_cache(maxsize=None)
def _grid_reference(name, dtype):
    args = [grid(dtype)] if name in K.UN else list(grid2(dtype))
    return _reference(name, args, dtype)


def grid_reference(name, dtype):
    """(reference, edge mask) of operation `name` over grid / grid2, computed once per process"""
    return _grid_reference(name, np.dtype(dtype))


def check_on_grid(name, got, dtype):
    """compare `got`, operation `name` over grid(dtype) / grid2(dtype), with the reference; the gate follows the class"""
    args = [grid(dtype)] if name in K.UN else list(grid2(dtype))
    ref, edge = grid_reference(name, dtype)
    if name in TRANS_UN or name in TRANS_BIN:
        return check_close(name, got, ref, edge, args)
    return check_exact(name, got, ref, args)
