"""`np.interp` in `elementwise` closures (include/sigops.h SO_EOP_INTERP; signaloperators.jl_amd/trace.py): what the
tracer records -- the program, the table in its constants, the types, the refusals, `period=` -- and the node tables
lowering makes of it, all without a device.  `interp_ref` restates NumPy's look-up in array operations exactly as the
device function (csrc/kmath.h so_interp) is specified; it is held to `np.interp` bit for bit here, on the very inputs the
device tests (tests/test_gpu_elementwise_interp.py) use."""
import ctypes as C
import os

import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import _capi as K
from sigops_amd import lowering as LW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 10 * so.kHz
INTERP, REMAINDER = K.EOP["interp"], K.BIN["remainder"]


# ---- the yardstick ---------------------------------------------------------------------------------------------------
def interp_ref(x, xp, fp, left=None, right=None, paths=False):
    """np.interp(x, xp, fp, left, right) restated operation for operation (include/sigops.h SO_EOP_INTERP).  paths: also
    the samples that take NumPy's first NaN fall-back (the slope from the other knot) and its second (fp[j] itself)"""
    x = np.asarray(x, dtype=np.float64)
    xp, fp = np.asarray(xp, dtype=np.float64), np.asarray(fp, dtype=np.float64)
    n = xp.shape[0]
    left = fp[0] if left is None else np.float64(left)
    right = fp[-1] if right is None else np.float64(right)
    none = np.zeros(x.shape, dtype=bool)
    with np.errstate(all="ignore"):
        if n == 1:  # (NumPy: a NaN is neither left nor right of the only knot)
            r = np.where(x < xp[0], left, np.where(x > xp[0], right, fp[0]))
            return (r, none, none) if paths else r
        j = np.clip(np.searchsorted(xp, x, side="right") - 1, 0, n - 2)  # xp[j] <= x < xp[j+1] inside the table
        x0, x1, f0, f1 = xp[j], xp[j + 1], fp[j], fp[j + 1]
        s = (f1 - f0) / (x1 - x0)
        r1 = s * (x - x0) + f0
        r2 = s * (x - x1) + f1
        inside = ~np.isnan(x) & (x >= xp[0]) & (x < xp[-1]) & (x != x0)
        fb1 = np.isnan(r1)
        fb2 = fb1 & np.isnan(r2) & (f0 == f1)
        r = np.where(fb1, r2, r1)
        r = np.where(fb2, f0, r)
        r = np.where(x == x0, f0, r)
        r = np.where(x == xp[-1], fp[-1], r)
        r = np.where(x > xp[-1], right, r)
        r = np.where(x < xp[0], left, r)
        r = np.where(np.isnan(x), x, r)
    return (r, inside & fb1, inside & fb2) if paths else r


def same_bits(a, b):
    """equal bit for bit; NaNs equal NaNs (their payloads are not compared)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.int64), b[ok].view(np.int64))


# ---- the inputs of the device tests (shared: the reference is pinned on exactly these) --------------------------------
def table(kind, n, seed=0):
    """(xp, fp): n knots over about [-3, 3], `uniform` or `random`; xp is exact in Float32 too, so that Float32 samples
    can sit on knots"""
    rng = np.random.default_rng(1000 + 7 * n + seed)
    if kind == "uniform":
        xp = (np.arange(n, dtype=np.float64) - (n - 1) / 2) * (2.0 ** -13 if n > 1024 else 2.0 ** -3)
    else:
        xp = np.unique(rng.uniform(-3.0, 3.0, 2 * n + 8).astype(np.float32).astype(np.float64))
        xp = np.sort(rng.choice(xp, n, replace=False))
    assert xp.shape[0] == n and (n == 1 or (np.diff(xp) > 0).all())
    return xp, rng.standard_normal(n)


TABLES = [("random", 1), ("random", 2), ("random", 3), ("random", 17), ("random", 1024), ("uniform", 65536)]


def planted(rng, n, nch, xp, dt=np.float64):
    """`standard_normal * 2` (wider than the table) with 500 exact knots, both end knots, +-Inf, NaN and -0.0 planted"""
    x = np.asfortranarray(rng.standard_normal((n, nch)) * 2).astype(dt, order="F")
    flat = x.reshape(-1, order="F")
    where = rng.choice(flat.shape[0], 500 + 6, replace=False)
    flat[where[:500]] = rng.choice(xp, 500).astype(dt)
    flat[where[500:]] = np.asarray([xp[0], xp[-1], np.inf, -np.inf, np.nan, -0.0], dtype=dt)
    return np.asfortranarray(flat.reshape((n, nch), order="F"))


def nonfinite_table():
    """17 knots whose fp holds Inf (twice next to each other, once alone) and a NaN: both of NumPy's fall-backs occur"""
    xp, fp = table("random", 17, seed=5)
    fp = fp.copy()
    fp[3] = fp[4] = np.inf   # between them: the slope is NaN, both products are NaN, fp[j] == fp[j+1] -> fp[j]
    fp[9] = -np.inf          # left of it the first form is finite, right of it -Inf*(x - x0) + (-Inf) ... the other knot
    fp[13] = np.nan
    return xp, fp


def program(fn, dts=(np.float64,)):
    (p,), dt = so.elementwise(fn).program(list(dts))
    return p[0], p[1], dt


def stored(consts, off):
    n = int(consts[off])
    return n, consts[off + 1], consts[off + 2], consts[off + 3:off + 3 + n], consts[off + 3 + n:off + 3 + 2 * n]


# ---- tracer ----------------------------------------------------------------------------------------------------------
def test_interp_traces_to_one_table_operation():
    """(fails before the feature: the trace raised `np.interp is not traceable`)"""
    xp, fp = table("random", 17)
    code, consts, dt = program(lambda x: np.interp(x, xp, fp))
    assert code.tolist() == [[K.EOP["arg"], 0], [INTERP, 0]] and dt == np.float64
    n, left, right, sx, sf = stored(consts, 0)
    assert n == 17 and left == fp[0] and right == fp[-1]
    assert sx.tobytes() == xp.tobytes() and sf.tobytes() == fp.tobytes() and consts.size == 3 + 2 * 17


def test_table_contents_left_right_and_conversion_to_float64():
    xp = [0, 1, 4]                                  # integers
    fp = np.asarray([1.5, -2.0, 0.25], dtype=np.float32)
    code, consts, _ = program(lambda x: 2.0 * np.interp(x, xp, fp, left=-7, right=np.float32(0.1)))
    (off,) = [a for c, a in code.tolist() if c == INTERP]
    assert off == 1 and consts[0] == 2.0            # the scalar constants first, the tables behind them
    n, left, right, sx, sf = stored(consts, off)
    assert consts.dtype == np.float64 and n == 3
    assert left == -7.0 and right == np.float64(np.float32(0.1))
    assert sx.tolist() == [0.0, 1.0, 4.0] and sf.tolist() == [1.5, -2.0, 0.25]
    # keyword spelling, one knot
    code, consts, _ = program(lambda x: np.interp(x=x, xp=[2.0], fp=[5.0], right=1.0))
    assert stored(consts, 0)[:3] == (1, 5.0, 1.0)


def test_result_type_is_float64_also_for_float32_arguments():
    xp, fp = table("random", 3)
    code, _, dt = program(lambda x: np.interp(x, xp, fp), (np.float32,))
    assert dt == np.float64 == np.interp(np.float32(0.5), xp, fp).dtype
    assert code.tolist() == [[K.EOP["arg"], 0], [INTERP, 0]]  # no ROUND32 behind the look-up
    # ... while Float32 arithmetic in front of it still rounds, and Float64 arithmetic behind it does not
    code, _, dt = program(lambda x: np.interp(x * x, xp, fp) + 1.0, (np.float32,))
    ops = [c for c, _ in code.tolist()]
    assert dt == np.float64 and ops.count(K.EOP["round32"]) == 1 and ops.index(K.EOP["round32"]) < ops.index(INTERP)


def test_one_table_used_twice_is_stored_once_and_two_tables_twice():
    xp, fp = table("random", 17)
    xq, fq = table("random", 3)
    code, consts, _ = program(lambda x, y: np.interp(x, xp, fp) - np.interp(y, xp.copy(), list(fp)), (np.float64, np.float64))
    offs = [a for c, a in code.tolist() if c == INTERP]
    assert len(offs) == 2 and offs[0] == offs[1] and consts.size == 3 + 2 * 17
    code, consts, _ = program(lambda x: np.interp(np.interp(x, xp, fp), xq, fq) * np.interp(x, xp, fp))
    offs = [a for c, a in code.tolist() if c == INTERP]
    assert len(offs) == 3 and len(set(offs)) == 2 and consts.size == (3 + 2 * 17) + (3 + 2 * 3)
    assert stored(consts, offs[1])[3].tobytes() == xq.tobytes()


def test_constant_x_is_folded_by_numpy():
    xp, fp = table("random", 17)
    code, consts, _ = program(lambda x: x * np.interp(0.25, xp, fp))
    assert INTERP not in [c for c, _ in code.tolist()] and consts.tolist() == [np.interp(0.25, xp, fp)]


def test_tables_that_differ_in_one_bit_between_the_traces_are_not_pure():
    xp, fp = table("random", 17)
    calls = []

    def drifting(x):
        t = fp.copy()
        if len(calls) % 2:
            t[5] = np.nextafter(t[5], np.inf)  # one bit of one knot
        calls.append(1)
        return np.interp(x, xp, t)

    with pytest.raises(so.ErrorException, match="not pure"):
        so.elementwise(drifting).program([np.float64])
    so.elementwise(lambda x: np.interp(x, xp, fp.copy())).program([np.float64])  # equal bytes: pure


REFUSALS = [
    ("traced xp", lambda x: np.interp(x, [0.0, x], [0.0, 1.0]), "traced"),
    ("traced fp", lambda x, y: np.interp(x, [0.0, 1.0], [y, 1.0]), "traced"),
    ("n = 0", lambda x: np.interp(x, [], []), "empty"),
    ("n > 1048576", lambda x: np.interp(x, np.arange(1048577.0), np.zeros(1048577)), "too large"),
    ("unequal lengths", lambda x: np.interp(x, [0.0, 1.0], [0.0, 1.0, 2.0]), "same length"),
    ("complex fp", lambda x: np.interp(x, [0.0, 1.0], [1j, 0.0]), "complex"),
    ("NaN in xp", lambda x: np.interp(x, [0.0, np.nan, 2.0], [0.0, 1.0, 2.0]), "NaN in xp"),
    ("equal knots", lambda x: np.interp(x, [0.0, 1.0, 1.0], [0.0, 1.0, 2.0]), "strictly increasing"),
    ("decreasing xp", lambda x: np.interp(x, [2.0, 1.0, 0.0], [0.0, 1.0, 2.0]), "strictly increasing"),
    ("two-dimensional", lambda x: np.interp(x, np.zeros((2, 2)), np.zeros((2, 2))), "one-dimensional"),
    ("left not a number", lambda x: np.interp(x, [0.0, 1.0], [0.0, 1.0], left="a"), "left"),
    ("period = 0", lambda x: np.interp(x, [0.0, 1.0], [0.0, 1.0], period=0), "non-zero"),
]


@pytest.mark.parametrize("what,fn,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_the_problem(what, fn, word):
    nargs = fn.__code__.co_argcount
    with pytest.raises(so.ErrorException, match=word):
        so.elementwise(fn).program([np.float64] * nargs)


def test_the_largest_table_is_accepted():
    n = 1 << 20
    code, consts, _ = program(lambda x: np.interp(x, np.arange(float(n)), np.zeros(n)))
    assert consts.size == 3 + 2 * n and consts[0] == n


def test_period_is_remainder_then_the_plain_table_operation():
    xp, fp = [190.0, -190.0, 350.0, -350.0], [5.0, 10.0, 3.0, 4.0]  # NumPy's own example
    for dts in ((np.float64,), (np.float32,)):
        code, consts, dt = program(lambda x: np.interp(x, xp, fp, left=99.0, right=-99.0, period=-360), dts)
        assert dt == np.float64
        assert code.tolist()[:3] == [[K.EOP["arg"], 0], [K.EOP["const"], 0], [K.EOP["bin"], REMAINDER]]
        assert code.tolist()[3:] == [[INTERP, 1]] and consts[0] == 360.0  # (no ROUND32: the remainder is taken in Float64)
        n, left, right, sx, sf = stored(consts, 1)
        assert n == 6 and sx.tolist() == [-10.0, 10.0, 170.0, 190.0, 350.0, 370.0]
        assert sf.tolist() == [3.0, 4.0, 10.0, 5.0, 3.0, 4.0]
        assert (left, right) == (3.0, 4.0)  # `left` / `right` are ignored, as NumPy ignores them
    x = np.asarray([-180.0, -170.0, -185.0, 185.0, -10.0, -5.0, 0.0, 365.0, 1e6, -0.0])
    assert same_bits(interp_ref(np.remainder(x, 360.0), sx, sf), np.interp(x, xp, fp, period=360))
    with pytest.raises(so.ErrorException, match="strictly increasing"):  # 0 and 1 are the same point of the period
        program(lambda x: np.interp(x, [0.0, 1.0], [0.0, 1.0], period=1.0))


# ---- lowering --------------------------------------------------------------------------------------------------------
def test_lowering_states_the_length_of_the_constants():
    xp, fp = table("random", 17)
    f = so.elementwise(lambda x: np.interp(x, xp, fp) * 0.5)
    x = so.Signal(np.zeros((64, 2)), FS)
    trees = [so.OperateOn(f, x), so.Amplify(x, so.Signal(f, FS)) | so.Until(64 * so.frames), so.RampOn(x, 0.001 * so.s, f)]
    for tree in trees:
        lw = LW.lower(tree)
        nodes = [lw.nodes[i] for i in range(lw.n) if lw.nodes[i].p1 and lw.nodes[i].kind in (K.NODE_MAP, K.NODE_RAMP)]
        assert len(nodes) == 1
        nd = nodes[0]
        assert nd.s0 == 1 + 3 + 2 * 17
        consts = np.ctypeslib.as_array(C.cast(nd.p1, C.POINTER(C.c_double)), shape=(nd.s0,))
        assert consts[0] == 0.5 and stored(consts, 1)[3].tobytes() == xp.tobytes()
        plen = nd.i2 if nd.kind == K.NODE_RAMP else nd.i3
        code = np.ctypeslib.as_array(C.cast(nd.p0, C.POINTER(C.c_int32)), shape=(plen, 2))
        assert [INTERP, 1] in code.tolist()


def test_a_different_table_per_output_channel():
    ta, tb = table("random", 3), table("random", 17)
    f = so.elementwise(lambda fr: (np.interp(fr[0], *ta), np.interp(fr[1], *tb)))
    progs, dt = f.program([np.float64], bychannel=False, nch=[2])
    assert dt == np.float64 and len(progs) == 2
    assert [stored(c, 0)[0] for _, c in progs] == [3, 17]


# ---- the yardstick is NumPy's ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", TABLES + [("uniform", 2), ("uniform", 3), ("uniform", 17), ("uniform", 1024), ("random", 65536)])
def test_reference_helper_equals_numpy_bit_for_bit(kind, n):
    xp, fp = table(kind, n)
    for nch, dt in ((1, np.float64), (3, np.float64), (8, np.float64), (2, np.float32)):
        x = planted(np.random.default_rng(100 * n + nch), 4099 if nch == 3 else 30_000, nch, xp, dt)
        assert np.isnan(x).any() and np.isinf(x).any() and (x == xp[0]).any() and np.signbit(x[x == 0]).any()
        for kw in ({}, {"left": -7.5, "right": np.inf}):
            assert same_bits(interp_ref(x, xp, fp, **kw), np.interp(x, xp, fp, **kw)), (kind, n, nch, kw)


def test_reference_helper_with_non_finite_fp_takes_both_fall_backs():
    xp, fp = nonfinite_table()
    x = planted(np.random.default_rng(77), 30_000, 2, xp)
    got, fb1, fb2 = interp_ref(x, xp, fp, paths=True)
    assert same_bits(got, np.interp(x, xp, fp))
    assert (fb1 & ~fb2).any() and fb2.any()
    assert np.isnan(got[~np.isnan(x)]).any() and np.isinf(got).any()


# ---- the device function as hipRTC source ----------------------------------------------------------------------------
def test_pointwise_body_with_the_table_operation_compiles_for_gfx950_without_a_device():
    """the source rtc.cpp writes for a step with a table: kmath.h in front, `so_interp` on the leaf that holds the table"""
    km = open(os.path.join(ROOT, "signaloperators.jl_amd", "csrc", "kmath.h")).read()
    km = "\n".join(l for l in km.splitlines() if not l.startswith("#pragma once") and not l.startswith("#include"))
    body = km + r'''
__device__ __forceinline__ void p0_frame(const DLeaf* __restrict__ L, long long N, double* M) {
    const int C = 0; (void)C; (void)N; (void)L; (void)M;
    M[0] = so_interp((const double*)L[2].base, func_eval(L[1], N));
}
__device__ __forceinline__ double p0_samp(const DLeaf* __restrict__ L, long long N, int C, const double* M, const double* X) {
    (void)N; (void)C; (void)L; (void)M; (void)X;
    return (so_m_tanh(so_interp((const double*)L[3].base, X[0])) * M[0]);
}
extern "C" __global__ __launch_bounds__(256) void k_rtc(const DPiece* __restrict__ pieces, int npieces, const DLeaf* __restrict__ L, OutView out) {
    const long long bid = blockIdx.x;
    const DPiece P = pieces[0];
    const long long n0 = P.a + bid * 512ll + 2ll * threadIdx.x;
    if (n0 >= P.b || npieces < 1) return;
    const bool ok1 = n0 + 1 < P.b;
    const long long n1 = ok1 ? n0 + 1 : n0;
    double M0[1], M1[1];
    p0_frame(L, n0, M0);
    p0_frame(L, n1, M1);
    for (int c = P.c0; c < P.c1; ++c) {
        double X0[1], X1[1];
        so_load2(L[0], n0, c, ok1, X0[0], X1[0]);
        so_store2(out, n0, c, p0_samp(L, n0, c, M0, X0), p0_samp(L, n1, c, M1, X1), ok1);
    }
}
'''
    log = C.create_string_buffer(8000)
    st = K.lib().so_rtc_compile_check(body.encode(), log, 8000)
    assert st == 0, log.value.decode()


def test_the_device_function_compiled_for_the_host_equals_numpy(tmp_path):
    """csrc/kmath.h `so_interp` itself -- the text both device paths compile -- built with the host compiler
    (-ffp-contract=off, as the device units are) and held to `np.interp` bit for bit: the device tests' inputs, non-finite
    fp, and tables a linear first guess is useless or undefined on (infinite knots, a range that overflows, knots
    clustered at one end, heavy-tailed knots)"""
    import shutil
    import subprocess

    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "interp_host.cpp"
    src.write_text('#include <cmath>\n#define __device__\n#define __forceinline__ inline\n#include "%s"\n'
                   'extern "C" void run(const double* t, const double* x, double* out, long n) {\n'
                   '    for (long i = 0; i < n; ++i) out[i] = so::so_interp(t, x[i]);\n}\n'
                   % os.path.join(ROOT, "signaloperators.jl_amd", "csrc", "kmath.h"))
    lib = tmp_path / "libinterp_host.so"
    subprocess.check_call([cxx, "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(lib), str(src)])
    run = C.CDLL(str(lib)).run
    run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]

    def dev(x, xp, fp, left=None, right=None):
        t = np.concatenate(([len(xp), fp[0] if left is None else left, fp[-1] if right is None else right], xp, fp))
        xf = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))
        out = np.empty_like(xf)
        run(t.ctypes.data, xf.ctypes.data, out.ctypes.data, xf.size)
        return out.reshape(np.shape(x))

    for kind, n in TABLES + [("uniform", 2), ("uniform", 17), ("random", 5), ("random", 65536)]:
        xp, fp = table(kind, n)
        x = planted(np.random.default_rng(n), 30_000, 2, xp)
        for kw in ({}, {"left": -7.5, "right": np.inf}):
            assert same_bits(dev(x, xp, fp, **kw), np.interp(x, xp, fp, **kw)), (kind, n, kw)
    xp, fp = nonfinite_table()
    x = planted(np.random.default_rng(77), 30_000, 2, xp)
    assert same_bits(dev(x, xp, fp), np.interp(x, xp, fp))
    hostile = [np.asarray([-np.inf, 0.0, 1.0, np.inf]), np.asarray([-1e308, 0.0, 1e308]),
               np.concatenate((np.linspace(0.0, 1e-300, 50), [1.0, 1e300])),
               np.unique(np.random.default_rng(1).standard_cauchy(999))]
    for xp in hostile:
        fp = np.random.default_rng(2).standard_normal(xp.shape[0])
        x = np.concatenate((np.random.default_rng(3).standard_cauchy(20_000) * 3, xp, [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-310]))
        with np.errstate(all="ignore"):
            assert same_bits(dev(x, xp, fp), np.interp(x, xp, fp)), xp[:4]
