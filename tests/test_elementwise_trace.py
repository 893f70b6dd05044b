"""`elementwise` closures traced into expression programs (include/sigops.h so_eop_t; signaloperators.jl_amd/trace.py):
what the tracer records, its types and its errors, and the node tables lowering makes of them -- all without a device.
The device side is tests/test_gpu_elementwise.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import _capi as K
from sigops_amd import lowering as LW
from sigops_amd import signals as S
from eop_ref import run_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def values(rng, n=160):
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 0.5, -0.5, 2.0, 1e-300, -3.5])
    return np.concatenate([special, rng.standard_normal(n) * 3, rng.uniform(-0.99, 0.99, n // 4)])


# (closure, number of arguments): together every so_un_t / so_bin_t / so_cmp_t id, select, both Python spellings
CLOSURES = [
    (lambda x: -x, 1), (lambda x: +x, 1), (lambda x: abs(x), 1), (lambda x: np.sqrt(x), 1), (lambda x: np.cbrt(x), 1),
    (lambda x: np.square(x), 1), (lambda x: np.reciprocal(x), 1), (lambda x: np.exp(x), 1), (lambda x: np.exp2(x), 1),
    (lambda x: np.expm1(x), 1), (lambda x: np.log(x), 1), (lambda x: np.log2(x), 1), (lambda x: np.log10(x), 1),
    (lambda x: np.log1p(x), 1), (lambda x: np.sin(x), 1), (lambda x: np.cos(x), 1), (lambda x: np.tan(x), 1),
    (lambda x: np.arcsin(x), 1), (lambda x: np.arccos(x), 1), (lambda x: np.arctan(x), 1), (lambda x: np.sinh(x), 1),
    (lambda x: np.cosh(x), 1), (lambda x: np.tanh(2.5 * x), 1), (lambda x: np.arcsinh(x), 1),
    (lambda x: np.arccosh(x), 1), (lambda x: np.arctanh(x), 1), (lambda x: np.floor(x), 1), (lambda x: np.ceil(x), 1),
    (lambda x: np.trunc(x), 1), (lambda x: np.rint(3.3 * x), 1), (lambda x: np.sign(x), 1),
    (lambda x, y: x + y - 0.25, 2), (lambda x, y: x * y / 3.0, 2), (lambda x, y: np.power(x, y), 2),
    (lambda x: x ** 3.0, 1), (lambda x: 2.0 ** x, 1), (lambda x, y: x % y, 2), (lambda x, y: np.fmod(x, y), 2),
    (lambda x, y: np.minimum(x, y), 2), (lambda x, y: np.maximum(x, y), 2), (lambda x, y: np.fmin(x, y), 2),
    (lambda x, y: np.fmax(x, y), 2), (lambda x, y: np.arctan2(x, y), 2), (lambda x, y: np.hypot(x, y), 2),
    (lambda x, y: np.copysign(x, y), 2), (lambda x, y: (x < y) * 1.0, 2), (lambda x, y: (x <= y) + 0.0, 2),
    (lambda x, y: 1.0 * (x > y), 2), (lambda x, y: (x >= y) * x, 2), (lambda x, y: (x == y) - 0.5, 2),
    (lambda x, y: (x != y) * y, 2), (lambda x, y: np.where(x > 0, x, y), 2), (lambda x: np.clip(x, -1.0, 0.5), 1),
    (lambda x, y, z: np.where(z < 0.3, np.sqrt(x * x + y * y), np.tanh(z) - x), 3),
]
# np.float_power is recorded as pow: NumPy's own float_power and power differ in the last bit now and then
FLOAT_POWER = lambda x: np.float_power(x, 2.5)  # noqa: E731
CLOSURES.append((FLOAT_POWER, 1))


def _ids():
    seen = {"un": set(), "bin": set(), "cmp": set(), "select": False}
    for fn, n in CLOSURES:
        (prog,), _ = so.elementwise(fn).program([np.float64] * n)
        for op, arg in prog[0]:
            if op == K.EOP["un"]:
                seen["un"].add(int(arg))
            elif op == K.EOP["bin"]:
                seen["bin"].add(int(arg))
            elif op == K.EOP["cmp"]:
                seen["cmp"].add(int(arg))
            elif op == K.EOP["select"]:
                seen["select"] = True
    return seen


def test_the_closures_cover_every_operation():
    seen = _ids()
    assert seen["un"] == set(K.UN.values())
    assert seen["bin"] == set(K.BIN.values())
    assert seen["cmp"] == set(K.CMP.values())
    assert seen["select"]


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("k", range(len(CLOSURES)))
def test_program_evaluates_to_the_closure(k, dt):
    fn, n = CLOSURES[k]
    rng = np.random.default_rng(100 + k)
    v = values(rng)
    args = [v] + [np.roll(values(rng), 3 * j + 1) for j in range(1, n)]
    args = [a.astype(dt) for a in args]
    (prog,), odt = so.elementwise(fn).program([dt] * n)
    with np.errstate(all="ignore"):
        want = np.asarray(fn(*args))
    assert odt == (want.dtype if want.dtype != np.bool_ else np.dtype(np.bool_))
    got = run_program(prog[0], prog[1], [a.astype(np.float64) for a in args])
    want = want.astype(np.float64)
    if fn is FLOAT_POWER:
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.allclose(got, want, rtol=4e-16, atol=0, equal_nan=True)
        return
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), (k, dt, args[0][bad][:4], got[bad][:4], want[bad][:4])


def _test_dtype(fn, sigs, bychannel=True):
    plain = so.OperateOn(fn, *sigs, bychannel=bychannel)  # host path: test-value inference
    marked = so.OperateOn(so.elementwise(fn), *sigs, bychannel=bychannel)
    assert isinstance(plain.fn, S.OpaqueFn) and isinstance(marked.fn, S.ExprFn)
    assert marked.dtype == plain.dtype and marked.nch == plain.nch
    return marked


@pytest.mark.parametrize("fn,dts,want", [
    (lambda x: x * 2.5 + 1, [np.float32], np.float32),                      # Python constants are weak
    (lambda x: x * np.float64(2.5), [np.float32], np.float64),              # a NumPy Float64 constant is not
    (lambda x: np.tanh(x) * np.float32(0.1), [np.float32], np.float32),
    (lambda x, y: x + y, [np.float32, np.float64], np.float64),             # mixed operands
    (lambda x, y: np.hypot(x, y) - 1, [np.float32, np.float32], np.float32),
    (lambda x: x > 0.5, [np.float32], np.float64),                          # a Boolean result is stored as Float64
    (lambda x: np.where(x > 0, x, 0.25), [np.float32], np.float32),
    (lambda x: np.sqrt(2.0) * x, [np.float32], np.float64),                 # np.sqrt(2.0) is a Float64 scalar
    (lambda x: 1.0, [np.float32], np.float64),
])
def test_traced_dtype_equals_test_value_inference(fn, dts, want):
    sigs = [so.Signal(np.ones(8, dtype=d), 100) for d in dts]
    m = _test_dtype(fn, sigs)
    assert m.dtype == want


def test_float32_constants_are_rounded_as_numpy_rounds_them():
    (prog,), _ = so.elementwise(lambda x: x * 0.1).program([np.float32])
    assert prog[1][0] == float(np.float32(0.1))  # the weak scalar in the operation's type
    (prog,), _ = so.elementwise(lambda x: x * 0.1).program([np.float64])
    assert prog[1][0] == 0.1
    x = np.random.default_rng(3).standard_normal(1000).astype(np.float32)
    (prog,), _ = so.elementwise(lambda x: np.tanh(x * 0.1) + 3).program([np.float32])
    assert (prog[0][:, 0] == K.EOP["round32"]).sum() == 3
    assert np.array_equal(run_program(prog[0], prog[1], [x]), (np.tanh(x * 0.1) + 3).astype(np.float64))


def test_channel_closures_dtype_and_programs():
    x = so.Signal(np.ones((8, 3), dtype=np.float32), 100)
    m = _test_dtype(lambda fr: ((fr[0] + fr[1]) / 2, (fr[0] - fr[1]) / 2), [x], bychannel=False)
    assert m.nch == 2 and m.dtype == np.float32 and len(m.programs) == 2
    m = _test_dtype(lambda fr: (fr[2], fr[0], fr[1]), [x], bychannel=False)
    assert [list(p[0][:, 1]) for p in m.programs] == [[2], [0], [1]]
    y = so.Signal(np.ones((8, 2)), 100)
    m = _test_dtype(lambda a, b: np.hypot(a[0], b[1]), [x, y], bychannel=False)
    assert m.nch == 1 and list(m.programs[0][0][:2, 1]) == [0, 4]  # arguments: operand by operand, channel by channel


def _raises(fn, match, nargs=1):
    with pytest.raises(so.ErrorException, match=match):
        so.OperateOn(so.elementwise(fn), *[so.Signal(np.ones(8), 100)] * nargs)


def test_untraceable_closures_raise_helpful_errors():
    _raises(lambda x: x if x > 0 else -x, r"`if`.*np\.where")
    _raises(lambda x: math.exp(x), r"math\.\*.*np\.")
    _raises(lambda x: float(x) * 2, r"float\(x\)")
    _raises(lambda x: np.frexp(x)[0], r"np\.frexp is not a traceable ufunc")
    _raises(lambda x: np.logaddexp(x, 1.0), r"np\.logaddexp is not a traceable ufunc")
    rng = np.random.default_rng(5)
    _raises(lambda x: x + rng.standard_normal(), r"not pure")
    count = [0]

    def counter(x):
        count[0] += 1
        return x * count[0]

    _raises(counter, r"not pure")
    with pytest.raises(so.ErrorException, match="ramp"):
        so.RampOn(so.Signal(np.ones(8), 100), 0.02 * so.s, lambda u: u ** 2)  # an unmarked closure stays refused


def test_unmarked_closures_keep_the_host_path():
    x = so.Signal(np.ones(8), 100)
    assert isinstance(so.OperateOn(lambda a: np.tanh(a), x).fn, S.OpaqueFn)
    assert isinstance(so.OperateOn(np.tanh, x).fn, S.OpaqueFn)
    assert so.Signal(lambda t: 2 * t, 100).fn == S.OPAQUE


def test_a_marked_closure_is_called_a_few_times_not_per_frame():
    calls = [0]

    @so.elementwise
    def soft(x):
        calls[0] += 1
        return np.tanh(3 * x)

    x = np.zeros((1_000_000, 2))
    tree = so.OperateOn(soft, so.Signal(x, 48 * so.kHz)) | so.Amplify(0.5)
    LW.lower(tree)
    LW.lower(tree)
    assert calls[0] <= 4


def _kinds(lw):
    return [(lw.nodes[i].kind, lw.nodes[i].i0, lw.nodes[i].i1) for i in range(lw.n)]


def test_lowering_makes_expression_nodes_and_no_host_leaf():
    rng = np.random.default_rng(7)
    a = np.asfortranarray(rng.standard_normal((5000, 2)))
    b = np.asfortranarray(rng.standard_normal((4000, 2)))
    fs = 10 * so.kHz
    trees = [
        so.OperateOn(so.elementwise(lambda x, y: np.hypot(x, y)), so.Signal(a, fs), so.Signal(b, fs)),
        so.OperateOn(so.elementwise(lambda fr: (fr[0] + fr[1], fr[0] - fr[1])), so.Signal(a, fs), bychannel=False),
        so.Amplify(so.Signal(a, fs), so.Signal(so.elementwise(lambda t: np.exp(-0.5 * t)), fs)),
        so.Amplify(so.Signal(a, fs), so.Signal(so.elementwise(lambda t: np.sin(t) ** 3.0), fs, ω=440 * so.Hz)),
        so.RampOn(so.Signal(a, fs), 0.1 * so.s, so.elementwise(lambda u: u ** 2)),
        so.Ramp(so.Signal(a, fs), 0.1 * so.s, np.sqrt),
        so.FadeTo(so.Signal(a, fs), so.Signal(b, fs), 0.05 * so.s, so.elementwise(lambda u: u * u * 0.5)),
        so.OperateOn(so.elementwise(lambda x: np.tanh(2.5 * x)), so.Signal(a, fs)) | so.Filt(so.Lowpass, 1 * so.kHz),
    ]
    for t in trees:
        lw = LW.lower(t)
        kinds = _kinds(lw)
        arrays = [lw.nodes[i] for i in range(lw.n) if lw.nodes[i].kind == K.NODE_ARRAY]
        assert all(n.p0 in (a.ctypes.data, b.ctypes.data) for n in arrays), "a host-materialised leaf"
        assert all(n.nframes != K.SO_LEN_UNCHECKED for n in arrays)
        has_map = any(k[0] == K.NODE_MAP and k[1] == K.MAPFN["expr"] for k in kinds)
        has_ramp = any(k[0] == K.NODE_RAMP and k[2] == K.RAMPFN["expr"] for k in kinds)
        assert has_map or has_ramp
    lw = LW.lower(trees[1])
    getchans = [k for k in _kinds(lw) if k[0] == K.NODE_MAP and k[1] == K.MAPFN["getchan"]]
    assert len(getchans) == 2 and _kinds(lw)[-1][1] == K.MAPFN["tuplecat"]


def _enum(text, prefix):
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\b" + prefix + r"([A-Z0-9_]+)\s*=\s*(-?\d+)", text)}


def test_header_constants_match_the_python_mirror():
    h = open(os.path.join(ROOT, "include", "sigops.h")).read()
    assert _enum(h, "SO_MAP_")["EXPR"] == K.MAPFN["expr"] == 10
    assert _enum(h, "SO_RAMP_")["EXPR"] == K.RAMPFN["expr"] == 2
    assert {k.lower(): v for k, v in _enum(h, "SO_EOP_").items()} == K.EOP
    for prefix, table in (("SO_UN_", K.UN), ("SO_BIN_", K.BIN), ("SO_CMP_", K.CMP)):
        got = {k.lower(): v for k, v in _enum(h, prefix).items() if k != "COUNT"}
        assert got == table
        assert _enum(h, prefix)["COUNT"] == len(table)
    # ... and the device functions (csrc/kmath.h) are listed under the same ids
    km = open(os.path.join(ROOT, "signaloperators.jl_amd", "csrc", "kmath.h")).read()
    for lst, table in (("SO_UN_LIST", K.UN), ("SO_BIN_LIST", K.BIN), ("SO_CMP_LIST", K.CMP)):
        body = re.search(r"#define " + lst + r"\(X\)(.*?)\n(?!\s)", km, re.S).group(1)
        assert {n: int(i) for i, n in re.findall(r"X\((\d+), (\w+)\)", body)} == table


def test_math_header_compiles_with_hiprtc_without_a_device():
    """the text rtc.cpp puts in front of a source that calls kmath.h compiles for gfx950 (no device needed)"""
    km = open(os.path.join(ROOT, "signaloperators.jl_amd", "csrc", "kmath.h")).read()
    km = "\n".join(l for l in km.splitlines() if not l.startswith("#pragma once") and not l.startswith("#include"))
    calls = " + ".join([f"so_m_{n}(x)" for n in K.UN] + [f"so_m_{n}(x, y)" for n in K.BIN] + [f"so_c_{n}(x, y)" for n in K.CMP])
    body = km + r'''
extern "C" __global__ __launch_bounds__(256) void k_rtc(const DPiece* __restrict__ pieces, int npieces, const DLeaf* __restrict__ L, OutView out) {
    const long long n = threadIdx.x;
    const double x = leaf_load(L[0], n, 0), y = L[1].v0;
    so_store2(out, n, 0, so_select(x, ''' + calls + r''', y), 0.0, false);
}
'''
    log = C.create_string_buffer(8000)
    st = K.lib().so_rtc_compile_check(body.encode(), log, 8000)
    assert st == 0, log.value.decode()
