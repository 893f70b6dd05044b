"""`elementwise` closures on the device (include/sigops.h SO_MAP_EXPR / SO_RAMP_EXPR): maps, time functions, ramp shapes
and channel maps against the host path (the same tree with the closure unmarked), NumPy on the operands, or the oracle
with the closure's values supplied as data; the interpreter's math instantiation (SIGOPS_RTC=0) and the hipRTC kernel
(SIGOPS_RTC=1) bit for bit.  The tracer itself is tests/test_elementwise_trace.py."""
import ctypes as C

import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import _capi as K
from sigops_amd import lowering as LW
from sigops_amd.engine import Plan
from oracle_bridge import oracle_sink, relerr

pytestmark = pytest.mark.gpu
FS = 10 * so.kHz
WORST = {}  # (what) -> worst relative error seen (printed with -s)


def _sink(tree, to=so.Array):
    return so.sink(tree, to)


def both(tree, monkeypatch, to=so.Array):
    """the tree through the interpreter (SIGOPS_RTC=0) and through hipRTC (=1): bit for bit the same"""
    monkeypatch.setenv("SIGOPS_RTC", "0")
    a = _sink(tree, to)
    monkeypatch.setenv("SIGOPS_RTC", "1")
    b = _sink(tree, to)
    monkeypatch.delenv("SIGOPS_RTC")
    if to == "torch":
        a, b = a[0].cpu().numpy(), b[0].cpu().numpy()  # (tensor, frame rate)
    assert a.shape == b.shape and a.dtype == b.dtype
    assert np.array_equal(a, b, equal_nan=True), f"interpreter and hipRTC differ: {relerr(a, b):.3e}"
    return b


def steps(tree, res):
    p = Plan(so.ToChannels(tree, res.shape[1]), res.shape, res.dtype, (1, res.shape[0]), False)
    p.set_profiling(True)
    p.execute(res.ctypes.data)
    names = [s["name"] for s in p.steps()]
    p.close()
    return names


def close(got, want, dt, what):
    assert got.shape == want.shape
    assert np.array_equal(np.isfinite(got), np.isfinite(want)) and np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    e = relerr(got[fin], want[fin]) if fin.any() else 0.0
    WORST[what] = max(WORST.get(what, 0.0), e)
    print(f"worst {what}: {WORST[what]:.3e}")
    assert e <= (1e-12 if dt == np.float64 else 1e-6), f"{what}: {e:.3e}"


def arrays(rng, n, nch, dt):
    return np.asfortranarray(rng.standard_normal((n, nch)) * 2).astype(dt, order="F")


MAPS = [
    (lambda x: np.tanh(2.5 * x), 1),
    (lambda x, y: np.hypot(x, y), 2),
    (lambda x, y, z: np.where(z < 0.3, np.sqrt(x * x + y * y), np.tanh(z) - x) * 0.5, 3),
]


@pytest.mark.parametrize("nch", [1, 2, 8])
@pytest.mark.parametrize("k", range(len(MAPS)))
@pytest.mark.parametrize("dts", [(np.float64,), (np.float32,), (np.float32, np.float64)])
def test_maps_match_the_host_path(k, nch, dts, monkeypatch):
    fn, n = MAPS[k]
    rng = np.random.default_rng(10 * k + nch)
    xs = [arrays(rng, 30_000 - 3000 * j, nch, dts[j % len(dts)]) for j in range(n)]  # different lengths: zero padding
    sigs = [so.Signal(x, FS) for x in xs]
    got = both(so.OperateOn(so.elementwise(fn), *sigs), monkeypatch)
    want = _sink(so.OperateOn(fn, *sigs))
    assert got.dtype == want.dtype
    # (Float32 operands: the device rounds every Float32 operation, as NumPy and the reference do, while the host path
    #  hands the closure Python floats and rounds once at the end -- the Float32 bound applies)
    close(got, want, np.float32 if np.float32 in dts else np.float64, f"map {k} {'+'.join(np.dtype(d).name for d in dts)}")


def test_exact_operations_are_bit_equal(monkeypatch):
    """Float64: bit-equal to the host path.  Float32: bit-equal to NumPy's Float32 arithmetic on the operands (the host
    path evaluates a closure on Python floats, i.e. in Float64, and rounds once when it stores the result)"""
    rng = np.random.default_rng(3)
    fn = lambda a, b: np.where(a > b, np.maximum(a, 0.5) * b, np.abs(b) / 3 - np.minimum(a, b)) + (a <= -1)  # noqa: E731
    for dt in (np.float64, np.float32):
        x, y = arrays(rng, 20_000, 2, dt), arrays(rng, 20_000, 2, dt)
        sigs = [so.Signal(x, FS), so.Signal(y, FS)]
        got = both(so.OperateOn(so.elementwise(fn), *sigs), monkeypatch)
        assert got.dtype == dt and np.array_equal(got, fn(x, y))
        if dt == np.float64:
            assert np.array_equal(got, _sink(so.OperateOn(fn, *sigs)))


def test_device_leaves_and_device_results(monkeypatch):
    import torch

    rng = np.random.default_rng(4)
    x, y = arrays(rng, 50_000, 8, np.float64), arrays(rng, 50_000, 8, np.float64)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t()  # noqa: E731
    fn = lambda a, b: np.hypot(a, b) * np.tanh(a)  # noqa: E731
    got = both(so.OperateOn(so.elementwise(fn), so.Signal(dev(x), FS), so.Signal(dev(y), FS)), monkeypatch, to="torch")
    close(got, fn(x, y), np.float64, "device leaves")
    got = both(so.OperateOn(so.elementwise(fn), so.Signal(x, FS), so.Signal(y, FS)), monkeypatch, to="torch")
    close(got, fn(x, y), np.float64, "device result")


def test_time_functions(monkeypatch):
    rng = np.random.default_rng(5)
    x = arrays(rng, 40_000, 2, np.float64)
    f = lambda t: np.exp(-0.5 * t) * np.cos(3 * t)  # noqa: E731
    for kw in ({}, {"ω": 440 * so.Hz}, {"ω": 3 * so.Hz, "phase": 0.25}):
        env = both(so.Signal(so.elementwise(f), FS, **kw) | so.Until(40_000 * so.frames), monkeypatch)
        host = _sink(so.Signal(f, FS, **kw) | so.Until(40_000 * so.frames))
        close(env, host, np.float64, "Signal(f)")
        got = both(so.Amplify(so.Signal(x, FS), so.Signal(so.elementwise(f), FS, **kw)) | so.Until(40_000 * so.frames), monkeypatch)
        close(got, x * host, np.float64, "Amplify(x, Signal(f))")


def _gain(n, R, direction, f):
    i = np.arange(n, dtype=np.float64)
    g = np.ones(n)
    if direction == "on":
        m = i < R
        g[m] = f(i[m] / R)
    else:
        m = i >= n - R
        g[m] = f(1.0 - (i[m] + 1 - (n - R)) / R)
    return g.reshape(-1, 1)


def test_custom_ramps_are_one_outside_the_ramp(monkeypatch):
    rng = np.random.default_rng(6)
    n, R = 30_000, 2500  # 0.25 s at 10 kHz
    x = arrays(rng, n, 2, np.float64)
    f = lambda u: u ** 2 + 0.5  # noqa: E731  (f(1) != 1: the flat part must not be f(1))
    s = so.Signal(x, FS)
    got = both(so.RampOn(s, 0.25 * so.s, so.elementwise(f)), monkeypatch)
    close(got, x * _gain(n, R, "on", f), np.float64, "RampOn")
    got = both(so.RampOff(s, 0.25 * so.s, so.elementwise(f)), monkeypatch)
    close(got, x * _gain(n, R, "off", f), np.float64, "RampOff")
    got = both(so.Ramp(s, 0.25 * so.s, so.elementwise(f)), monkeypatch)
    close(got, x * _gain(n, R, "on", f) * _gain(n, R, "off", f), np.float64, "Ramp")
    got = both(so.Ramp(s, 0.25 * so.s, np.sqrt), monkeypatch)  # a bare ufunc in the ramp position
    close(got, x * _gain(n, R, "on", np.sqrt) * _gain(n, R, "off", np.sqrt), np.float64, "Ramp(sqrt)")
    y = arrays(rng, n, 2, np.float64)
    got = both(so.FadeTo(s, so.Signal(y, FS), 0.25 * so.s, so.elementwise(f)), monkeypatch)
    # Mix(RampOff(x), Prepend(RampOn(y), silence of n - R frames)): 2n - R frames, x zero-padded
    want = np.vstack([x * _gain(n, R, "off", f), np.zeros((n - R, 2))]) + np.vstack([np.zeros((n - R, 2)), y * _gain(n, R, "on", f)])
    close(got, want, np.float64, "FadeTo")


def test_channel_maps_are_bit_equal_to_the_host_path(monkeypatch):
    rng = np.random.default_rng(7)
    for dt in (np.float64, np.float32):
        x = arrays(rng, 25_000, 3, dt)
        for fn in (lambda fr: ((fr[0] + fr[1]) / 2, (fr[0] - fr[1]) / 2),
                   lambda fr: (fr[2], fr[0], fr[1]),
                   lambda fr: fr[0] * 0.5 + fr[2]):
            got = both(so.OperateOn(so.elementwise(fn), so.Signal(x, FS), bychannel=False), monkeypatch)
            want = _sink(so.OperateOn(fn, so.Signal(x, FS), bychannel=False))
            assert got.dtype == want.dtype and np.array_equal(got, want)


def test_closures_inside_larger_plans(monkeypatch):
    rng = np.random.default_rng(8)
    x = arrays(rng, 40_000, 2, np.float64)
    y = arrays(rng, 40_000, 2, np.float64)
    soft = lambda a: np.tanh(3 * a)  # noqa: E731
    m = lambda f: so.OperateOn(f, so.Signal(x, FS))  # noqa: E731
    for build in (lambda t: t | so.Filt(so.Lowpass, 1 * so.kHz),
                  lambda t: t | so.ToFramerate(12 * so.kHz),
                  lambda t: t | so.Normpower,
                  lambda t: so.Append(t | so.Until(20_000 * so.frames), so.Signal(y, FS)),
                  lambda t: t | so.After(1234 * so.frames) | so.Until(30_000 * so.frames)):
        got = both(build(m(so.elementwise(soft))), monkeypatch)
        want = _sink(build(m(soft)))
        close(got, want, np.float64, "inside plans")
    # the oracle, with the closure's values supplied as an array
    want = oracle_sink(so.Signal(np.asfortranarray(soft(x)), FS) | so.Filt(so.Lowpass, 1 * so.kHz))
    close(_sink(m(so.elementwise(soft)) | so.Filt(so.Lowpass, 1 * so.kHz)), want, np.float64, "oracle")


def test_streamed_equals_one_shot():
    rng = np.random.default_rng(9)
    x = arrays(rng, 48_000, 2, np.float64)
    f = so.elementwise(lambda a: np.tanh(3 * a) - 0.1 * a)
    tree = so.Amplify(so.OperateOn(f, so.Signal(x, FS)), so.Signal(so.elementwise(lambda t: np.exp(-t)), FS)) | so.Until(48_000 * so.frames)
    one = _sink(tree)
    blocks = np.vstack([b for b, _ in so.stream(tree, 7000)])
    assert np.array_equal(blocks, one)
    filt = _sink(tree | so.Filt(so.Lowpass, 1 * so.kHz))  # (a filter starts warm in every block: the stream's own bound)
    sfilt = np.vstack([b for b, _ in so.stream(tree | so.Filt(so.Lowpass, 1 * so.kHz), 7000)])
    assert relerr(sfilt, filt) < 1e-11


def test_block_stream_equals_one_shot():
    rng = np.random.default_rng(10)
    x = arrays(rng, 30_000, 2, np.float64)
    f = so.elementwise(lambda a: np.where(a > 0, np.sqrt(a), -np.log1p(-a)))
    bs = so.BlockStream(lambda s: so.OperateOn(f, s) | so.Amplify(0.5), FS, nch=2)
    outs = [bs.push(x[k:k + 4096]).cpu().numpy() for k in range(0, 30_000, 4096)]
    outs.append(bs.finish().cpu().numpy())
    got = np.concatenate(outs, axis=0)
    want = _sink(so.OperateOn(f, so.Signal(x, FS)) | so.Amplify(0.5))
    assert got.shape == want.shape and np.array_equal(got, want)


def test_non_finite_values(monkeypatch):
    rng = np.random.default_rng(11)
    x = arrays(rng, 20_000, 2, np.float64)
    x[::97, 0] = np.nan
    x[5::101, 1] = np.inf
    x[7::103, 1] = -np.inf
    x[::89, 0] = 0.0
    # (np.divide, not `1 / a`: the host path hands the closure Python floats, which raise on 1 / 0.0)
    for fn in (lambda a: np.log(a), lambda a: np.divide(1.0, a), lambda a: np.sqrt(a) + np.arctanh(a),
               lambda a: np.fmax(a, 0.0) * np.minimum(a, 1)):
        got = both(so.OperateOn(so.elementwise(fn), so.Signal(x, FS)), monkeypatch)
        want = _sink(so.OperateOn(fn, so.Signal(x, FS)))
        close(got, want, np.float64, "non-finite")


def test_steps_use_hiprtc_or_the_math_interpreter(monkeypatch):
    x = np.asfortranarray(np.random.default_rng(12).standard_normal((20_000, 2)))
    tree = so.OperateOn(so.elementwise(lambda a: np.tanh(a)), so.Signal(x, FS))
    res = np.zeros((20_000, 2), order="F")
    assert steps(tree, res) == ["k_pointwise_rtc"]  # compiled whenever hipRTC is allowed
    monkeypatch.setenv("SIGOPS_RTC", "0")
    assert steps(tree, res) == ["k_pointwise"]
    assert np.array_equal(res, np.tanh(x)) or relerr(res, np.tanh(x)) < 1e-14


def test_malformed_programs_are_refused():
    x = np.zeros((16, 1))
    lw = LW.lower(so.OperateOn(so.elementwise(lambda a: a * 2.0), so.Signal(x, FS)))
    node = next(i for i in range(lw.n) if lw.nodes[i].kind == K.NODE_MAP)
    out = K.so_out_desc_t(dtype=K.SO_F64, nch=1, nframes=16, frame_stride=1, chan_stride=16, is_device=0)
    bad = [
        [(K.EOP["arg"], 0), (K.EOP["bin"], K.BIN["mul"])],           # stack underflow
        [(K.EOP["arg"], 0), (K.EOP["arg"], 0)],                      # two values left
        [(K.EOP["arg"], 3)],                                         # argument out of range
        [(K.EOP["arg"], 0), (42, 0)],                                # unknown code
        [(K.EOP["arg"], 0), (K.EOP["un"], 99)],                      # unknown function
    ]
    for prog in bad:
        code = np.ascontiguousarray(np.asarray(prog, dtype=np.int32))
        lw.nodes[node].p0 = code.ctypes.data
        lw.nodes[node].i3 = len(prog)
        plan = C.c_void_p()
        st = K.lib().so_plan_create(lw.nodes, lw.n, lw.root, C.byref(out), 0, C.byref(plan))
        assert st == -1, prog  # SO_ERR_INVALID
        assert f"node {node}" in K.last_error()
