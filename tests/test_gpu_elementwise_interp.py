"""`np.interp` in `elementwise` closures on the device (include/sigops.h SO_EOP_INTERP; csrc/kmath.h so_interp): look-up
tables in maps, time functions, ramp shapes and channel maps, against `np.interp` on the operands bit for bit -- or the
host path (the same tree with the closure unmarked) where the engine computes the closure's argument itself.  Every tree
runs through the interpreter's math instantiation (SIGOPS_RTC=0) and through hipRTC (SIGOPS_RTC=1), bit for bit the same.
The tracer, and the NumPy restatement the device function is specified by, are tests/test_elementwise_interp_trace.py."""
import ctypes as C

import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import _capi as K
from sigops_amd import lowering as LW
from sigops_amd.engine import Plan
from oracle_bridge import oracle_sink, relerr
from test_elementwise_interp_trace import TABLES, interp_ref, nonfinite_table, planted, same_bits, table

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


def close(got, want, dt, what):
    assert got.shape == want.shape
    assert np.array_equal(np.isfinite(got), np.isfinite(want)) and np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    e = relerr(got[fin], want[fin]) if fin.any() else 0.0
    WORST[what] = max(WORST.get(what, 0.0), e)
    print(f"worst {what}: {WORST[what]:.3e}")
    assert e <= (1e-12 if dt == np.float64 else 1e-6), f"{what}: {e:.3e}"


def bit_equal(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got, want, equal_nan=True), f"{what}: {np.count_nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))} samples differ"
    assert same_bits(got, want), f"{what}: a zero of the other sign"


# ---- 1. maps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2, 3, 8])
@pytest.mark.parametrize("kind,n", TABLES, ids=[f"{k}{n}" for k, n in TABLES])
def test_maps_equal_numpy_bit_for_bit(kind, n, nch, monkeypatch):
    xp, fp = table(kind, n)
    frames = 4099 if nch == 3 else 30_000
    x = planted(np.random.default_rng(100 * n + nch), frames, nch, xp)
    sig = so.Signal(x, FS)
    got = both(so.OperateOn(so.elementwise(lambda a: np.interp(a, xp, fp)), sig), monkeypatch)
    bit_equal(got, np.interp(x, xp, fp), f"{kind} {n} x {nch}")
    assert same_bits(got, interp_ref(x, xp, fp))
    got = both(so.OperateOn(so.elementwise(lambda a: np.interp(a, xp, fp, left=-7.5, right=np.inf)), sig), monkeypatch)
    bit_equal(got, np.interp(x, xp, fp, left=-7.5, right=np.inf), f"{kind} {n} x {nch} left / right")


@pytest.mark.parametrize("kind,n", [("random", 1), ("random", 17), ("random", 1024), ("uniform", 65536)])
def test_float32_operands_give_numpys_float64(kind, n, monkeypatch):
    xp, fp = table(kind, n)
    x = planted(np.random.default_rng(100 * n + 2), 30_000, 2, xp, np.float32)
    assert (x == xp[-1]).any()  # (the tables' knots are exact in Float32: samples do sit on them)
    got = both(so.OperateOn(so.elementwise(lambda a: np.interp(a, xp, fp)), so.Signal(x, FS)), monkeypatch)
    assert got.dtype == np.float64
    bit_equal(got, np.interp(x, xp, fp), f"Float32 {kind} {n}")


# ---- 2. non-finite fp ------------------------------------------------------------------------------------------------
def test_non_finite_fp_takes_numpys_fall_backs(monkeypatch):
    xp, fp = nonfinite_table()
    x = planted(np.random.default_rng(77), 30_000, 2, xp)
    want, fb1, fb2 = interp_ref(x, xp, fp, paths=True)
    assert (fb1 & ~fb2).any() and fb2.any()  # at least one sample takes each fall-back
    got = both(so.OperateOn(so.elementwise(lambda a: np.interp(a, xp, fp)), so.Signal(x, FS)), monkeypatch)
    bit_equal(got, np.interp(x, xp, fp), "non-finite fp")
    assert same_bits(got, want)


# ---- 3. composition --------------------------------------------------------------------------------------------------
def test_composition_with_other_operations(monkeypatch):
    ta, tb = table("random", 17), table("random", 1024)
    rng = np.random.default_rng(31)
    x, y = planted(rng, 30_000, 2, ta[0]), planted(rng, 27_000, 2, tb[0])  # different lengths: zero padding
    ypad = np.vstack([y, np.zeros((3000, 2))])
    sigs = [so.Signal(x, FS), so.Signal(y, FS)]
    fn = lambda a, b: np.tanh(np.interp(a, *ta)) * b + np.interp(b, *tb)  # noqa: E731
    with np.errstate(all="ignore"):
        got = both(so.OperateOn(so.elementwise(fn), *sigs), monkeypatch)
        close(got, fn(x, ypad), np.float64, "tanh(interp) * y + interp")
        # only exact operations around the look-ups: bit-equal
        ex = lambda a, b: np.where(a > 0, np.interp(a, *ta), -np.interp(b, *tb)) * b - np.abs(np.interp(b, *ta))  # noqa: E731
        got = both(so.OperateOn(so.elementwise(ex), *sigs), monkeypatch)
        bit_equal(got, ex(x, ypad), "exact operations around look-ups")
    # a look-up of a look-up, and more tables than the interpreter's stack is deep
    tabs = [table("random", 17, seed=s) for s in range(5)]
    deep = lambda a: sum(np.interp(a * (k + 1), *t) for k, t in enumerate(tabs)) + np.interp(np.interp(a, *ta), *tb)  # noqa: E731
    got = both(so.OperateOn(so.elementwise(deep), sigs[0]), monkeypatch)
    with np.errstate(all="ignore"):
        close(got, deep(x), np.float64, "six tables")


# ---- 4. Signal(fn) ---------------------------------------------------------------------------------------------------
def test_envelopes_and_wavetables_match_the_host_path(monkeypatch):
    rng = np.random.default_rng(41)
    n = 30_000
    x = np.asfortranarray(rng.standard_normal((n, 2)))
    tp = np.asarray([0.0, 0.05, 0.3, 1.2, 2.5, 2.9])  # an ADSR over 3 s
    vp = np.asarray([0.0, 1.0, 0.6, 0.6, 0.1, 0.0])
    env = lambda t: np.interp(t, tp, vp)  # noqa: E731
    for kw in ({}, {"ω": 3 * so.Hz, "phase": 0.25}):
        got = both(so.Amplify(so.Signal(x, FS), so.Signal(so.elementwise(env), FS, **kw)) | so.Until(n * so.frames), monkeypatch)
        host = _sink(so.Amplify(so.Signal(x, FS), so.Signal(env, FS, **kw)) | so.Until(n * so.frames))
        bit_equal(got, host, f"envelope {kw}")
    e = both(so.Signal(so.elementwise(env), FS) | so.Until(n * so.frames), monkeypatch)
    assert e.max() == 1.0 and e[-1, 0] == 0.0 and np.count_nonzero(e == 0.6) > 8000  # the curve itself, not zeros
    # a single-cycle wavetable read with `period=`: the argument of Signal(fn, ω) is a phase in radians
    ph = np.linspace(0.0, 2 * np.pi, 64, endpoint=False)
    wt = np.sin(ph) + 0.3 * np.sin(3 * ph + 1.0)
    wave = lambda t: np.interp(t, ph, wt, period=2 * np.pi)  # noqa: E731
    # (the wave itself, not a constant: whole cycles span the fundamental's 2 less twice the harmonic's 0.3; the bare
    #  time argument runs over (0, 3] only, from >= 1 - 0.3 at pi/2 down to <= sin(3) + 0.3)
    for kw, span in (({"ω": 440 * so.Hz}, 1.4), ({}, 0.25)):
        got = both(so.Signal(so.elementwise(wave), FS, **kw) | so.Until(n * so.frames), monkeypatch)
        host = _sink(so.Signal(wave, FS, **kw) | so.Until(n * so.frames))
        bit_equal(got, host, f"wavetable {kw}")
        assert np.ptp(got) > span


# ---- 5. ramp shapes --------------------------------------------------------------------------------------------------
def _gain(n, R, direction, f):
    """the ramp's definition on the host (reference src/ramps.jl:60-72), as tests/test_gpu_elementwise.py has it"""
    i = np.arange(n, dtype=np.float64)
    g = np.ones(n)
    if direction == "on":
        m = i < R
        g[m] = f(i[m] / R)
    else:
        m = i >= n - R
        g[m] = f(1.0 - (i[m] + 1 - (n - R)) / R)
    return g.reshape(-1, 1)


def test_a_ramp_shape_given_as_a_table(monkeypatch):
    """(an unmarked closure in the ramp position has no host path -- it is refused --, so the host side of this
    comparison is the ramp's definition evaluated with NumPy, under the bound the existing ramp tests use for it)"""
    rng = np.random.default_rng(51)
    n, R = 30_000, 2500  # 0.25 s at 10 kHz
    x = np.asfortranarray(rng.standard_normal((n, 2)))
    up, uv = np.asarray([0.0, 0.1, 0.5, 0.9, 1.0]), np.asarray([0.5, 0.02, 0.5, 0.98, 0.75])  # f(1) != 1
    shape = lambda u: np.interp(u, up, uv)  # noqa: E731
    s = so.Signal(x, FS)
    got = both(so.RampOn(s, 0.25 * so.s, so.elementwise(shape)), monkeypatch)
    close(got, x * _gain(n, R, "on", shape), np.float64, "RampOn(table)")
    got = both(so.RampOff(s, 0.25 * so.s, so.elementwise(shape)), monkeypatch)
    close(got, x * _gain(n, R, "off", shape), np.float64, "RampOff(table)")
    got = both(so.Ramp(s, 0.25 * so.s, so.elementwise(shape)), monkeypatch)
    close(got, x * _gain(n, R, "on", shape) * _gain(n, R, "off", shape), np.float64, "Ramp(table)")
    assert np.array_equal(got[R:n - R], x[R:n - R]) and got[0, 0] == x[0, 0] * 0.5  # one outside the ramps, fp[0] at its start


# ---- 6. bychannel=False ----------------------------------------------------------------------------------------------
def test_a_different_table_per_output_channel(monkeypatch):
    tabs = [table("random", 3), table("random", 17), table("uniform", 1024)]
    x = planted(np.random.default_rng(61), 4099, 3, tabs[1][0])
    fn = lambda fr: (np.interp(fr[0], *tabs[0]), np.interp(fr[2], *tabs[1]), np.interp(fr[1], *tabs[2]), np.interp(fr[0], *tabs[1]))  # noqa: E731
    got = both(so.OperateOn(so.elementwise(fn), so.Signal(x, FS), bychannel=False), monkeypatch)
    want = np.stack([np.interp(x[:, 0], *tabs[0]), np.interp(x[:, 2], *tabs[1]), np.interp(x[:, 1], *tabs[2]), np.interp(x[:, 0], *tabs[1])], axis=1)
    bit_equal(got, np.asfortranarray(want), "a table per channel")


# ---- 7. a consumer behind it -----------------------------------------------------------------------------------------
def test_a_filter_and_a_resampler_behind_the_look_up(monkeypatch):
    xp, fp = table("random", 1024)
    x = np.asfortranarray(np.random.default_rng(71).standard_normal((30_000, 2)) * 2)
    curve = so.elementwise(lambda a: np.interp(a, xp, fp))
    tail = lambda t: t | so.Filt(so.Lowpass, 1 * so.kHz) | so.ToFramerate(12 * so.kHz)  # noqa: E731
    got = both(tail(so.Signal(x, FS) | so.Operate(curve)), monkeypatch)
    want = _sink(tail(so.Signal(np.asfortranarray(np.interp(x, xp, fp)), FS)))
    close(got, want, np.float64, "Filt | ToFramerate behind a look-up")
    want = oracle_sink(so.Signal(np.asfortranarray(np.interp(x, xp, fp)), FS) | so.Filt(so.Lowpass, 1 * so.kHz))
    close(_sink(so.Signal(x, FS) | so.Operate(curve) | so.Filt(so.Lowpass, 1 * so.kHz)), want, np.float64, "oracle")


# ---- 8. blocks and reuse ---------------------------------------------------------------------------------------------
def test_stream_blocks_equal_the_whole_sink():
    xp, fp = table("random", 1024)
    x = planted(np.random.default_rng(81), 30_000, 2, xp)
    tp, vp = np.asarray([0.0, 0.5, 2.0, 3.0]), np.asarray([0.0, 1.0, 0.25, 0.0])
    tree = so.Amplify(so.OperateOn(so.elementwise(lambda a: np.interp(a, xp, fp)), so.Signal(x, FS)),
                      so.Signal(so.elementwise(lambda t: np.interp(t, tp, vp)), FS)) | so.Until(30_000 * so.frames)
    one = _sink(tree)
    blocks = np.vstack([b for b, _ in so.stream(tree, 7000)])
    bit_equal(blocks, one, "stream")
    t = np.arange(1, 30_001) / 10_000.0
    bit_equal(one, np.asfortranarray(np.interp(x, xp, fp) * np.interp(t, tp, vp).reshape(-1, 1)), "stream against NumPy")


def test_a_plan_executed_twice_with_new_arrays(monkeypatch):
    xp, fp = table("uniform", 65536)
    rng = np.random.default_rng(82)
    xs = [planted(rng, 30_000, 2, xp) for _ in range(3)]
    for rtc in ("0", "1"):
        monkeypatch.setenv("SIGOPS_RTC", rtc)
        res = np.zeros((30_000, 2), order="F")
        p = Plan(so.OperateOn(so.elementwise(lambda a: np.interp(a, xp, fp)), so.Signal(xs[0], FS)), res.shape, res.dtype, (1, res.shape[0]), False)
        scratch = p.stats()["scratch_bytes"]
        assert scratch >= (3 + 2 * 65536) * 8  # the plan's own copy of the table is counted
        for k, x in enumerate(xs):
            if k:
                p.set_array(0, x)
            p.execute(res.ctypes.data)
            bit_equal(res, np.interp(x, xp, fp), f"execute {k}")
            s = p.stats()
            assert s["scratch_bytes"] == scratch and s["h2d_bytes"] == x.nbytes  # the leaf goes up per execute, the table never again
        p.close()


# ---- 9. device leaves, torch results ---------------------------------------------------------------------------------
def test_device_leaves_and_device_results(monkeypatch):
    import torch

    xp, fp = table("random", 1024)
    rng = np.random.default_rng(91)
    x, y = planted(rng, 30_000, 8, xp), planted(rng, 30_000, 8, xp)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t()  # noqa: E731
    fn = lambda a, b: np.interp(a, xp, fp) - np.interp(b, xp, fp, left=2.0)  # noqa: E731
    with np.errstate(all="ignore"):
        want = fn(x, y)
    got = both(so.OperateOn(so.elementwise(fn), so.Signal(dev(x), FS), so.Signal(dev(y), FS)), monkeypatch, to="torch")
    bit_equal(got, want, "device leaves")
    got = both(so.OperateOn(so.elementwise(fn), so.Signal(x, FS), so.Signal(y, FS)), monkeypatch, to="torch")
    bit_equal(got, want, "device result")


# ---- 10. malformed programs ------------------------------------------------------------------------------------------
def test_malformed_table_programs_are_refused():
    x = np.zeros((16, 1))
    lw = LW.lower(so.OperateOn(so.elementwise(lambda a: np.interp(a, [0.0, 1.0, 2.0], [1.0, 2.0, 4.0])), so.Signal(x, FS)))
    node = next(i for i in range(lw.n) if lw.nodes[i].kind == K.NODE_MAP)
    assert lw.nodes[node].s0 == 9
    out = K.so_out_desc_t(dtype=K.SO_F64, nch=1, nframes=16, frame_stride=1, chan_stride=16, is_device=0)
    arg, interp = K.EOP["arg"], K.EOP["interp"]
    good = [3.0, 1.0, 4.0, 0.0, 1.0, 2.0, 1.0, 2.0, 4.0]
    bad = [
        ([(interp, 0)], good, "stack underflow"),
        ([(arg, 0), (interp, 7)], good, "out of range"),              # the header itself past the constants
        ([(arg, 0), (interp, -1)], good, "out of range"),
        ([(arg, 0), (interp, 3)], good, "at least one knot"),         # (constants[3] = 0.0 read as a header: n = 0)
        ([(arg, 0), (interp, 0)], [0.0] + good[1:], "at least one knot"),
        ([(arg, 0), (interp, 0)], [4.0] + good[1:], "out of range"),  # more knots than constants
        ([(arg, 0), (interp, 0)], good[:3] + [2.0, 1.0, 0.0] + good[6:], "strictly increasing"),
        ([(arg, 0), (interp, 0)], good[:3] + [0.0, 1.0, 1.0] + good[6:], "strictly increasing"),
        ([(arg, 0), (interp, 0)], good[:3] + [0.0, np.nan, 2.0] + good[6:], "strictly increasing"),
    ]
    for prog, consts, word in bad:
        code = np.ascontiguousarray(np.asarray(prog, dtype=np.int32))
        cst = np.ascontiguousarray(np.asarray(consts, dtype=np.float64))
        lw.nodes[node].p0 = code.ctypes.data
        lw.nodes[node].i3 = len(prog)
        lw.nodes[node].p1 = cst.ctypes.data
        lw.nodes[node].s0 = cst.size
        plan = C.c_void_p()
        st = K.lib().so_plan_create(lw.nodes, lw.n, lw.root, C.byref(out), 0, C.byref(plan))
        assert st == -1 and not plan.value, (prog, consts)  # SO_ERR_INVALID, and no plan: nothing is launched
        assert f"node {node}" in K.last_error() and word in K.last_error(), K.last_error()
    # ... and without the length of the constants a table cannot be checked at all
    code = np.ascontiguousarray(np.asarray([(arg, 0), (interp, 0)], dtype=np.int32))
    cst = np.ascontiguousarray(np.asarray(good))
    lw.nodes[node].p0, lw.nodes[node].i3, lw.nodes[node].p1, lw.nodes[node].s0 = code.ctypes.data, 2, cst.ctypes.data, 0
    plan = C.c_void_p()
    assert K.lib().so_plan_create(lw.nodes, lw.n, lw.root, C.byref(out), 0, C.byref(plan)) == -1
    lw.nodes[node].s0 = 9  # the well-formed program, hand-built the same way, runs
    assert K.lib().so_plan_create(lw.nodes, lw.n, lw.root, C.byref(out), 0, C.byref(plan)) == 0
    res = np.full((16, 1), -1.0, order="F")
    assert K.lib().so_plan_execute(plan, C.c_void_p(res.ctypes.data), None) == 0
    K.lib().so_plan_destroy(plan)
    assert np.array_equal(res, np.ones((16, 1)))
