"""`Recur2(a1, a2, b)`, `Resonator` and `Sweep` above the C-ABI (signals.py, lowering.py): the NumPy definition the device is
held to (tests/recur2_ref.py) checked against its scalar restatement, against itself on every prefix, against the
sequential loop inside run 0 and against the extended-precision loop for accuracy; length, rate and channel algebra,
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
from recur_ref import recur_ref
from recur2_ref import (CH, EXTENDED, G, L, LENGTHS, T, W, coef, inf_example, kernel_constants, overflow_example, planted, recur2_loop,
                        recur2_loop_ext, recur2_ref, recur2_tree_loop, resonator_coefs, same_bits, signal, sweep_coefs, sweep_input, wide)

FS = 10 * so.kHz
CUTS = [L + 2, T - 1, T, T + 1, T + 2, CH - 1, CH, CH + 1, CH + 2, 2 * CH, 2 * CH + 3]


def _x(n=100, c=2, dtype=np.float64, fs=FS):
    return so.Signal(np.asfortranarray(np.arange(n * c, dtype=dtype).reshape(c, n).T), fs)


def _inputs(N, seed=0):
    """one channel of stable coefficients and samples"""
    a1, a2 = coef(("reson", "u1h")[seed % 2], N, 1, seed)
    return a1[:, 0], a2[:, 0], np.random.default_rng(100 * N + seed).standard_normal(N)


# ---- 1. the reference ------------------------------------------------------------------------------------------------
def test_the_constants_are_the_kernels():
    assert kernel_constants() == (L, G) and (L, W, T, G, CH) == (16, 64, 1024, 16, 16384)
    assert LENGTHS == [1, 2, 3, 15, 16, 17, 18, 1023, 1024, 1025, 1026, 16383, 16384, 16385, 16386, 2 * 16384 + 1, 3 * 16384 + 77]
    text = (Path(__file__).resolve().parent.parent / "signaloperators.jl_amd" / "csrc" / "k_recur2.hip").read_text()
    assert "kRecur2Waves = kCumsumTiles" in text and "kCumsumRun" in text  # the kernel takes the tree's constants from kernels.h


def test_the_block_form_equals_the_scalar_loops_bit_for_bit():
    for N in list(range(1, 301)) + CUTS:
        a1, a2, b = _inputs(N, N)
        assert same_bits(recur2_ref(a1, a2, b)[:, 0], recur2_tree_loop(a1, a2, b)), N
    for N in (T + L + 3, 2 * CH + 3):  # wide magnitudes, planted zeros, infinities and NaNs, in b and in the coefficients
        a1, a2 = coef("u1h", N, 3)
        for A1, A2, b in ((a1, a2, planted(wide(N, 3))), (planted(a1), a2, signal(N, 3)), (a1, planted(a2), signal(N, 3))):
            y = recur2_ref(A1, A2, b)
            with np.errstate(all="ignore"):
                for c in range(3):
                    assert same_bits(y[:, c], recur2_tree_loop(A1[:, c], A2[:, c], b[:, c])), (N, c)
    b32 = signal(CH + 77, 1, np.float32)
    a1, a2 = (v.astype(np.float32) for v in coef("reson", CH + 77, 1))
    assert same_bits(recur2_ref(a1, a2, b32)[:, 0], recur2_tree_loop(a1[:, 0].astype(np.float64), a2[:, 0].astype(np.float64), b32[:, 0].astype(np.float64)))


def test_a_prefix_does_not_depend_on_what_follows():
    N = 2 * CH + 3
    a1, a2 = coef("reson", N, 2)
    b = wide(N, 2)
    whole = recur2_ref(a1, a2, b)
    for n in [1, 2, 3, L - 1, L, L + 1] + CUTS:
        assert same_bits(recur2_ref(a1[:n], a2[:n], b[:n]), whole[:n]), n


def test_a_constant_gives_the_bits_of_a_row_of_it():
    for N in (L + 2, T + 5, CH + 2):
        b = wide(N, 3)
        for c1, c2 in ((1.9, -0.95), (0.0, 0.0), (-0.5, 0.25), (1.0, 0.0)):
            want = recur2_ref(c1, c2, b)
            assert same_bits(recur2_ref(np.full((N, 1), c1), np.full((N, 3), c2), b), want)
            assert same_bits(recur2_ref(c1, np.full((N, 1), c2), b), want)


def test_within_run_0_the_tree_is_the_loop():
    for seed in range(20):
        N = L + 5
        a1, a2, b = _inputs(N, seed)
        b = b * np.exp2(np.random.default_rng(seed).integers(-60, 61, N).astype(np.float64))
        b[seed % L] = (-0.0, 0.0)[seed % 2]
        assert same_bits(recur2_ref(a1, a2, b)[:L, 0], recur2_loop(a1, a2, b)[:L]), seed
    assert np.signbit(recur2_ref(0.5, 0.25, np.array([-0.0]))[0, 0])  # y[0] is the sample itself
    assert same_bits(recur2_ref(0.5, 0.25, np.array([-0.0, -0.0]))[:, 0], np.array([-0.0, 0.0]))  # (0.5 * -0 + 0.25 * +0) + -0 = +0


def test_with_a2_zero_the_frames_up_to_L_are_recurs():
    """The fact, pinned: with a2 = 0 and a1 >= 0 the frames [0, L] equal `recur_ref` bit for bit -- run 0 is the loop in both
    definitions, and frame L is a1 y[L-1] + b in both -- and from frame L + 1 on they are different roundings of the same
    value: Recur applies its composites to every frame, Recur2 walks the loop from the state that entered the run."""
    firsts = []
    for seed in range(3):
        rng = np.random.default_rng(77 + seed)
        N = 3 * T
        a, b = rng.uniform(0.0, 1.0, (N, 1)), rng.standard_normal((N, 1))
        y2, y1 = recur2_ref(a, 0.0, b)[:, 0], recur_ref(a, b)[:, 0]
        assert same_bits(y2[:L + 1], y1[:L + 1])
        assert np.max(np.abs(y2 - y1) / np.abs(y1)) < 1e-12
        firsts.append(int(np.argmin(y2 == y1)))
    assert firsts == [18, 20, 17]


def test_an_infinity_that_meets_a_zero_of_a_composite_is_nan():
    """the documented property: joins are general products, so where a product of coefficients has underflowed to zero an
    Inf in v gives NaN; the loop keeps the Inf"""
    a1, a2, b = inf_example()
    tree = recur2_ref(a1, a2, b)[:, 0]
    loop = recur2_loop(np.full(b.size, a1), np.full(b.size, a2), b)
    assert np.isfinite(loop[:3]).all() and (loop[3:] == np.inf).all()
    assert same_bits(tree[:2 * L], loop[:2 * L]) and np.isnan(tree[2 * L:]).all()
    with np.errstate(all="ignore"):
        assert same_bits(tree, recur2_tree_loop(np.full(b.size, a1), np.full(b.size, a2), b))


def test_unstable_coefficients_overflow_the_composites_where_a_loop_stays_finite():
    """the documented property: poles at 2 +- sqrt 3 over a tile; M passes 2^1024 in run 34, and Inf * 0 is NaN from
    frame T + 34 L on, where the loop's 4 * 0 - 0 + 0 stays 0"""
    a1, a2, b = overflow_example()
    tree = recur2_ref(a1, a2, b)[:, 0]
    loop = recur2_loop(np.full(b.size, a1), np.full(b.size, a2), b)
    first = T + 34 * L
    assert first == 1568 and not loop.any() and not tree[:first].any() and np.isnan(tree[first:]).all()
    with np.errstate(all="ignore"):
        assert same_bits(tree, recur2_tree_loop(np.full(b.size, a1), np.full(b.size, a2), b))


# ---- 2. accuracy: the tree and the loop against the extended-precision loop ----------------------------------------------
NA = 2 * CH + 1500


def _accuracy_inputs():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(NA)
    n = np.arange(NA)
    out = []
    for r in (0.9, 0.999, 0.99999):
        for th in (0.003, 0.3, 1.5, 3.1):
            out.append((f"resonator r={r} theta={th}", np.full(NA, 2.0 * r * math.cos(th)), np.full(NA, -(r * r)), x))
    for mod in ("constant", "sine", "noise"):
        for f in (4e-4, 0.05, 0.45):
            for q in (0.5, 0.707, 8):
                if mod == "constant":
                    fc = np.full(NA, f)
                elif mod == "sine":  # +-50 % over 5000 frames
                    fc = f * (1.0 + 0.5 * np.sin(2.0 * np.pi * n / 5000.0))
                else:  # +-50 %, a new value every frame
                    fc = f * (1.0 + 0.5 * rng.uniform(-1.0, 1.0, NA))
                fc = np.minimum(fc, 0.499)  # (below Nyquist)
                a1, a2, c0, c1, c2 = sweep_coefs("lowpass", fc, q, 1.0)
                out.append((f"lowpass {mod} fc/fs={f} q={q}", a1, a2, sweep_input(x, c0, c1, c2)[:, 0]))
    return out


ACCURACY = _accuracy_inputs()
# the input on which the sequential Float64 loop itself is not within 1e-8 of the extended-precision loop (it overflows:
# a cutoff that jumps between 0.22 fs and Nyquist every frame at q = 8 is not a stable system): outside the node's
# domain (DESIGN.md "Recur2"): the tree is not asked to beat the loop
OUTSIDE = {"lowpass noise fc/fs=0.45 q=8"}
_errors = {}


def _err(y, e):
    return float(np.sqrt(np.sum((y.astype(np.longdouble) - e) ** 2) / np.sum(e ** 2)))


def _measure(k):
    if k not in _errors:
        name, a1, a2, b = ACCURACY[k]
        with np.errstate(all="ignore"):
            e = recur2_loop_ext(a1, a2, b)
            _errors[k] = (_err(recur2_ref(a1, a2, b)[:, 0], e), _err(recur2_loop(a1, a2, b), e))
    return _errors[k]


def test_the_yardstick_is_extended_precision():
    assert EXTENDED  # np.longdouble is the x87 80-bit type here: 11 more bits than the tree and the loop under test


@pytest.mark.parametrize("k", range(len(ACCURACY)), ids=[a[0] for a in ACCURACY])
def test_the_loop_stays_within_the_contract_on_every_listed_input(k):
    tree, loop = _measure(k)
    print(f"{ACCURACY[k][0]}: loop {loop:.3e}")
    if ACCURACY[k][0] in OUTSIDE:
        assert not loop <= 1e-8
    else:
        assert loop <= 1e-8


@pytest.mark.parametrize("k", [k for k in range(len(ACCURACY)) if ACCURACY[k][0] not in OUTSIDE], ids=[a[0] for a in ACCURACY if a[0] not in OUTSIDE])
def test_the_tree_stays_within_the_contract(k):
    """Norm-wise relative error against the extended-precision loop, N = 2 CH + 1500: <= 1e-8, the project's Float64
    contract.  Measured: all 38 inputs hold; the worst are the low-pass fc / fs = 4e-4, q = 8 (7.9e-10, the loop 1.6e-12:
    the worst ratio, 506) and the resonator r = 0.99999, theta = 0.003 (3.9e-10, the loop 4.5e-12); most lie at 1e-16 ..
    1e-12.  With the joins in plain Float64 those two were at 1.4e-8 and 4.6e-8: the reason the definition carries the
    joins' entries as double-doubles (DESIGN.md "Recur2", accuracy)."""
    tree, loop = _measure(k)
    print(f"{ACCURACY[k][0]}: tree {tree:.3e} loop {loop:.3e} ratio {tree / loop:.1f}")
    assert tree <= 1e-8


# ---- 3. the wrappers against their formulas ------------------------------------------------------------------------------
def _fields(y):
    assert isinstance(y, so.Recur2Signal) and y.evaltrait == "computed"
    return y.a1, y.a2, y.coefs, y.signal


def _number(k):
    while isinstance(k, so.MapSignal):  # (`Uniform` spreads the number over the channels of x)
        assert len(k.signals) == 1
        k = k.signals[0]
    assert isinstance(k, so.NumberSig) and k.dtype == np.float64 and not k.dB
    return k.val


def test_resonator_and_sweep_with_numbers_are_their_formulas_on_the_host():
    x = _x(100, 2, np.float32, fs=44.1 * so.kHz)
    a1, a2, coefs, b = _fields(so.Resonator(x, 440 * so.Hz, 20 * so.Hz))
    w1, w2, g = resonator_coefs(440.0, 20.0, 44_100.0)
    r, th = math.exp(-math.pi * 20.0 / 44_100.0), 2.0 * math.pi * 440.0 / 44_100.0
    assert (w1, w2, g) == (2.0 * r * math.cos(th), -(r * r), (1.0 - r * r) * math.sin(th))
    assert (a1, a2, coefs) == (w1, w2, None) and isinstance(b, so.MapSignal) and b.fn == so.signals.MUL
    assert b.signals[0] is x and _number(b.signals[1]) == g
    assert so.Resonator(x, 440.0, 20.0).a1 == w1  # bare numbers are Hz
    for kind, name in ((so.Lowpass, "lowpass"), (so.Highpass, "highpass"), (so.Bandpass, "bandpass")):
        a1, a2, coefs, b = _fields(so.Sweep(x, kind, 1 * so.kHz, 2.0))
        w1, w2, c0, c1, c2 = sweep_coefs(name, 1000.0, 2.0, 44_100.0)
        assert (a1, a2, coefs) == (w1, w2, None) and isinstance(b, so.MapSignal) and isinstance(b.fn, so.signals.ExprFn)
        taps = np.array([[3.0], [5.0], [7.0]])
        assert float(np.asarray(b.fn.fn(*taps)).ravel()[0]) == (c0 * 3.0 + c1 * 5.0) + c2 * 7.0
        assert b.signals[0] is x and all(so.nframes(t) == 100 for t in b.signals)
    w = 2.0 * math.pi * 1000.0 / 44_100.0
    alpha = math.sin(w) / (2.0 * math.sqrt(0.5))
    assert so.Sweep(x, so.Lowpass, 1 * so.kHz).a1 == 2.0 * math.cos(w) / (1.0 + alpha)  # q = sqrt(1/2) by default
    assert so.Sweep(x, so.Lowpass, 1 * so.kHz).a2 == -(1.0 - alpha) / (1.0 + alpha)
    # the values: unit gain at DC for the low-pass, none for the high-pass and the band-pass; about one at fc for the resonator
    step = np.ones((6000, 1))
    for name, dc in (("lowpass", 1.0), ("highpass", 0.0), ("bandpass", 0.0)):
        a1, a2, c0, c1, c2 = sweep_coefs(name, 300.0, 0.707, 10_000.0)
        assert abs(recur2_ref(a1, a2, sweep_input(step, c0, c1, c2))[-1, 0] - dc) < 1e-9
    a1, a2, g = resonator_coefs(500.0, 5.0, 10_000.0)
    tone = np.sin(2.0 * np.pi * 500.0 / 10_000.0 * np.arange(40_000))[:, None]
    assert abs(np.abs(recur2_ref(a1, a2, g * tone)[-2000:]).max() - 1.0) < 0.01


def test_signal_arguments_build_traced_maps():
    x = _x(100, 2, fs=FS)
    fc = so.Signal(np.full((100, 1), 300.0, dtype=np.float32), FS)
    q = so.Signal(np.full((100, 1), 2.0), FS)
    for y, want in ((so.Resonator(x, fc, 20 * so.Hz), resonator_coefs(300.0, 20.0, 10_000.0)[:2]),
                    (so.Resonator(x, 300 * so.Hz, so.Signal(np.full((100, 1), 20.0), FS)), resonator_coefs(300.0, 20.0, 10_000.0)[:2]),
                    (so.Sweep(x, so.Lowpass, fc, 2.0), sweep_coefs("lowpass", 300.0, 2.0, 10_000.0)[:2]),
                    (so.Sweep(x, so.Bandpass, 300.0, q), sweep_coefs("bandpass", 300.0, 2.0, 10_000.0)[:2]),
                    (so.Sweep(x, so.Highpass, fc, q), sweep_coefs("highpass", 300.0, 2.0, 10_000.0)[:2])):
        a1, a2, coefs, b = _fields(y)
        assert a1 is None and a2 is None and y.children == (coefs[0], coefs[1], b)
        for c, w in zip(coefs, want):
            assert isinstance(c, so.MapSignal) and isinstance(c.fn, so.signals.ExprFn) and c.nch == 1 and c.dtype == np.float64
            args = [np.array([float(s.signals[0].data.ravel()[0]) if isinstance(s, so.MapSignal) else float(s.data.ravel()[0])]) for s in c.signals]
            assert abs(float(np.asarray(c.fn.fn(*args)).ravel()[0]) - w) < 1e-15
        assert so.nframes(b) == 100 and b.nch == 2 and so.nframes(y) == 100
    inf = so.Signal(np.sin, FS, ω=2 * so.Hz)  # an infinite control signal: the node keeps the length of x
    y = so.Sweep(x, so.Lowpass, so.OperateOn(so.elementwise(lambda v: 500.0 + 100.0 * v), inf))
    assert so.nframes(y) == 100 and so.signals.isknowninf(so.nframes(y.coefs[0]))


# ---- 4. algebra ------------------------------------------------------------------------------------------------------
def test_length_rate_channels_and_type():
    b = _x(100, 3, np.float32, fs=44.1 * so.kHz)
    y = so.Recur2(0.5, -0.25, b)
    assert isinstance(y, so.Recur2Signal) and y.signal is b and y.children == (b,) and (y.a1, y.a2, y.coefs) == (0.5, -0.25, None)
    assert so.nframes(y) == 100 and so.nchannels(y) == 3 and so.framerate(y) == 44_100.0
    assert so.sampletype(y) == np.float64 and so.duration(y) == 100 / 44_100.0
    c1 = so.Signal(np.full((150, 1), 0.5, dtype=np.float32), 44.1 * so.kHz)  # one channel, longer than b
    c3 = so.Signal(np.full((100, 3), -0.25), 44.1 * so.kHz)
    y = so.Recur2(c1, c3, b)
    assert y.coefs == (c1, c3) and y.a1 is None and y.children == (c1, c3, b) and so.nframes(y) == 100 and y.nch == 3
    y = so.Recur2(c1, -0.25, b)  # a number next to a signal: a row of it
    assert y.coefs[0] is c1 and isinstance(y.coefs[1], so.NumberSig) and y.coefs[1].val == -0.25 and y.coefs[1].fs == 44_100.0
    y = so.Recur2(0.5, c3, b)
    assert isinstance(y.coefs[0], so.NumberSig) and y.coefs[0].val == 0.5 and y.coefs[1] is c3
    ainf = so.Signal(np.sin, 44.1 * so.kHz, ω=5 * so.Hz)  # infinite
    assert so.nframes(so.Recur2(ainf, c3, b)) == 100
    norate = so.Signal(np.full((100, 1), 0.5))
    y = so.Recur2(norate, c3, b)
    assert y.coefs[0].fs == 44_100.0  # a coefficient without a rate takes the others'
    y = so.Recur2(c1, norate, _x(100, 3, fs=None))
    assert y.signal.fs == 44_100.0 and y.coefs[1].fs == 44_100.0 and y.fs == 44_100.0  # b without a rate takes a1's
    assert so.Recur2(0.5, 0.1, _x(fs=None)).fs is None and so.Recur2(norate, 0.1, _x(fs=None)).fs is None
    assert so.nframes(so.Recur2(0.5, 0.1, b | so.Filt(so.Lowpass, 1 * so.kHz))) == 100  # a computed child


def test_currying_and_piping():
    x = _x()
    y = x | so.Recur2(0.5, -0.25)
    assert isinstance(y, so.Recur2Signal) and y.signal is x and (y.a1, y.a2) == (0.5, -0.25)
    z = np.zeros((100, 2)) | so.Recur2(0.5, -0.25)  # a bare array on the left
    assert isinstance(z, so.Recur2Signal) and z.nch == 2
    assert so.nframes(so.pipe(x, so.Recur2(0.5, 0.1), so.Recur2(0.25, 0.1), so.Until(10 * so.frames))) == 10
    for made in (x | so.Resonator(1 * so.kHz, 50 * so.Hz), x | so.Sweep(so.Lowpass, 1 * so.kHz), x | so.Sweep(so.Bandpass, 1 * so.kHz, q=4.0)):
        assert isinstance(made, so.Recur2Signal) and so.nframes(made) == 100 and made.nch == 2
    assert (x | so.Sweep(so.Highpass, 1 * so.kHz, q=4.0)).a1 == so.Sweep(x, so.Highpass, 1 * so.kHz, 4.0).a1 == so.Sweep(x, so.Highpass, 1 * so.kHz, q=4.0).a1
    assert (x | so.Resonator(1 * so.kHz, 50 * so.Hz)).a2 == so.Resonator(x, 1 * so.kHz, 50 * so.Hz).a2


def test_toframerate():
    y = so.Recur2(so.Signal(np.full((100, 1), 0.5)), -0.25, _x(fs=None))  # no rate: it is handed to every input
    z = so.ToFramerate(y, 8 * so.kHz)
    assert isinstance(z, so.Recur2Signal) and z.fs == 8000.0 and z.signal.fs == 8000.0 and so.nframes(z) == 100
    assert z.coefs[0].fs == 8000.0 and z.coefs[1].fs == 8000.0 and z.coefs[1].val == -0.25
    z = so.ToFramerate(so.Recur2(0.5, -0.25, _x(fs=None)), 8 * so.kHz)
    assert isinstance(z, so.Recur2Signal) and (z.a1, z.a2, z.fs, z.signal.fs) == (0.5, -0.25, 8000.0, 8000.0)
    y = so.Recur2(0.5, -0.25, _x())  # a rate: resampled like any computed signal
    z = so.ToFramerate(y, 20 * so.kHz)
    assert isinstance(z, so.FilteredSignal) and isinstance(z.fn, so.ResamplerFn) and z.signal is y
    assert z.fs == 20_000.0 and so.nframes(z) == 200
    assert so.ToFramerate(y, FS) is y


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_name_the_construct():
    x = _x()
    sine = so.Signal(np.sin, FS, ω=5 * so.Hz)
    short = so.Signal(np.full((50, 1), 0.5), FS)
    ok = so.Signal(np.full((100, 1), 0.5), FS)
    hz = so.Signal(np.full((100, 1), 300.0), FS)
    cases = [
        (lambda: so.Recur2(0.5, 0.1, sine), "Recur2", "use `Until`"),
        (lambda: sine | so.Recur2(0.5, 0.1), "Recur2", "use `Until`"),
        (lambda: so.Recur2(0.5, 0.1, so.Signal(np.zeros(10)) | so.Filt(so.Lowpass, 1 * so.kHz)), "Recur2", "use `Until`"),  # unknown: no rate
        (lambda: so.Resonator(sine, 1 * so.kHz, 10 * so.Hz), "Resonator", "use `Until`"),
        (lambda: so.Sweep(sine, so.Lowpass, 1 * so.kHz), "Sweep", "use `Until`"),
        (lambda: so.Sweep(sine, so.Lowpass, hz), "Sweep", "use `Until`"),
        (lambda: so.Recur2(0.5, 0.1, so.Signal(np.arange(10), FS)), "Recur2", "Float32 or Float64"),
        (lambda: so.Recur2(so.Signal(np.arange(100), FS), 0.1, x), "Recur2", "Float32 or Float64"),
        (lambda: so.Recur2(0.5, so.Signal(np.arange(100), FS), x), "Recur2", "Float32 or Float64"),
        (lambda: so.Resonator(so.Signal(np.arange(10), FS), 1 * so.kHz, 10 * so.Hz), "Resonator", "Float32 or Float64"),
        (lambda: so.Sweep(so.Signal(np.arange(10), FS), so.Lowpass, 1 * so.kHz), "Sweep", "Float32 or Float64"),
        (lambda: so.Sweep(x, so.Lowpass, so.Signal(np.arange(100), FS)), "Sweep", "Float32 or Float64"),
        (lambda: so.Recur2(short, 0.1, x), "Recur2", "at least as long as b"),
        (lambda: so.Recur2(ok, short, x), "Recur2", "at least as long as b"),
        (lambda: so.Resonator(x, so.Signal(np.full((50, 1), 300.0), FS), 10.0), "Resonator", "at least as long as b"),
        (lambda: so.Sweep(x, so.Lowpass, 300.0, so.Signal(np.full((50, 1), 2.0), FS)), "Sweep", "at least as long as b"),
        (lambda: so.Recur2(so.Signal(np.full((100, 3), 0.5), FS), 0.1, x), "Recur2", "a1 has 3 channels; 1 or b's 2"),
        (lambda: so.Recur2(0.5, so.Signal(np.full((100, 3), 0.5), FS), x), "Recur2", "a2 has 3 channels; 1 or b's 2"),
        (lambda: so.Sweep(x, so.Lowpass, so.Signal(np.full((100, 3), 300.0), FS)), "Sweep", "3 channels; 1 or x's 2"),
        (lambda: so.Recur2(so.Signal(np.full((100, 1), 0.5), 8 * so.kHz), 0.1, x), "Recur2", "use `ToFramerate`"),
        (lambda: so.Recur2(ok, so.Signal(np.full((100, 1), 0.5), 8 * so.kHz), _x(fs=None)), "Recur2", "use `ToFramerate`"),
        (lambda: so.Resonator(x, so.Signal(np.full((100, 1), 300.0), 8 * so.kHz), 10.0), "Resonator", "use `ToFramerate`"),
        (lambda: so.Sweep(x, so.Lowpass, 300.0, so.Signal(np.full((100, 1), 2.0), 8 * so.kHz)), "Sweep", "use `ToFramerate`"),
        (lambda: so.Recur2(math.inf, 0.1, x), "Recur2", "finite number"),
        (lambda: so.Recur2(0.5, math.nan, x), "Recur2", "finite number"),
        (lambda: so.Recur2("half", 0.1, x), "Recur2", "a number or a signal"),
        (lambda: so.Recur2(0.5, 1 * so.Hz, x), "Recur2", "a number or a signal"),
        (lambda: so.Resonator(_x(fs=None), 1 * so.kHz, 10 * so.Hz), "Resonator", "needs the frame rate of x"),
        (lambda: so.Resonator(_x(fs=None), so.Signal(np.full((100, 1), 300.0)), 10.0), "Resonator", "needs the frame rate of x"),
        (lambda: so.Sweep(_x(fs=None), so.Lowpass, 1 * so.kHz), "Sweep", "needs the frame rate of x"),
        (lambda: so.Resonator(x, -1 * so.Hz, 10 * so.Hz), "Resonator", "fc must be a finite frequency >= 0"),
        (lambda: so.Resonator(x, 1 * so.kHz, -10 * so.Hz), "Resonator", "bw must be a finite frequency >= 0"),
        (lambda: so.Resonator(x, math.inf, 10.0), "Resonator", ">= 0"),
        (lambda: so.Resonator(x, 1 * so.ms, 10.0), "Resonator", "not a frequency"),
        (lambda: so.Sweep(x, so.Lowpass, -1 * so.Hz), "Sweep", "fc must be a finite frequency >= 0"),
        (lambda: so.Sweep(x, so.Lowpass, 1 * so.kHz, 0.0), "Sweep", "q must be a finite number > 0"),
        (lambda: so.Sweep(x, so.Lowpass, 1 * so.kHz, q=-2.0), "Sweep", "q must be a finite number > 0"),
        (lambda: so.Sweep(x, so.Lowpass, 1 * so.kHz, q=math.nan), "Sweep", "q must be a finite number > 0"),
        (lambda: so.Sweep(x, so.Lowpass, 1 * so.kHz, q=2 * so.Hz), "Sweep", "q is a plain number"),
        (lambda: so.Sweep(x, so.Bandstop, 1 * so.kHz), "Sweep", "Lowpass, Highpass or Bandpass"),
        (lambda: engine._streamable(so.Recur2(0.5, 0.1, x) | so.Filt(so.Lowpass, 1 * so.kHz)), "BlockStream: Recur2", "not streamable"),
        (lambda: engine._streamable(so.Mix(so.Sweep(x, so.Lowpass, 1 * so.kHz), 1.0)), "BlockStream: Recur2", "not streamable"),
        (lambda: sharding.shard_time(so.Recur2(0.5, 0.1, x), 0, 2), "Recur2", "Recur2 / Resonator / Sweep over several GPUs is not built"),
        (lambda: sharding.shard_channels(so.Mix(so.Resonator(x, 1 * so.kHz, 10.0), 1.0), 0, 2), "Recur2", "over several GPUs is not built"),
        (lambda: sharding.shard_append(so.Append(so.Resonator(x, hz, 10.0), x), 0, 2), "Recur2", "over several GPUs is not built"),
    ]
    for make, name, words in cases:
        with pytest.raises(so.ErrorException) as e:
            make()
        assert name in str(e.value) and "Recur2" in str(e.value) and words in str(e.value), str(e.value)
    assert (so.Recur2Signal, "Recur2 / Resonator / Sweep") in sharding._FROM_FRAME_0


# ---- 6. the lowered node ---------------------------------------------------------------------------------------------
def test_the_lowered_node_in_both_forms():
    assert K.NODE_RECUR2 == 18 and K.NODE_RECUR == 17
    text = (Path(__file__).resolve().parent.parent / "include" / "sigops.h").read_text()
    assert re.search(r"SO_NODE_RECUR2 = 18\b", text) and re.search(r"SO_NODE_RECUR = 17,", text)
    assert re.search(r"\*  RECUR2 +one child: child 0 = b, d0 = the constant a1, d1 = the constant a2", text)
    b = _x(100, 2, np.float32)
    lw = LW.lower(so.Recur2(0.75, -0.5, b))
    nd = lw.nodes[lw.root]
    assert nd.kind == K.NODE_RECUR2 and nd.n_children == 1 and nd.nch == 2 and nd.dtype == K.SO_F64 and nd.nframes == 100 and nd.fs == 10_000.0
    cb = lw.nodes[nd.children[0]]
    assert cb.kind == K.NODE_ARRAY and cb.l0 == 100 and cb.dtype == K.SO_F32 and cb.nch == 2
    assert (nd.d0, nd.d1) == (0.75, -0.5)
    assert (nd.i0, nd.i1, nd.i2, nd.i3, nd.l0, nd.l1, nd.s0, nd.s1, nd.d2, nd.d3) == (0,) * 10 and not nd.p0 and not nd.p1
    a1 = so.Signal(np.full((150, 1), 0.5), FS)
    a2 = so.Signal(np.full((100, 2), -0.25, dtype=np.float32), FS)
    lw = LW.lower(so.Recur2(a1, a2, b))
    nd = lw.nodes[lw.root]
    assert nd.kind == K.NODE_RECUR2 and nd.n_children == 3 and nd.nch == 2 and nd.dtype == K.SO_F64 and nd.nframes == 100
    c1, c2, cb = (lw.nodes[nd.children[k]] for k in range(3))
    assert c1.kind == K.NODE_ARRAY and c1.l0 == 150 and c1.dtype == K.SO_F64 and c1.nch == 1
    assert c2.kind == K.NODE_ARRAY and c2.l0 == 100 and c2.dtype == K.SO_F32 and c2.nch == 2
    assert cb.kind == K.NODE_ARRAY and cb.l0 == 100 and cb.dtype == K.SO_F32 and cb.nch == 2
    assert (nd.d0, nd.d1, nd.i0) == (0.0, 0.0, 0)
    lw = LW.lower(so.Recur2(a1, -0.25, b))  # a number next to a signal: a CONST child
    nd = lw.nodes[lw.root]
    assert nd.n_children == 3 and lw.nodes[nd.children[1]].kind == K.NODE_CONST and lw.nodes[nd.children[1]].d0 == -0.25


def test_demand_sizes_all_three_children_from_frame_0():
    a1, a2, b = so.Signal(np.full((150, 1), 0.5), FS), so.Signal(np.full((100, 2), 0.1), FS), _x(100, 2)
    tree = so.Recur2(a1, a2, b)
    need = {}
    LW._demand(tree | so.Until(10 * so.frames), 10, need)
    assert need[id(a1)] == (10, 0) and need[id(a2)] == (10, 0) and need[id(b)] == (10, 0)
    need = {}
    LW._demand(tree | so.After(5 * so.frames) | so.Until(10 * so.frames), 10, need)
    assert need[id(a1)] == (15, 0) and need[id(a2)] == (15, 0) and need[id(b)] == (15, 0)  # the skipped frames are computed too
    need = {}
    LW._demand(so.Recur2(0.5, 0.1, b) | so.After(5 * so.frames), 95, need)
    assert need[id(b)] == (100, 0)
