"""`Comb(x, d, g)` / `Allpass(x, d, g)` above the C-ABI (signals.py, lowering.py): the NumPy definition the device is held
to (tests/comb_ref.py) checked against its scalar restatement, closed forms and `scipy.signal.lfilter`; length, rate and
channel algebra, currying, the forms of a delay, the `ToFramerate` rules, every refusal and the lowered node.  No GPU
needed."""
import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import _capi as K
from sigops_amd import engine, sharding
from sigops_amd import lowering as LW
from comb_ref import FORMS, allpass, comb, comb_loop, comb_ref, planted, same_bits, signal, unroll

FS = 10 * so.kHz


def _x(n=100, c=2, dtype=np.float64, fs=FS):
    return so.Signal(np.asfortranarray(np.arange(n * c, dtype=dtype).reshape(c, n).T), fs)


# ---- 1. the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 7, 64, 65])
def test_the_block_form_equals_the_scalar_loop_bit_for_bit(D):
    for N in (1, D, D + 1, 5 * D + 3):
        for name, b0, bD, a in FORMS + [("overflow", 1.0, 0.0, 1e30)]:
            for x in (signal(N, 2), planted(N, 2, D), signal(N, 1, np.float32)):
                assert same_bits(comb_ref(x, D, b0, bD, a), comb_loop(x, D, b0, bD, a)), (D, N, name)


def test_an_impulse_through_the_comb_and_the_allpass():
    D, g, N = 7, 0.6, 7 * 12 + 3
    x = np.zeros((N, 1))
    x[0] = 1.0
    y = comb(x, D, g)[:, 0]
    k = np.arange(1, N // D + 1)
    assert y[0] == 1.0 and np.array_equal(y[k * D], np.cumprod(np.full(k.size, g)))  # y[kD] == cumprod(g)[k-1], exactly
    rest = np.ones(N, bool)
    rest[::D] = False
    assert not y[rest].any() and not np.signbit(y[rest]).any()
    h = allpass(x, D, g)[:, 0]
    assert h[0] == -g and h[D] == 1.0 + g * (-g)
    for j in range(2, N // D + 1):
        assert h[j * D] == g * h[(j - 1) * D]  # g times the previous value
    assert not h[rest].any()


def test_the_omitted_term_keeps_zero_times_inf_out_of_a_plain_comb():
    D = 5
    x = np.ones((4 * D, 1))
    x[2] = np.inf
    y = comb(x, D, 0.5)[:, 0]  # bD == 0: the Inf of x is never multiplied by it
    assert np.isinf(y[2::D]).all() and not np.isnan(y).any() and np.isfinite(np.delete(y, np.arange(2, 4 * D, D))).all()
    z = comb_ref(x, D, 1.0, 1e-300, 0.5)[:, 0]  # a feed-forward term, however small, is applied
    assert np.isinf(z[2::D]).all() and not np.isnan(z).any()
    assert not np.isnan(comb_ref(-x, D, 1.0, 1.0, 0.5)).any()  # (-Inf) + (-Inf): still no NaN
    assert np.isnan(comb_ref(x, D, 1.0, -1.0, 1.0)[2 + D, 0])  # 1 - Inf + Inf: the NaN a sequential loop gives


# ---- 2. an independent check: scipy.signal.lfilter over the dense b and a ----------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 63, 64, 65, 257, 1000])
def test_against_lfilter(D):
    from scipy.signal import lfilter

    x = np.random.default_rng(D).standard_normal(20_000)
    worst = 0.0
    for name, b0, bD, a in [("comb", 1.0, 0.0, 0.95), ("comb -", 1.0, 0.0, -0.95), ("allpass", -0.7, 1.0, 0.7), ("three", 0.9, -0.35, 0.5), ("fir", 0.8, 0.45, 0.0)]:
        b = np.zeros(D + 1)
        b[0] += b0
        b[D] += bD
        den = np.zeros(D + 1)
        den[0] = 1.0
        den[D] = -a
        want = lfilter(b, den, x)
        got = comb_ref(x.reshape(-1, 1), D, b0, bD, a)[:, 0]
        # three roundings per step times the loop gain 1 / (1 - |a|) <= 20: about 7e-15 norm-wise
        e = np.linalg.norm(got - want) / np.linalg.norm(want)
        worst = max(worst, e)
        assert e <= 1e-13, (name, e)
        if bD == 0.0:  # the plain comb: the same operations in the same order
            assert np.array_equal(got, want), name
    print(f"D={D}: worst norm-wise difference to lfilter {worst:.2e}")


# ---- 3. algebra ------------------------------------------------------------------------------------------------------
def test_length_rate_channels_and_type():
    x = _x(100, 3, np.float32, fs=44.1 * so.kHz)
    y = so.Comb(x, 7, 0.5)
    assert isinstance(y, so.CombSignal) and y.evaltrait == "computed" and y.signal is x
    assert so.nframes(y) == 100 and so.nchannels(y) == 3 and so.framerate(y) == 44_100.0
    assert so.sampletype(y) == np.float64 and so.duration(y) == 100 / 44_100.0
    assert (y.delay, y.b0, y.bD, y.a) == (7, 1.0, 0.0, 0.5)
    z = so.Comb(x, 7, 0.5, feedforward=0.25, direct=-2.0)
    assert (z.b0, z.bD, z.a) == (-2.0, 0.25, 0.5)
    ap = so.Allpass(x, 9, 0.6)
    assert isinstance(ap, so.CombSignal) and (ap.delay, ap.b0, ap.bD, ap.a) == (9, -0.6, 1.0, 0.6)
    # the tail of an echo is the caller's to ask for
    tail = x | so.Pad(so.zero) | so.Until(300 * so.frames) | so.Comb(7, 0.5)
    assert so.nframes(tail) == 300
    assert so.nframes(so.Comb(x | so.Filt(so.Lowpass, 1 * so.kHz), 3, 0.5)) == 100  # a computed child
    assert so.sampletype(y | so.ToEltype(np.float32)) == np.float32


def test_currying_and_piping():
    x = _x()
    y = x | so.Comb(5, 0.5, feedforward=0.1, direct=0.9)
    assert isinstance(y, so.CombSignal) and y.signal is x and (y.delay, y.b0, y.bD, y.a) == (5, 0.9, 0.1, 0.5)
    a = x | so.Allpass(5, -0.5)
    assert (a.delay, a.b0, a.bD, a.a) == (5, 0.5, 1.0, -0.5)
    z = np.zeros((100, 2)) | so.Comb(3, 0.5)  # a bare array on the left
    assert isinstance(z, so.CombSignal) and z.nch == 2
    assert so.nframes(so.pipe(x, so.Comb(3, 0.5), so.Allpass(4, 0.5), so.Until(10 * so.frames))) == 10


def test_a_delay_as_a_time_as_frames_and_as_a_number():
    x = _x(fs=10 * so.kHz)
    assert so.Comb(x, 7, 0.5).delay == 7
    assert so.Comb(x, 7.0, 0.5).delay == 7 and so.Comb(x, np.int64(7), 0.5).delay == 7
    assert so.Comb(x, 7 * so.frames, 0.5).delay == 7
    assert so.Comb(x, 2 * so.ms, 0.5).delay == 20 and so.Comb(x, 0.0021 * so.s, 0.5).delay == 21
    assert so.Comb(x, 0.25 * so.ms, 0.5).delay == 2  # floor(2.5), as cuts convert a time
    assert so.Allpass(x, 1 * so.ms, 0.5).delay == 10
    assert so.Comb(_x(fs=None), 7, 0.5).fs is None


def test_toframerate():
    y = so.Comb(_x(fs=None), 7, 0.5)  # no rate: it is handed to x, the delay stays a number of frames
    z = so.ToFramerate(y, 8 * so.kHz)
    assert isinstance(z, so.CombSignal) and z.fs == 8000.0 and z.signal.fs == 8000.0 and z.delay == 7 and (z.b0, z.bD, z.a) == (y.b0, y.bD, y.a)
    assert so.nframes(z) == 100
    y = so.Comb(_x(), 7, 0.5)  # a rate: resampled like any computed signal
    z = so.ToFramerate(y, 20 * so.kHz)
    assert isinstance(z, so.FilteredSignal) and isinstance(z.fn, so.ResamplerFn) and z.signal is y
    assert z.fs == 20_000.0 and so.nframes(z) == 200
    assert so.ToFramerate(y, FS) is y


# ---- 4. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_name_the_construct():
    x = _x()
    cases = [
        (lambda: so.Comb(so.Signal(np.sin, FS, ω=5 * so.Hz), 7, 0.5), "use `Until`"),
        (lambda: so.Comb(so.Signal(np.zeros(10)) | so.Filt(so.Lowpass, 1 * so.kHz), 7, 0.5), "use `Until`"),  # unknown: no rate
        (lambda: so.Allpass(so.Signal(np.sin, FS, ω=5 * so.Hz), 7, 0.5), "use `Until`"),
        (lambda: so.Comb(so.Signal(np.arange(10), FS), 7, 0.5), "Float32 or Float64"),
        (lambda: so.Comb(x, 0, 0.5), "at least one frame"),
        (lambda: so.Comb(x, -3, 0.5), "at least one frame"),
        (lambda: so.Comb(x, 0.00001 * so.ms, 0.5), "at least one frame"),
        (lambda: so.Comb(x, 2.5, 0.5), "whole number of frames"),
        (lambda: so.Comb(x, 2.5 * so.frames, 0.5), "whole number of frames"),
        (lambda: so.Comb(x, np.nan, 0.5), "whole number of frames"),
        (lambda: so.Comb(x, "7", 0.5), "whole number of frames"),
        (lambda: so.Comb(x, 3 * so.Hz, 0.5), "neither a time nor a number of frames"),
        (lambda: so.Comb(_x(fs=None), 2 * so.ms, 0.5), "needs the frame rate of x"),
        (lambda: so.Comb(x, 7, np.inf), "g must be a finite number"),
        (lambda: so.Comb(x, 7, np.nan), "g must be a finite number"),
        (lambda: so.Comb(x, 7, "0.5"), "g must be a finite number"),
        (lambda: so.Comb(x, 7, 1 + 2j), "g must be a finite number"),
        (lambda: so.Comb(x, 7, 0.5, feedforward=np.inf), "feedforward must be a finite number"),
        (lambda: so.Comb(x, 7, 0.5, direct=None), "direct must be a finite number"),
        (lambda: so.Allpass(x, 7, np.nan), "must be a finite number"),
        (lambda: so.Allpass(x, 7, None), "must be a finite number"),
        (lambda: engine._streamable(so.Comb(x, 7, 0.5) | so.Filt(so.Lowpass, 1 * so.kHz)), "BlockStream: Comb"),
        (lambda: engine._streamable(so.Mix(so.Allpass(x, 7, 0.5), 1.0)), "BlockStream: Comb"),
        (lambda: sharding.shard_time(so.Comb(x, 7, 0.5), 0, 2), "Comb / Allpass over several GPUs is not built"),
        (lambda: sharding.shard_channels(so.Mix(so.Allpass(x, 7, 0.5), 1.0), 0, 2), "Comb / Allpass over several GPUs is not built"),
        (lambda: sharding.shard_append(so.Append(so.Comb(x, 7, 0.5), so.Comb(x, 7, 0.5)), 0, 2), "Comb / Allpass over several GPUs is not built"),
    ]
    for make, words in cases:
        with pytest.raises(so.ErrorException) as e:
            make()
        assert "Comb" in str(e.value) and words in str(e.value), str(e.value)


# ---- 5. the lowered node ---------------------------------------------------------------------------------------------
def test_the_lowered_node():
    assert K.NODE_COMB == 13
    x = _x(100, 2, np.float32)
    for tree, fields in ((so.Comb(x, 7, 0.5), (7, 1.0, 0.0, 0.5)), (so.Comb(x, 9, -0.25, feedforward=0.75, direct=2.0), (9, 2.0, 0.75, -0.25)),
                         (so.Allpass(x, 11, 0.6), (11, -0.6, 1.0, 0.6))):
        lw = LW.lower(tree)
        nd = lw.nodes[lw.root]
        assert nd.kind == K.NODE_COMB and (nd.l0, nd.d0, nd.d1, nd.d2) == fields
        assert nd.n_children == 1 and nd.nch == 2 and nd.dtype == K.SO_F64 and nd.nframes == 100 and nd.fs == 10_000.0
        cx = lw.nodes[nd.children[0]]
        assert cx.kind == K.NODE_ARRAY and cx.l0 == 100 and cx.dtype == K.SO_F32 and cx.nch == 2
        assert (nd.i0, nd.i1, nd.i2, nd.i3, nd.l1, nd.s0, nd.s1, nd.d3) == (0,) * 8 and not nd.p0 and not nd.p1


def test_demand_starts_at_frame_0_whatever_the_window():
    x = _x(100, 2)
    tree = so.Comb(x, 7, 0.5)
    need = {}
    LW._demand(tree | so.Until(10 * so.frames), 10, need)
    assert need[id(x)] == (10, 0)
    need = {}
    LW._demand(tree | so.After(5 * so.frames) | so.Until(10 * so.frames), 10, need)
    assert need[id(x)] == (15, 0)  # the skipped frames are computed too: the skip is not handed on


def test_the_exported_unroll_depth_is_read_from_the_header():
    assert 2 <= unroll() <= 64
