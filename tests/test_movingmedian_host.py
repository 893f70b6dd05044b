"""`MovingMedian(x, w)` / `MovingQuantile(x, w, q)` above the C-ABI (signals.py, lowering.py): the vectorised NumPy form the
device is held to (tests/movingmedian_ref.py) checked bit for bit against the loop that states the definition, the ranks 0
and m - 1 against `MovingMin` / `MovingMax`'s reference, `np.median` where the two agree and the pinned fact where they do
not, the constructors and their refusals, the `ToFramerate` rules, the `BlockStream` and shard refusals and the lowered
node.  No GPU needed."""
import re
from pathlib import Path

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

import sigops_amd as so
from sigops_amd import _capi as K
from sigops_amd import engine, sharding
from sigops_amd import lowering as LW
from sigops_amd import signals as S
from moving_ref import moving_1d
from movingmedian_ref import halves, kernel_constants, movrank_1d, movrank_loop, movrank_ref, rank_of, same_bits, tied

FS = 10 * so.kHz
NZ, PZ, INF, NAN = -0.0, 0.0, np.inf, np.nan
QS = (0, 0.25, 0.3, 0.5, 0.9, 1)
ROOT = Path(__file__).resolve().parent.parent


def _x(n=100, c=2, dtype=np.float64, fs=FS):
    return so.Signal(np.asfortranarray(np.arange(n * c, dtype=dtype).reshape(c, n).T), fs)


# ---- 1. the reference ------------------------------------------------------------------------------------------------
def test_the_constants_are_read_from_the_kernel_header():
    T, H = kernel_constants()
    assert T >= 64 and T % 256 == 0 and 1 <= H <= T
    assert S.MOVING_RANK_HALO == H  # the constructor's limit is the kernel's


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_numpy_form_equals_the_loop_bit_for_bit(dtype):
    """N in 1 .. 70, W in 1 .. 12 with every `ahead`, every q of the list: the full product, on inputs full of ties, with zeros
    of both signs, both infinities and a NaN"""
    for N in range(1, 71):
        x = tied(N, dtype, seed=N)
        for W in range(1, 13):
            for ahead in range(W):
                for q in QS:
                    got, want = movrank_1d(x, W - 1 - ahead, ahead, q), movrank_loop(x, W - 1 - ahead, ahead, q)
                    assert same_bits(got, want), (N, W, ahead, q)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ranks_0_and_m_less_1_are_the_minimum_and_the_maximum(dtype):
    for N in (1, 2, 7, 64, 300):
        x = tied(N, dtype, seed=2)
        for back, ahead in [(0, 0), (1, 0), (0, 1), (3, 2), (63, 0), (0, 64), (N - 1, 0), (N + 5, N + 5), (17, 5)]:
            for f in (movrank_1d, movrank_loop):
                assert same_bits(f(x, back, ahead, 0), moving_1d(x, back, ahead, True)), (N, back, ahead, f.__name__)
                assert same_bits(f(x, back, ahead, 1), moving_1d(x, back, ahead, False)), (N, back, ahead, f.__name__)  # (the NaN rule too)


def test_interior_frames_of_an_odd_centred_window_are_numpys_median():
    x = halves(500, 1, seed=9)[:, 0].copy()
    for W in (1, 3, 5, 11, 101):
        a = (W - 1) // 2
        y = movrank_1d(x, a, a, 0.5)
        assert np.array_equal(y[a:500 - a], np.median(sliding_window_view(x, W), axis=1))


def test_the_lower_median_at_an_even_edge_window():
    x = np.array([1.0, 4.0, 2.0, 8.0, 16.0])
    for f in (movrank_1d, movrank_loop):
        y = f(x, 1, 1, 0.5)  # windows {1, 4} | {1, 4, 2} | {4, 2, 8} | {2, 8, 16} | {8, 16}
        assert same_bits(y, np.array([1.0, 2.0, 4.0, 8.0, 8.0]))  # the LOWER of two, where np.median gives 2.5 and 12
        assert np.median(x[:2]) == 2.5 and np.median(x[3:]) == 12.0
        assert same_bits(f(x, 1, 0, 0.5), np.array([1.0, 1.0, 2.0, 2.0, 8.0]))  # an even window: the lower everywhere


def test_hand_written_answers():
    a = lambda v: np.array(v, dtype=np.float64)  # noqa: E731
    for f in (movrank_1d, movrank_loop):
        # the zeros are distinct and ordered: of {-0.0, +0.0, -0.0} the ranks 0, 1 are -0.0 and rank 2 is +0.0
        z = a([NZ, PZ, NZ])
        assert same_bits(f(z, 2, 2, 0.0), a([NZ] * 3)) and same_bits(f(z, 2, 2, 0.5), a([NZ] * 3)) and same_bits(f(z, 2, 2, 1.0), a([PZ] * 3))
        assert same_bits(f(a([PZ, NZ, PZ]), 2, 2, 0.5), a([PZ] * 3)) and same_bits(f(a([PZ, NZ]), 1, 1, 0.5), a([NZ, NZ]))
        # W = 1 is x itself, NaN, infinities and zeros of both signs included
        z = a([NZ, PZ, -INF, NAN, INF, 1.5])
        for q in QS:
            assert same_bits(f(z, 0, 0, q), z)
        # a NaN covers exactly the frames whose window holds it: n - back <= k <= n + ahead
        y = f(a([1, 2, 3, NAN, 5, 6, 7, 8]), 2, 1, 0.5)
        assert list(np.isnan(y)) == [False, False, True, True, True, True, False, False]
        assert same_bits(y[[0, 1, 6, 7]], a([1, 2, 6, 7]))
        # infinities are ordinary samples
        assert same_bits(f(a([1, INF, -INF, 2, 3]), 1, 1, 0.5), a([1, 1, 2, 2, 2]))
        # quantiles of a clipped causal window of 5: m = 1 .. 5, r = floor(0.9 (m - 1)) = 0, 0, 1, 2, 3
        assert same_bits(f(a([5, 3, 4, 1, 2, 9]), 4, 0, 0.9), a([5, 3, 4, 4, 4, 4]))
        assert f(np.array([1, 2], np.float32), 1, 0, 0.5).dtype == np.float32


def test_the_rank_is_one_float64_product_floored():
    assert rank_of(0.3, 11) == int(np.floor(np.float64(0.3) * 10)) == 3
    assert rank_of(0.7, 11) == int(np.floor(np.float64(0.7) * 10)) == 7
    assert rank_of(0.29, 101) == int(np.floor(np.float64(0.29) * 100)) == 28  # 0.29 * 100 = 28.999999999999996 in Float64
    assert [rank_of(0.5, m) for m in (1, 2, 3, 4, 5)] == [0, 0, 1, 1, 2] and rank_of(1, 7) == 6 and rank_of(0, 7) == 0


def test_the_reference_handles_channels_and_vectors():
    x = np.asfortranarray(np.stack([tied(50, seed=s) for s in range(3)], axis=1))
    y = movrank_ref(x, 4, 2, 0.3)
    assert y.shape == (50, 3) and y.dtype == np.float64
    for c in range(3):
        assert same_bits(y[:, c], movrank_loop(x[:, c], 4, 2, 0.3))
    assert movrank_ref(x[:, 0], 4, 2, 0.5).shape == (50, 1)


# ---- 2. constructors -------------------------------------------------------------------------------------------------
def test_direct_and_curried_forms():
    x = _x()
    y = so.MovingMedian(x, 5)
    assert isinstance(y, so.MovingRankSignal) and y.evaltrait == "computed" and y.signal is x and y.children == (x,)
    assert (y.back, y.ahead, y.q) == (4, 0, 0.5)  # the causal window [n - W + 1, n]
    z = x | so.MovingMedian(5, center=True)
    assert isinstance(z, so.MovingRankSignal) and z.signal is x and (z.back, z.ahead, z.q) == (2, 2, 0.5)
    u = so.MovingQuantile(x, 480, 0.1)
    assert isinstance(u, so.MovingRankSignal) and (u.back, u.ahead, u.q) == (479, 0, 0.1)
    v = x | so.MovingQuantile(480, 0.1, ahead=3)
    assert v.signal is x and (v.back, v.ahead, v.q) == (476, 3, 0.1)
    assert (so.MovingQuantile(x, 6, 1, center=True).back, so.MovingQuantile(x, 6, 0, center=True).ahead) == (3, 2)
    assert (so.MovingMedian(x, 1).back, so.MovingMedian(x, 1).ahead) == (0, 0)
    b = np.zeros((100, 2)) | so.MovingMedian(3)  # a bare array on the left
    assert isinstance(b, so.MovingRankSignal) and b.nch == 2 and b.fs is None
    assert so.MovingMedian.__doc__ and "LOWER" in so.MovingMedian.__doc__ and "np.median" in so.MovingMedian.__doc__
    assert so.MovingQuantile.__doc__ and "floor(q * (m - 1))" in so.MovingQuantile.__doc__


def test_frames_and_times_give_the_same_node():
    x = _x()  # 10 kHz: 1 ms = 10 frames
    a = so.MovingMedian(x, 50, ahead=20)
    for w, ah in ((50 * so.frames, 20 * so.frames), (5 * so.ms, 2 * so.ms), (5 * so.ms, 20), (50.0, 20 * so.frames)):
        b = so.MovingQuantile(x, w, 0.5, ahead=ah)
        assert (b.back, b.ahead, b.q) == (a.back, a.ahead, a.q) == (29, 20, 0.5), (w, ah)
    assert (so.MovingMedian(x, 5 * so.ms, center=True).back, so.MovingMedian(x, 5 * so.ms, center=True).ahead) == (25, 24)


def test_length_rate_channels_and_type():
    x = _x(100, 3, np.float32, fs=44.1 * so.kHz)
    y = so.MovingMedian(x, 9, center=True)
    assert so.nframes(y) == 100 and so.nchannels(y) == 3 and so.framerate(y) == 44_100.0
    assert so.sampletype(y) == np.float32 and so.duration(y) == 100 / 44_100.0  # Float32 stays Float32
    assert so.sampletype(so.MovingQuantile(_x(), 3, 0.25)) == np.float64
    assert so.nframes(so.MovingMedian(x | so.Filt(so.Lowpass, 1 * so.kHz), 5)) == 100  # a computed child
    assert so.MovingMedian(_x(fs=None), 3).fs is None
    s = so.Signal(np.sin, FS, ω=5 * so.Hz)  # an infinite x is accepted, and stays infinite
    y = s | so.MovingMedian(2 * so.ms, ahead=1 * so.ms)
    assert isinstance(y, so.MovingRankSignal) and S.isknowninf(so.nframes(y)) and (y.back, y.ahead) == (9, 10)
    assert so.nframes(y | so.Until(300 * so.frames)) == 300


def test_constructor_refusals():
    T, H = kernel_constants()
    x = _x()
    long = _x(3 * H, 1)
    cases = [
        (lambda: so.MovingMedian(so.Signal(np.arange(10), FS), 3), "MovingMedian", "Float32 or Float64"),
        (lambda: so.MovingQuantile(so.Signal(np.arange(10), FS), 3, 0.5), "MovingQuantile", "Float32 or Float64"),
        (lambda: so.MovingMedian(x, 0), "MovingMedian", "at least one frame"),
        (lambda: so.MovingQuantile(x, -3, 0.5), "MovingQuantile", "at least one frame"),
        (lambda: so.MovingMedian(x, 2.5), "MovingMedian", "whole number of frames"),
        (lambda: so.MovingMedian(x, 5, ahead=5), "MovingMedian", "[0, 4]"),
        (lambda: so.MovingQuantile(x, 5, 0.5, ahead=-1), "MovingQuantile", "[0, 4]"),
        (lambda: so.MovingMedian(x, 5, ahead=2, center=True), "MovingMedian", "not both"),
        (lambda: x | so.MovingQuantile(5, 0.5, ahead=0, center=True), "MovingQuantile", "not both"),
        (lambda: so.MovingQuantile(x, 5, -0.01), "MovingQuantile", "in [0, 1]"),
        (lambda: so.MovingQuantile(x, 5, 1.01), "MovingQuantile", "in [0, 1]"),
        (lambda: so.MovingQuantile(x, 5, float("nan")), "MovingQuantile", "in [0, 1]"),
        (lambda: so.MovingQuantile(x, 5, float("inf")), "MovingQuantile", "in [0, 1]"),
        (lambda: x | so.MovingQuantile(5, "0.5"), "MovingQuantile", "in [0, 1]"),
        (lambda: so.MovingMedian(_x(fs=None), 5 * so.ms), "MovingMedian", "needs the frame rate of x"),
        (lambda: np.zeros(10) | so.MovingQuantile(5 * so.ms, 0.5), "MovingQuantile", "needs the frame rate of x"),
        (lambda: so.MovingMedian(x, 5 * so.Hz), "MovingMedian", "neither a time nor a number of frames"),
        (lambda: so.MovingMedian(long, H + 2), "MovingMedian", f"longer than the {H + 1} frames"),
        (lambda: long | so.MovingQuantile(H + 2, 0.1, center=True), "MovingQuantile", f"longer than the {H + 1} frames"),
        (lambda: so.Signal(np.sin, FS, ω=5 * so.Hz) | so.MovingMedian(H + 2), "MovingMedian", f"longer than the {H + 1} frames"),
        (lambda: so.MovingMedian(), "MovingMedian", "MovingMedian(x, w) expected"),
        (lambda: so.MovingMedian(x, 3, 1), "MovingMedian", "MovingMedian(x, w) expected"),
        (lambda: so.MovingQuantile(x), "MovingQuantile", "MovingQuantile(x, w, q) expected"),
    ]
    for make, name, words in cases:
        with pytest.raises(so.ErrorException) as e:
            make()
        assert name in str(e.value) and words in str(e.value), str(e.value)
    # the limit is the kernel's, and a window longer than the signal is the signal: not refused for its nominal length
    assert so.MovingMedian(long, H + 1).back == H
    y = so.MovingMedian(_x(100, 1), 5000, center=True)
    assert (y.back, y.ahead) == (2500, 2499)


def test_toframerate():
    y = so.MovingMedian(_x(fs=None), 7, ahead=2)  # no rate: it is handed to x, the frame counts stay
    z = so.ToFramerate(y, 8 * so.kHz)
    assert isinstance(z, so.MovingRankSignal) and z.fs == 8000.0 and z.signal.fs == 8000.0 and so.nframes(z) == 100
    assert (z.back, z.ahead, z.q) == (4, 2, 0.5)
    y = so.MovingQuantile(_x(), 7, 0.25)  # a rate: resampled like any computed signal
    z = so.ToFramerate(y, 20 * so.kHz)
    assert isinstance(z, so.FilteredSignal) and isinstance(z.fn, so.ResamplerFn) and z.signal is y
    assert z.fs == 20_000.0 and so.nframes(z) == 200
    assert so.ToFramerate(y, FS) is y


# ---- 3. refusals above the node --------------------------------------------------------------------------------------
def test_blockstream_and_shards_refuse_the_node_by_name():
    x = _x()
    name = "MovingMedian / MovingQuantile"
    cases = [
        (lambda: engine._streamable(so.MovingMedian(x, 5) | so.Filt(so.Lowpass, 1 * so.kHz)), f"BlockStream: {name}", "not streamable"),
        (lambda: engine._streamable(so.Mix(so.MovingQuantile(x, 5, 0.1, center=True), 1.0)), f"BlockStream: {name}", "not streamable"),
        (lambda: sharding.shard_time(so.MovingMedian(x, 5), 0, 2), "shard_time", f"{name} over several GPUs is not built"),
        (lambda: sharding.shard_channels(so.Mix(so.MovingQuantile(x, 5, 0.9), 1.0), 0, 2), "shard_channels", f"{name} over several GPUs is not built"),
        (lambda: sharding.shard_append(so.Append(so.MovingMedian(x, 5), so.MovingMedian(x, 5)), 0, 2), "shard_append", f"{name} over several GPUs is not built"),
    ]
    for make, where, words in cases:
        with pytest.raises(so.ErrorException) as e:
            make()
        assert where in str(e.value) and words in str(e.value), str(e.value)
    with pytest.raises(so.ErrorException) as e:  # its own reason, and the other refusals still name their nodes
        sharding.shard_time(so.MovingMedian(x, 5), 0, 2)
    assert "halo" in str(e.value) and "every frame before" not in str(e.value)
    with pytest.raises(so.ErrorException) as e:
        sharding.shard_time(so.MovingMax(x, 5), 0, 2)
    assert "MovingMax / MovingMin over several GPUs is not built" in str(e.value)


# ---- 4. the lowered node ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,code", [(np.float32, K.SO_F32), (np.float64, K.SO_F64)])
def test_the_lowered_node(dtype, code):
    x = _x(100, 2, dtype)
    for tree, q in ((so.MovingMedian(x, 12, ahead=4), 0.5), (so.MovingQuantile(x, 12, 0.3, ahead=4), 0.3)):
        lw = LW.lower(tree)
        nd = lw.nodes[lw.root]
        assert nd.kind == K.NODE_MOVRANK and nd.n_children == 1 and nd.nch == 2 and nd.dtype == code and nd.nframes == 100 and nd.fs == 10_000.0
        assert (nd.l0, nd.l1, nd.d0) == (7, 4, q)
        cx = lw.nodes[nd.children[0]]
        assert cx.kind == K.NODE_ARRAY and cx.l0 == 100 and cx.dtype == code and cx.nch == 2
        assert (nd.i0, nd.i1, nd.i2, nd.i3, nd.s0, nd.s1, nd.d1, nd.d2, nd.d3) == (0,) * 9 and not nd.p0 and not nd.p1


def test_demand_reaches_ahead_and_starts_at_frame_0():
    x = _x(100, 2)
    tree = so.MovingMedian(x, 8, ahead=5)
    need = {}
    LW._demand(tree | so.Until(10 * so.frames), 10, need)
    assert need[id(x)] == (15, 0)  # the last frame's window reaches 5 frames further
    need = {}
    LW._demand(tree | so.After(5 * so.frames) | so.Until(10 * so.frames), 10, need)
    assert need[id(x)] == (20, 0)
    need = {}
    LW._demand(tree, 100, need)
    assert need[id(x)] == (100, 0)  # capped by the length of x


def test_the_node_kind_and_the_header():
    assert K.NODE_MOVRANK == 19 and K.NODE_RECUR2 == 18
    text = (ROOT / "include" / "sigops.h").read_text()
    assert re.search(r"SO_NODE_MOVRANK = 19\s+/\* MovingMedian / MovingQuantile", text)
    assert re.search(r"\*  MOVRANK   child 0 = x", text) and "d0 = q, a number in [0, 1]" in text
    assert len(re.findall(r"^[A-Za-z_][^\n]*\bso_[a-z_0-9]+\(", text, re.M)) == 32  # no new entry point: the node came with none
