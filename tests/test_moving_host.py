"""`MovingMax(x, w)` / `MovingMin(x, w)` above the C-ABI (signals.py, lowering.py): the O(N) NumPy form the device is held to
(tests/moving_ref.py) checked bit for bit against the scalar loop that states the definition, the identity
`MovingMin(x) == -MovingMax(-x)`, hand-written answers, the constructors and their refusals, the `ToFramerate` rules, the
`BlockStream` and shard refusals and the lowered node.  No GPU needed."""
import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import _capi as K
from sigops_amd import engine, sharding
from sigops_amd import lowering as LW
from moving_ref import kernel_constants, moving_1d, moving_loop, moving_ref, same_bits, tied

FS = 10 * so.kHz
NZ, PZ, INF, NAN = -0.0, 0.0, np.inf, np.nan


def _x(n=100, c=2, dtype=np.float64, fs=FS):
    return so.Signal(np.asfortranarray(np.arange(n * c, dtype=dtype).reshape(c, n).T), fs)


def _windows(N):
    return [(0, 0), (1, 0), (0, 1), (3, 2), (63, 0), (0, 64), (N - 1, 0), (N + 5, N + 5), (17, 5)]


# ---- 1. the reference ------------------------------------------------------------------------------------------------
def test_the_constants_are_read_from_the_kernel_header():
    T, H = kernel_constants()
    assert T >= 64 and T & (T - 1) == 0 and H >= 1


@pytest.mark.parametrize("is_min", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_numpy_form_equals_the_scalar_loop_bit_for_bit(dtype, is_min):
    for N in (1, 2, 7, 64, 300):
        x = tied(N, dtype)
        for back, ahead in _windows(N):
            got, want = moving_1d(x, back, ahead, is_min), moving_loop(x, back, ahead, is_min)
            assert got.dtype == dtype and same_bits(got, want), (N, back, ahead)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_minimum_is_the_negated_maximum_of_the_negated_signal(dtype):
    for N in (1, 2, 7, 64, 300):
        x = tied(N, dtype, seed=1)
        for back, ahead in _windows(N):
            for f in (moving_1d, moving_loop):
                assert same_bits(f(x, back, ahead, True), -f(-x, back, ahead, False)), (N, back, ahead, f.__name__)


def test_hand_written_answers():
    for f in (moving_1d, moving_loop):
        a = lambda v: np.array(v, dtype=np.float64)  # noqa: E731
        # only -0.0 stays -0.0; +0.0 beats -0.0 for the maximum, -0.0 beats +0.0 for the minimum
        assert same_bits(f(a([NZ, NZ, NZ]), 1, 1), a([NZ, NZ, NZ]))
        assert same_bits(f(a([NZ, NZ, NZ]), 1, 1, True), a([NZ, NZ, NZ]))
        assert same_bits(f(a([NZ, PZ]), 1, 1), a([PZ, PZ]))
        assert same_bits(f(a([NZ, PZ]), 1, 1, True), a([NZ, NZ]))
        assert same_bits(f(a([PZ, NZ, NZ]), 1, 0), a([PZ, PZ, NZ]))
        # clipping at both ends: causal, anti-causal and centred windows of 3 frames
        x = a([3, 1, 4, 1, 5, 9, 2, 6])
        assert same_bits(f(x, 2, 0), a([3, 3, 4, 4, 5, 9, 9, 9]))
        assert same_bits(f(x, 0, 2), a([4, 4, 5, 9, 9, 9, 6, 6]))
        assert same_bits(f(x, 1, 1), a([3, 4, 4, 5, 9, 9, 9, 6]))
        assert same_bits(f(x, 1, 1, True), a([1, 1, 1, 1, 1, 2, 2, 2]))
        assert same_bits(f(x, 100, 100), np.full(8, 9.0)) and same_bits(f(x, 100, 100, True), np.full(8, 1.0))
        # W = 1 is the identity, NaN, infinities and zeros of both signs included
        z = a([NZ, PZ, -INF, NAN, INF, 1.5])
        assert same_bits(f(z, 0, 0), z) and same_bits(f(z, 0, 0, True), z)
        # NaN covers exactly the frames whose window holds it: n - back <= k <= n + ahead
        y = f(a([1, 2, 3, NAN, 5, 6, 7, 8]), 2, 1)
        assert list(np.isnan(y)) == [False, False, True, True, True, True, False, False]
        assert same_bits(y[[0, 1, 6, 7]], a([2, 3, 8, 8]))
        y = f(a([NAN, 2, 3, 4]), 1, 0, True)
        assert list(np.isnan(y)) == [True, True, False, False]
        # infinities are ordinary samples
        assert same_bits(f(a([1, INF, -INF, 2]), 1, 0), a([1, INF, INF, 2]))
        assert same_bits(f(a([1, INF, -INF, 2]), 1, 0, True), a([1, 1, -INF, -INF]))
        # Float32 stays Float32
        assert f(np.array([1, 2], np.float32), 1, 0).dtype == np.float32


# ---- 2. constructors -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctor,is_min", [(so.MovingMax, False), (so.MovingMin, True)])
def test_direct_and_curried_forms(ctor, is_min):
    x = _x()
    y = ctor(x, 5)
    assert isinstance(y, so.MovingSignal) and y.evaltrait == "computed" and y.signal is x and y.children == (x,)
    assert (y.back, y.ahead, y.is_min) == (4, 0, is_min)  # the causal window [n - W + 1, n]
    z = x | ctor(5, ahead=3)
    assert isinstance(z, so.MovingSignal) and z.signal is x and (z.back, z.ahead, z.is_min) == (1, 3, is_min)
    c = ctor(x, 6, center=True)
    assert (c.back, c.ahead) == (3, 2)
    c = x | ctor(7, center=True)
    assert (c.back, c.ahead) == (3, 3)
    assert (ctor(x, 1).back, ctor(x, 1).ahead) == (0, 0)
    assert (ctor(x, 4, ahead=3).back, ctor(x, 4, ahead=3).ahead) == (0, 3)
    b = np.zeros((100, 2)) | ctor(3)  # a bare array on the left
    assert isinstance(b, so.MovingSignal) and b.nch == 2 and b.fs is None


def test_frames_and_times_give_the_same_node():
    x = _x()  # 10 kHz: 1 ms = 10 frames
    a = so.MovingMax(x, 50, ahead=20)
    for w, ah in ((50 * so.frames, 20 * so.frames), (5 * so.ms, 2 * so.ms), (5 * so.ms, 20), (50.0, 20 * so.frames)):
        b = so.MovingMax(x, w, ahead=ah)
        assert (b.back, b.ahead, b.is_min) == (a.back, a.ahead, a.is_min) == (29, 20, False), (w, ah)
    assert (so.MovingMin(x, 5 * so.ms, center=True).back, so.MovingMin(x, 5 * so.ms, center=True).ahead) == (25, 24)


def test_length_rate_channels_and_type():
    x = _x(100, 3, np.float32, fs=44.1 * so.kHz)
    y = so.MovingMax(x, 9, center=True)
    assert so.nframes(y) == 100 and so.nchannels(y) == 3 and so.framerate(y) == 44_100.0
    assert so.sampletype(y) == np.float32 and so.duration(y) == 100 / 44_100.0  # Float32 stays Float32
    assert so.sampletype(so.MovingMin(_x(), 3)) == np.float64
    assert so.nframes(so.MovingMax(x | so.Filt(so.Lowpass, 1 * so.kHz), 5)) == 100  # a computed child
    assert so.MovingMax(_x(fs=None), 3).fs is None
    # an infinite x is accepted, and stays infinite
    s = so.Signal(np.sin, FS, ω=5 * so.Hz)
    y = s | so.MovingMax(2 * so.ms, ahead=1 * so.ms)
    assert isinstance(y, so.MovingSignal) and so.signals.isknowninf(so.nframes(y)) and (y.back, y.ahead) == (9, 10)
    assert so.nframes(y | so.Until(300 * so.frames)) == 300


def test_constructor_refusals():
    x = _x()
    cases = [
        (lambda: so.MovingMax(x, 0), "MovingMax", "at least one frame"),
        (lambda: so.MovingMin(x, -3), "MovingMin", "at least one frame"),
        (lambda: so.MovingMax(x, 2.5), "MovingMax", "whole number of frames"),
        (lambda: so.MovingMax(x, 5, ahead=1.5), "MovingMax", "whole number of frames"),
        (lambda: so.MovingMax(x, float("nan")), "MovingMax", "whole number of frames"),
        (lambda: so.MovingMax(x, "5"), "MovingMax", "whole number of frames"),
        (lambda: so.MovingMax(_x(fs=None), 5 * so.ms), "MovingMax", "needs the frame rate of x"),
        (lambda: np.zeros(10) | so.MovingMin(5 * so.ms), "MovingMin", "needs the frame rate of x"),
        (lambda: so.MovingMax(_x(fs=None), 5, ahead=1 * so.ms), "MovingMax", "needs the frame rate of x"),
        (lambda: so.MovingMax(x, 5 * so.Hz), "MovingMax", "neither a time nor a number of frames"),
        (lambda: so.MovingMax(x, 5, ahead=5), "MovingMax", "[0, 4]"),
        (lambda: so.MovingMin(x, 5, ahead=-1), "MovingMin", "[0, 4]"),
        (lambda: so.MovingMax(x, 5, ahead=2, center=True), "MovingMax", "not both"),
        (lambda: x | so.MovingMax(5, ahead=0, center=True), "MovingMax", "not both"),
        (lambda: so.MovingMax(so.Signal(np.arange(10), FS), 3), "MovingMax", "Float32 or Float64"),
        (lambda: so.MovingMin(so.Signal(np.arange(10), FS), 3), "MovingMin", "Float32 or Float64"),
        (lambda: so.MovingMax(), "MovingMax", "MovingMax(x, w) expected"),
        (lambda: so.MovingMin(x, 3, 1), "MovingMin", "MovingMin(x, w) expected"),
    ]
    for make, name, words in cases:
        with pytest.raises(so.ErrorException) as e:
            make()
        assert name in str(e.value) and words in str(e.value), str(e.value)


def test_toframerate():
    y = so.MovingMax(_x(fs=None), 7, ahead=2)  # no rate: it is handed to x, the frame counts stay
    z = so.ToFramerate(y, 8 * so.kHz)
    assert isinstance(z, so.MovingSignal) and z.fs == 8000.0 and z.signal.fs == 8000.0 and so.nframes(z) == 100
    assert (z.back, z.ahead, z.is_min) == (4, 2, False)
    y = so.MovingMin(_x(), 7)  # a rate: resampled like any computed signal
    z = so.ToFramerate(y, 20 * so.kHz)
    assert isinstance(z, so.FilteredSignal) and isinstance(z.fn, so.ResamplerFn) and z.signal is y
    assert z.fs == 20_000.0 and so.nframes(z) == 200
    assert so.ToFramerate(y, FS) is y


# ---- 3. refusals above the node --------------------------------------------------------------------------------------
def test_blockstream_and_shards_refuse_the_node_by_name():
    x = _x()
    cases = [
        (lambda: engine._streamable(so.MovingMax(x, 5) | so.Filt(so.Lowpass, 1 * so.kHz)), "BlockStream: MovingMax / MovingMin", "not streamable"),
        (lambda: engine._streamable(so.Mix(so.MovingMin(x, 5, center=True), 1.0)), "BlockStream: MovingMax / MovingMin", "not streamable"),
        (lambda: sharding.shard_time(so.MovingMax(x, 5), 0, 2), "shard_time", "MovingMax / MovingMin over several GPUs is not built"),
        (lambda: sharding.shard_channels(so.Mix(so.MovingMin(x, 5), 1.0), 0, 2), "shard_channels", "MovingMax / MovingMin over several GPUs is not built"),
        (lambda: sharding.shard_append(so.Append(so.MovingMax(x, 5), so.MovingMax(x, 5)), 0, 2), "shard_append", "MovingMax / MovingMin over several GPUs is not built"),
    ]
    for make, name, words in cases:
        with pytest.raises(so.ErrorException) as e:
            make()
        assert name in str(e.value) and words in str(e.value), str(e.value)
    with pytest.raises(so.ErrorException) as e:  # its own reason, not the recurrences'
        sharding.shard_time(so.MovingMax(x, 5), 0, 2)
    assert "halo" in str(e.value) and "every frame before" not in str(e.value)
    with pytest.raises(so.ErrorException) as e:  # the other refusals still name their nodes
        sharding.shard_time(so.Comb(x, 7, 0.5), 0, 2)
    assert "Comb / Allpass over several GPUs is not built" in str(e.value)


# ---- 4. the lowered node ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,code", [(np.float32, K.SO_F32), (np.float64, K.SO_F64)])
def test_the_lowered_node(dtype, code):
    assert K.NODE_MOVING == 15
    x = _x(100, 2, dtype)
    for ctor, i0 in ((so.MovingMax, 0), (so.MovingMin, 1)):
        lw = LW.lower(ctor(x, 12, ahead=4))
        nd = lw.nodes[lw.root]
        assert nd.kind == K.NODE_MOVING and nd.n_children == 1 and nd.nch == 2 and nd.dtype == code and nd.nframes == 100 and nd.fs == 10_000.0
        assert (nd.l0, nd.l1, nd.i0) == (7, 4, i0)
        cx = lw.nodes[nd.children[0]]
        assert cx.kind == K.NODE_ARRAY and cx.l0 == 100 and cx.dtype == code and cx.nch == 2
        assert (nd.i1, nd.i2, nd.i3, nd.s0, nd.s1, nd.d0, nd.d1, nd.d2, nd.d3) == (0,) * 9 and not nd.p0 and not nd.p1


def test_demand_reaches_ahead_and_starts_at_frame_0():
    x = _x(100, 2)
    tree = so.MovingMax(x, 8, ahead=5)
    need = {}
    LW._demand(tree | so.Until(10 * so.frames), 10, need)
    assert need[id(x)] == (15, 0)  # the last frame's window reaches 5 frames further
    need = {}
    LW._demand(tree | so.After(5 * so.frames) | so.Until(10 * so.frames), 10, need)
    assert need[id(x)] == (20, 0)
    need = {}
    LW._demand(tree, 100, need)
    assert need[id(x)] == (100, 0)  # capped by the length of x


def test_the_reference_handles_channels_and_vectors():
    x = np.asfortranarray(np.stack([tied(50, seed=s) for s in range(3)], axis=1))
    y = moving_ref(x, 4, 2)
    assert y.shape == (50, 3) and y.dtype == np.float64
    for c in range(3):
        assert same_bits(y[:, c], moving_loop(x[:, c], 4, 2))
    assert moving_ref(x[:, 0], 4, 2).shape == (50, 1)
