"""`MovingSum(x, w)` / `MovingMean(x, w)` / `MovingRMS(x, w)` above the C-ABI (signals.py, lowering.py): the array form of
the summation tree the device is held to (tests/movingsum_ref.py) checked bit for bit against the scalar loop that states
the definition, against `np.sum` where every order is exact, against `math.fsum` within the derived bound; the identity
-0.0, the extent of infinities and NaN; mean and rms against their one-line definitions; the constructors and their
refusals, the `ToFramerate` rules, the `BlockStream` and shard refusals, the lowered node and `_demand`.  No GPU needed."""
import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import _capi as K
from sigops_amd import engine, sharding
from sigops_amd import lowering as LW
import movingsum_ref as M
from movingsum_ref import aheads, movingsum_ref, movsum_1d, movsum_loop, same_bits

FS = 10 * so.kHz
WINDOWS = [1, 2, 3, 16, 17, 33, 480, 1025, 1026, 2049, 4097, 7 * 1024 + 5]
LONG_LENGTHS = [1023, 1024, 1025, 2049, 3 * 1024 + 77]
CTORS = ((so.MovingSum, "MovingSum", 0), (so.MovingMean, "MovingMean", 1), (so.MovingRMS, "MovingRMS", 2))


def _x(n=100, c=2, dtype=np.float64, fs=FS):
    return so.Signal(np.asfortranarray(np.arange(n * c, dtype=dtype).reshape(c, n).T), fs)


def _clipped(x, n, back, ahead):
    return x[max(0, n - back):min(x.size - 1, n + ahead) + 1]


# ---- 1. the reference ------------------------------------------------------------------------------------------------
def test_the_constants_are_read_from_the_kernel_header():
    R, B, tile, halo = M.kernel_constants()
    assert (R, B) == (M.R, M.B) == (16, 1024) and tile == M.TILE == 2 * B
    assert halo == B and tile + halo + B - 1 <= 4096  # the short form's image: tile, halo and the lead-in to a multiple of S
    assert [M.segment(w) for w in (2, 3, 4, 5, 17, 1024, 1025, 1026, 5000)] == [1, 2, 2, 4, 16, 512, 1024, 1024, 1024]


def test_the_cover_is_canonical():
    assert M.cover(3, 5) == [(0, 4)] and M.cover(3, 4) == []
    assert M.cover(0, 7) == [(0, 1), (1, 1), (1, 2), (0, 6)]
    assert M.cover(-1, 8) == [(3, 0)] and M.cover(-1, 7) == [(2, 0), (1, 2), (0, 6)]
    assert M.cover(-4, 3) == [(0, -3), (1, -1), (1, 0), (0, 2)]  # no node straddles segment 0's first frame
    for a in range(-9, 9):
        for b in range(a + 1, a + 40):
            p = a + 1
            for l, q in M.cover(a, b):
                assert q << l == p and (l == 62 or p % (2 << l) or p + (2 << l) > b)  # aligned, adjacent and maximal
                p += 1 << l
            assert p == b


@pytest.mark.parametrize("w", WINDOWS)
def test_the_array_form_equals_the_scalar_loop_bit_for_bit(w):
    """lengths 1 .. 300 and around one, two and three blocks, every window causal, centred and fully ahead; w > N included"""
    for N in list(range(1, 301)) + LONG_LENGTHS:
        x = M.wide(N, 1, seed=w)[:, 0]
        for ahead in aheads(w):
            assert same_bits(movsum_1d(x, w - 1 - ahead, ahead), movsum_loop(x, w - 1 - ahead, ahead)), (N, w, ahead)


@pytest.mark.parametrize("w", WINDOWS)
def test_small_integers_equal_np_sum_of_the_clipped_window(w):
    """every order of the additions is exact, so the tree must give the plain sum of exactly the window's frames"""
    for N in (1, 2, 15, 16, 17, 100, 300, 1023, 1025, 2049, 3 * 1024 + 77):
        x = M.small_ints(N, 1)[:, 0]
        c = np.concatenate([[0.0], np.cumsum(x)])  # exact
        n = np.arange(N)
        for ahead in aheads(w):
            back = w - 1 - ahead
            want = c[np.minimum(N - 1, n + ahead) + 1] - c[np.maximum(0, n - back)]
            got = movsum_1d(x, back, ahead)
            assert np.array_equal(got, want), (N, w, ahead)
            for k in (0, N // 2, N - 1):
                assert got[k] == np.sum(_clipped(x, k, back, ahead))


@pytest.mark.parametrize("w", WINDOWS)
def test_the_error_against_fsum_stays_within_the_derived_bound(w):
    """data over 2^-60 .. 2^60; the bound is error_units(w) * 2^-53 * sum |window| (movingsum_ref's docstring)"""
    worst = 0.0
    for N in (1, 50, 300, 1025, 3 * 1024 + 77):
        x = M.wide(N, 1, seed=1)[:, 0]
        for ahead in aheads(w):
            back = w - 1 - ahead
            exact, mag = M.fsum_windows(x, back, ahead)
            err = np.abs(movsum_1d(x, back, ahead) - exact)
            unit = mag * 2.0 ** -53
            assert (err <= M.error_units(w) * unit * (1 + 2.0 ** -50)).all(), (N, w, ahead)
            worst = max(worst, float((err / unit).max()))
    print(f"worst error, w={w}: {worst:.2f} of {M.error_units(w):.0f} units")


def test_a_channel_of_negative_zero_sums_to_negative_zero():
    for N in (1, 17, 300, 2049):
        x = np.full(N, -0.0)
        for w in WINDOWS:
            for ahead in aheads(w):
                got = movsum_1d(x, w - 1 - ahead, ahead)
                assert np.signbit(got).all() and not got.any(), (N, w, ahead)
        y = movingsum_ref(x, 7, 3, M.MEAN)
        assert np.signbit(y).all() and not y.any()
        y = movingsum_ref(x, 7, 3, M.RMS)  # (-0.0)^2 = +0.0
        assert not np.signbit(y).any() and not y.any()
    z = np.array([0.0, -0.0, -0.0, 0.0, -0.0])  # a +0.0 anywhere in the window makes the sum +0.0
    assert np.array_equal(np.signbit(movsum_1d(z, 1, 0)), [False, False, True, False, False])


@pytest.mark.parametrize("w", [1, 3, 17, 480, 1026, 2049])
def test_infinities_and_nan_cover_exactly_their_extent(w):
    N = 3 * 1024 + 77
    n = np.arange(N)
    for ahead in aheads(w):
        back = w - 1 - ahead
        x = M.signal(N, 1)[:, 0]
        p, q = 1500, 1500 + min(w - 1, 700)  # +Inf and -Inf within a window's reach of each other
        if p == q:  # (w == 1: no window holds two frames)
            q = p + 1
        x[p], x[q] = np.inf, -np.inf
        got = movsum_1d(x, back, ahead)
        has_p, has_q = (n - back <= p) & (p <= n + ahead), (n - back <= q) & (q <= n + ahead)
        assert np.array_equal(np.isnan(got), has_p & has_q), (w, ahead)
        assert (got[has_p & ~has_q] == np.inf).all() and (got[has_q & ~has_p] == -np.inf).all()
        assert np.isfinite(got[~has_p & ~has_q]).all()
        for v in (np.inf, np.nan):  # a single one
            x = M.signal(N, 1)[:, 0]
            x[1023] = v
            got = movsum_1d(x, back, ahead)
            has = (n - back <= 1023) & (1023 <= n + ahead)
            assert np.array_equal(np.isnan(got) if v != v else got == v, has) and np.isfinite(got[~has]).all(), (w, ahead, v)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_mean_and_rms_are_their_one_line_definitions(dtype):
    for N, w in ((1, 5), (40, 7), (300, 33), (300, 480), (1500, 1026)):
        x = M.signal(N, 2, dtype)
        for ahead in aheads(w):
            back = w - 1 - ahead
            s, mean, rms = (movingsum_ref(x, back, ahead, op) for op in (M.SUM, M.MEAN, M.RMS))
            assert s.dtype == mean.dtype == rms.dtype == np.float64 and s.shape == (N, 2)
            cnt = np.array([len(_clipped(x[:, 0], n, back, ahead)) for n in range(N)], dtype=np.float64)
            assert np.array_equal(cnt, M.counts(N, back, ahead)) and cnt.min() >= 1 and cnt.max() == min(w, N)
            x64 = x.astype(np.float64)
            for c in range(2):
                assert same_bits(s[:, c], movsum_loop(x64[:, c], back, ahead))
                assert same_bits(mean[:, c], s[:, c] / cnt)
                q = movsum_loop(x64[:, c] * x64[:, c], back, ahead)
                assert same_bits(rms[:, c], np.sqrt(q / cnt))
            # edge frames are the mean of what is there
            assert abs(mean[0, 0] - np.mean(x64[:ahead + 1, 0])) <= 1e-12 * (1 + np.abs(x64[:ahead + 1, 0]).sum())
            assert abs(rms[-1, 1] - np.sqrt(np.mean(x64[max(0, N - 1 - back):, 1] ** 2))) <= 1e-12 * (1 + np.abs(x64[:, 1]).max())


def test_the_reference_handles_channels_and_vectors():
    x = M.wide(50, 3)
    y = movingsum_ref(x, 4, 2)
    assert y.shape == (50, 3) and y.dtype == np.float64 and y.flags.f_contiguous
    for c in range(3):
        assert same_bits(y[:, c], movsum_loop(x[:, c], 4, 2))
    assert movingsum_ref(x[:, 0], 4, 2).shape == (50, 1)
    assert same_bits(movingsum_ref(x, 4, 2, one=movsum_loop), y)


# ---- 2. the constructors ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctor,name,op", CTORS)
def test_constructors_and_curried_forms(ctor, name, op):
    x = _x()
    y = ctor(x, 5)
    assert isinstance(y, so.MovingSumSignal) and not isinstance(y, so.MovingSignal)
    assert y.signal is x and (y.back, y.ahead, y.op) == (4, 0, op)
    z = x | ctor(5, ahead=3)
    assert isinstance(z, so.MovingSumSignal) and z.signal is x and (z.back, z.ahead, z.op) == (1, 3, op)
    c = ctor(x, 6, center=True)
    assert (c.back, c.ahead) == (3, 2)
    c = x | ctor(7, center=True)
    assert (c.back, c.ahead) == (3, 3)
    assert (ctor(x, 1).back, ctor(x, 1).ahead) == (0, 0)
    assert (ctor(x, 4, ahead=3).back, ctor(x, 4, ahead=3).ahead) == (0, 3)
    b = np.zeros((100, 2)) | ctor(3)  # a bare array on the left
    assert isinstance(b, so.MovingSumSignal) and b.nch == 2 and b.fs is None
    assert ctor.__name__ == name and name in ctor.__doc__


def test_frames_and_times_give_the_same_node():
    x = _x()  # 10 kHz: 1 ms = 10 frames
    a = so.MovingSum(x, 50, ahead=20)
    for w, ah in ((50 * so.frames, 20 * so.frames), (5 * so.ms, 2 * so.ms), (5 * so.ms, 20), (50.0, 20 * so.frames)):
        b = so.MovingSum(x, w, ahead=ah)
        assert (b.back, b.ahead, b.op) == (a.back, a.ahead, a.op) == (29, 20, 0), (w, ah)
    assert (so.MovingRMS(x, 5 * so.ms, center=True).back, so.MovingRMS(x, 5 * so.ms, center=True).ahead) == (25, 24)


def test_length_rate_channels_and_type():
    x = _x(100, 3, np.float32, fs=44.1 * so.kHz)
    for ctor, _, _ in CTORS:
        y = ctor(x, 9, center=True)
        assert so.nframes(y) == 100 and so.nchannels(y) == 3 and so.framerate(y) == 44_100.0
        assert so.sampletype(y) == np.float64 and so.duration(y) == 100 / 44_100.0  # Float32 widens, as under Cumsum
        assert so.sampletype(ctor(_x(), 3)) == np.float64
    assert so.nframes(so.MovingMean(x | so.Filt(so.Lowpass, 1 * so.kHz), 5)) == 100  # a computed child
    assert so.MovingSum(_x(fs=None), 3).fs is None
    # an infinite x is accepted, and stays infinite
    s = so.Signal(np.sin, FS, ω=5 * so.Hz)
    y = s | so.MovingRMS(2 * so.ms, ahead=1 * so.ms)
    assert isinstance(y, so.MovingSumSignal) and so.signals.isknowninf(so.nframes(y)) and (y.back, y.ahead) == (9, 10)
    assert so.nframes(y | so.Until(300 * so.frames)) == 300


def test_constructor_refusals():
    x = _x()
    cases = [
        (lambda: so.MovingSum(x, 0), "MovingSum", "at least one frame"),
        (lambda: so.MovingMean(x, -3), "MovingMean", "at least one frame"),
        (lambda: so.MovingRMS(x, 2.5), "MovingRMS", "whole number of frames"),
        (lambda: so.MovingSum(x, 5, ahead=1.5), "MovingSum", "whole number of frames"),
        (lambda: so.MovingMean(x, float("nan")), "MovingMean", "whole number of frames"),
        (lambda: so.MovingRMS(x, "5"), "MovingRMS", "whole number of frames"),
        (lambda: so.MovingSum(_x(fs=None), 5 * so.ms), "MovingSum", "needs the frame rate of x"),
        (lambda: np.zeros(10) | so.MovingMean(5 * so.ms), "MovingMean", "needs the frame rate of x"),
        (lambda: so.MovingRMS(_x(fs=None), 5, ahead=1 * so.ms), "MovingRMS", "needs the frame rate of x"),
        (lambda: so.MovingSum(x, 5 * so.Hz), "MovingSum", "neither a time nor a number of frames"),
        (lambda: so.MovingSum(x, 5, ahead=5), "MovingSum", "[0, 4]"),
        (lambda: so.MovingMean(x, 5, ahead=-1), "MovingMean", "[0, 4]"),
        (lambda: so.MovingRMS(x, 5, ahead=2, center=True), "MovingRMS", "not both"),
        (lambda: x | so.MovingSum(5, ahead=0, center=True), "MovingSum", "not both"),
        (lambda: so.MovingSum(so.Signal(np.arange(10), FS), 3), "MovingSum", "Float32 or Float64"),
        (lambda: so.MovingMean(so.Signal(np.arange(10), FS), 3), "MovingMean", "Float32 or Float64"),
        (lambda: so.MovingRMS(so.Signal(np.arange(10), FS), 3), "MovingRMS", "Float32 or Float64"),
        (lambda: so.MovingSum(), "MovingSum", "MovingSum(x, w) expected"),
        (lambda: so.MovingMean(x, 3, 1), "MovingMean", "MovingMean(x, w) expected"),
        (lambda: so.MovingRMS(x, 3, 1), "MovingRMS", "MovingRMS(x, w) expected"),
    ]
    for make, name, words in cases:
        with pytest.raises(so.ErrorException) as e:
            make()
        assert name in str(e.value) and words in str(e.value), str(e.value)
        assert "MovingMax" not in str(e.value)


def test_toframerate():
    y = so.MovingMean(_x(fs=None), 7, ahead=2)  # no rate: it is handed to x, the frame counts stay
    z = so.ToFramerate(y, 8 * so.kHz)
    assert isinstance(z, so.MovingSumSignal) and z.fs == 8000.0 and z.signal.fs == 8000.0 and so.nframes(z) == 100
    assert (z.back, z.ahead, z.op) == (4, 2, 1)
    y = so.MovingRMS(_x(), 7)  # a rate: resampled like any computed signal
    z = so.ToFramerate(y, 20 * so.kHz)
    assert isinstance(z, so.FilteredSignal) and isinstance(z.fn, so.ResamplerFn) and z.signal is y
    assert z.fs == 20_000.0 and so.nframes(z) == 200
    assert so.ToFramerate(y, FS) is y


# ---- 3. refusals above the node --------------------------------------------------------------------------------------
def test_blockstream_and_shards_refuse_the_node_by_name():
    x = _x()
    names = "MovingSum / MovingMean / MovingRMS"
    cases = [
        (lambda: engine._streamable(so.MovingSum(x, 5) | so.Filt(so.Lowpass, 1 * so.kHz)), "BlockStream: " + names, "not streamable"),
        (lambda: engine._streamable(so.Mix(so.MovingRMS(x, 5, center=True), 1.0)), "BlockStream: " + names, "not streamable"),
        (lambda: sharding.shard_time(so.MovingMean(x, 5), 0, 2), "shard_time", names + " over several GPUs is not built"),
        (lambda: sharding.shard_channels(so.Mix(so.MovingRMS(x, 5), 1.0), 0, 2), "shard_channels", names + " over several GPUs is not built"),
        (lambda: sharding.shard_append(so.Append(so.MovingSum(x, 5), so.MovingSum(x, 5)), 0, 2), "shard_append", names + " over several GPUs is not built"),
    ]
    for make, name, words in cases:
        with pytest.raises(so.ErrorException) as e:
            make()
        assert name in str(e.value) and words in str(e.value), str(e.value)
    with pytest.raises(so.ErrorException) as e:  # its own reason, not the extrema's and not the recurrences'
        sharding.shard_time(so.MovingSum(x, 5), 0, 2)
    assert "halo" in str(e.value) and "tree" in str(e.value) and "MovingMax" not in str(e.value) and "every frame before" not in str(e.value)
    with pytest.raises(so.ErrorException) as e:
        engine._streamable(so.MovingSum(x, 5))
    assert "summation tree" in str(e.value) and "MovingMax" not in str(e.value)
    with pytest.raises(so.ErrorException) as e:  # the other refusals still name their nodes
        sharding.shard_time(so.MovingMax(x, 5), 0, 2)
    assert "MovingMax / MovingMin over several GPUs is not built" in str(e.value)


# ---- 4. the lowered node ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,code", [(np.float32, K.SO_F32), (np.float64, K.SO_F64)])
def test_the_lowered_node(dtype, code):
    assert K.NODE_MOVSUM == 16 and K.NODE_MOVING == 15
    x = _x(100, 2, dtype)
    for ctor, _, i0 in CTORS:
        lw = LW.lower(ctor(x, 12, ahead=4))
        nd = lw.nodes[lw.root]
        assert nd.kind == K.NODE_MOVSUM and nd.n_children == 1 and nd.nch == 2 and nd.dtype == K.SO_F64 and nd.nframes == 100 and nd.fs == 10_000.0
        assert (nd.l0, nd.l1, nd.i0) == (7, 4, i0)
        cx = lw.nodes[nd.children[0]]
        assert cx.kind == K.NODE_ARRAY and cx.l0 == 100 and cx.dtype == code and cx.nch == 2
        assert (nd.i1, nd.i2, nd.i3, nd.s0, nd.s1, nd.d0, nd.d1, nd.d2, nd.d3) == (0,) * 9 and not nd.p0 and not nd.p1


def test_the_header_declares_the_node_kind():
    import re
    from pathlib import Path

    text = (Path(__file__).resolve().parent.parent / "include" / "sigops.h").read_text()
    assert re.search(r"SO_NODE_MOVSUM = 16\b", text) and re.search(r"SO_NODE_MOVING = 15,", text)


def test_demand_reaches_ahead_and_starts_at_frame_0():
    x = _x(100, 2)
    tree = so.MovingMean(x, 8, ahead=5)
    need = {}
    LW._demand(tree | so.Until(10 * so.frames), 10, need)
    assert need[id(x)] == (15, 0)  # the last frame's window reaches 5 frames further
    need = {}
    LW._demand(tree | so.After(5 * so.frames) | so.Until(10 * so.frames), 10, need)
    assert need[id(x)] == (20, 0)
    need = {}
    LW._demand(tree, 100, need)
    assert need[id(x)] == (100, 0)  # capped by the length of x
