"""`MovingMedian(x, w)` and `MovingQuantile(x, w, q)` on the device (include/sigops.h SO_NODE_MOVRANK; csrc/k_movrank.hip),
through the public interface and the C-ABI: bit for bit against the NumPy definition (tests/movingmedian_ref.py movrank_ref)
-- no tolerance: a selection rounds nothing.  The definition is held to its scalar restatement without a GPU in
tests/test_movingmedian_host.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import _capi as K
from sigops_amd import lowering as LW
from sigops_amd import signals as S
from sigops_amd.engine import Plan
from oracle_bridge import relerr
from movingmedian_ref import halves, kernel_constants, movrank_ref, same_bits, spikes, tied

pytestmark = pytest.mark.gpu
FS = 10 * so.kHz
T, H = kernel_constants()  # a workgroup's output frames; W - 1 <= H is what is built
WINDOWS = (1, 2, 3, 5, 64, 65, 257, H, H + 1)
QS = (0, 0.1, 0.5, 1)


def bit_equal(got, want, what=""):
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} against {want.dtype} {want.shape}"
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} samples differ, first at {np.argwhere(bad)[0]}"
    assert same_bits(got, want), f"{what}: a zero of the other sign"


def planar(a):
    a = np.asarray(a)
    return np.asfortranarray(a.reshape(a.shape[0], -1))


def sunk(tree):
    """a sub-tree sunk on its own, planar, frames x channels"""
    return planar(so.sink(tree, so.Array))


def check(x, W, ahead, q, what=""):
    got = sunk(so.MovingQuantile(so.Signal(x, FS), W, q, ahead=ahead))
    bit_equal(got, movrank_ref(x, W - 1 - ahead, ahead, q), f"{what} N={x.shape[0]} C={x.shape[1]} {x.dtype.name} W={W} ahead={ahead} q={q}")
    return got


def dev(a):
    """a planar device tensor [frames x channels]"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t()


def close(got, want, what, tol=1e-8):
    """the project's Float64 contract, norm-wise, the observed value printed"""
    assert got.shape == want.shape and got.dtype == want.dtype
    e = relerr(got, want)
    print(f"worst {what}: {e:.3e}")
    assert e <= tol, f"{what}: {e:.3e}"


def _aheads(W):
    return sorted({0, (W - 1) // 2, W - 1})


# ---- 1. geometry -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", WINDOWS)
def test_every_window_meets_every_length(W):
    """every window at the lengths 1, 2, W - 1, W and around the tile; the offset, the quantile, the channel count and the
    sample type take turns, and at T + 1 frames every offset meets every quantile; Gaussian data rounded to halves, so ties
    are common"""
    lengths = sorted({N for N in (1, 2, W - 1, W, T - 1, T, T + 1, 2 * T + 5) if N >= 1})
    turn = itertools.count(WINDOWS.index(W))
    for N in lengths:
        i = next(turn)
        ah = _aheads(W)
        chans = (1, 3, 8) if W < H else (1, 3)  # (the reference sorts every window: eight channels stay with the shorter ones)
        Cn = chans[i % len(chans)]
        dtype = (np.float64, np.float32)[(i // 2) % 2]
        check(halves(N, Cn, dtype, seed=i), W, ah[i % len(ah)], QS[i % 4])
        check(halves(N, 1, dtype, seed=i + 1), W, ah[(i + 1) % len(ah)], QS[(i + 2) % 4])
    x = halves(T + 1, 2, seed=W)
    for ahead in _aheads(W):
        for q in QS:
            check(x, W, ahead, q)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_eight_channels_and_the_quantiles_between(dtype):
    x = halves(2 * T + 5, 8, dtype, seed=5)
    for W, ahead, q in ((5, 2, 0.5), (64, 0, 0.25), (257, 256, 0.3), (257, 128, 0.9)):
        check(x, W, ahead, q)


@pytest.mark.parametrize("make", ["tied", "spikes"])
def test_ties_and_one_spike_a_tile(make):
    """`tied`: few distinct values, zeros of both signs, both infinities and a NaN; `spikes`: one spike a tile at a random
    offset, a different height each, so a wrong tile or halo index shows in the upper quantiles"""
    N = 2 * T + 5
    x = planar(tied(N, seed=1)) if make == "tied" else spikes(N, 3, T)
    for W, ahead in ((5, 2), (257, 0), (H + 1, H // 2), (H + 1, H)):
        for q in (0.5, 0.999, 1):
            check(x, W, ahead, q, make)
    check(np.asfortranarray(x.astype(np.float32)), 65, 32, 0.5, make)


def test_the_ranks_0_and_m_less_1_are_movingmin_and_movingmax_on_the_device():
    N = 2 * T + 5
    for dtype in (np.float64, np.float32):
        x = planar(np.stack([tied(N, dtype, seed=s) for s in range(2)], axis=1))
        xs = so.Signal(x, FS)
        for W, ahead in ((1, 0), (2, 1), (5, 2), (65, 0), (H + 1, 300)):
            bit_equal(sunk(so.MovingQuantile(xs, W, 0, ahead=ahead)), sunk(so.MovingMin(xs, W, ahead=ahead)), f"q = 0, W={W}")
            bit_equal(sunk(so.MovingQuantile(xs, W, 1, ahead=ahead)), sunk(so.MovingMax(xs, W, ahead=ahead)), f"q = 1, W={W}")
        bit_equal(sunk(so.MovingMedian(xs, 1)), x, "W = 1 is x itself")


# ---- 2. planted values ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_planted_zeros_infinities_and_nans(dtype):
    N = 2 * T + 5
    for W, ahead, q in ((1, 0, 0.5), (5, 2, 0.5), (300, 299, 0.1), (H + 1, 7, 0.5), (64, 0, 1)):
        back = W - 1 - ahead
        x = halves(N, 5, dtype, seed=3)
        x[np.abs(x) < 0.75] = 0.0
        for b in (T, 2 * T):  # zeros of both signs on both sides of the tile boundaries
            x[b - 2:b + 2, 0] = (-0.0, 0.0, -0.0, 0.0)
            x[b - 2:b + 2, 1] = (0.0, -0.0, 0.0, -0.0)
        x[:, 2] = -0.0  # a channel of only -0.0
        at = (T - 1, T, None, 0, N - 1)  # one NaN a channel: either side of the tile boundary, the first frame, the last
        for c in (0, 1, 3, 4):
            x[(at[c] + 40) % N, c] = np.inf
            x[(at[c] + 49) % N, c] = -np.inf
            x[at[c], c] = np.nan
        x[0, 1], x[N - 1, 1], x[0, 0], x[N - 1, 0] = np.inf, -np.inf, -0.0, 0.0
        got = check(x, W, ahead, q, "planted")
        assert got.dtype == dtype
        assert np.signbit(got[:, 2]).all() and not got[:, 2].any()  # all -0.0 stays -0.0
        n = np.arange(N)
        for c in (0, 1, 3, 4):  # NaN covers exactly the frames whose window holds it, fewer at the edges
            assert np.array_equal(np.isnan(got[:, c]), (n >= at[c] - ahead) & (n <= at[c] + back)), (W, ahead, c)


# ---- 3. leaf kinds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,ahead,q", [(65, 20, 0.5), (H + 1, 700, 0.1)])
def test_leaf_kinds(W, ahead, q):
    import torch

    N = T + 77
    back = W - 1 - ahead
    for Cn in (1, 3):
        x = halves(N, Cn)
        want = movrank_ref(x, back, ahead, q)
        tree = lambda leaf: so.MovingQuantile(so.Signal(leaf, FS), W, q, ahead=ahead)  # noqa: E731
        x32 = halves(N, Cn, np.float32)
        want32 = movrank_ref(x32, back, ahead, q)
        got = so.sink(tree(x32), so.Array)
        assert got.dtype == np.float32
        bit_equal(planar(got), want32, "a Float32 array")
        bit_equal(planar(so.sink(tree(x), so.Array)), want, "a Fortran-ordered host array")
        xi = np.ascontiguousarray(x)  # frames x channels, C order: frame stride = channels
        bit_equal(planar(so.sink(tree(xi), so.Array)), want, "a C-ordered host array")
        big = np.asfortranarray(np.random.default_rng(5).standard_normal((2 * N, 2 * Cn)))
        big[::2, ::2] = x
        bit_equal(planar(so.sink(tree(big[::2, ::2]), so.Array)), want, "a strided view: every second frame, every second channel")
        got, fs = so.sink(tree(dev(x)), "torch")
        assert fs == 10_000.0 and got.is_cuda and got.dtype == torch.float64
        bit_equal(got.cpu().numpy().reshape(N, Cn), np.ascontiguousarray(want), "a planar device tensor, device result")
        got, fs = so.sink(tree(dev(x32)), "torch")
        assert got.dtype == torch.float32
        bit_equal(got.cpu().numpy().reshape(N, Cn), np.ascontiguousarray(want32), "a planar Float32 device tensor, device result")
        di = torch.from_numpy(xi).cuda()  # interleaved on the device
        bit_equal(planar(so.sink(tree(di), so.Array)), want, "an interleaved device tensor")
        out = torch.full((Cn, N + 1), 7.0, dtype=torch.float64, device="cuda")[:, 1:].t()  # rows that start 8 bytes off a 16-byte boundary
        so.sink_into(out, tree(dev(x)))
        bit_equal(out.cpu().numpy(), np.ascontiguousarray(want), "sink_into a device tensor, unaligned rows")
        bit_equal(planar(so.sink(tree(dev(x)[1:]), so.Array)), movrank_ref(x[1:], back, ahead, q), "a device leaf whose rows start 8 bytes off a 16-byte boundary")
        bit_equal(planar(so.sink(tree(dev(x32)[1:]), so.Array)), movrank_ref(x32[1:], back, ahead, q), "a Float32 device leaf whose rows start 4 bytes off")


# ---- 4. children ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [129, H + 1])
def test_a_sub_tree_as_x(W):
    N = T + 37
    a = (W - 1) // 2
    raw = halves(N + 1000, 2, seed=1)
    xs = so.Signal(raw, FS)
    children = (("a formula", so.Signal(np.sin, FS, ω=50 * so.Hz) | so.Until(N * so.frames)),
                ("a traced map", so.OperateOn(so.elementwise(lambda v: np.abs(v) - 0.5), xs)),
                ("Filt", xs | so.Filt(so.Highpass, 1 * so.kHz)),
                ("Cumsum", so.Cumsum(xs)),
                ("MovingRMS", so.MovingRMS(xs, 480)))
    for name, child in children:
        mid = sunk(child)  # the child, sunk separately
        assert np.isfinite(mid).all() and np.ptp(mid) > 0.1 and mid.shape[0] >= N
        bit_equal(sunk(so.MovingMedian(child, W, center=True)), movrank_ref(mid, W - 1 - a, a, 0.5), f"MovingMedian({name})")
    bit_equal(sunk(so.MovingQuantile(so.MovingRMS(xs, 480), W, 0.1)), movrank_ref(sunk(so.MovingRMS(xs, 480)), W - 1, 0, 0.1), "a noise floor: a low quantile of MovingRMS")


@pytest.mark.parametrize("W,ahead", [(100, 33), (H + 1, 900)])
def test_an_infinite_signal_under_until_above_the_node(W, ahead):
    tree = so.Signal(np.sin, FS, ω=37 * so.Hz) | so.MovingMedian(W, ahead=ahead)
    assert S.isknowninf(so.nframes(tree))
    n = T + 5
    whole = sunk(tree | so.Until(n * so.frames))  # no upper clip: the windows of the last frames read beyond them
    s = sunk(so.Signal(np.sin, FS, ω=37 * so.Hz) | so.Until((n + ahead) * so.frames))
    bit_equal(whole, movrank_ref(s, W - 1 - ahead, ahead, 0.5)[:n], "against the reference over the frames it reads")
    blocks = [np.asarray(b).reshape(len(b), -1) for b in itertools.islice(so.stream(tree, 1000, so.Array), 2)]
    bit_equal(np.vstack(blocks), whole[:2000], "two blocks of an infinite signal")


# ---- 5. windows and streams -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,ahead,q", [(100, 33, 0.5), (H + 1, 900, 0.25)])
def test_windows_and_streams_equal_the_whole_sink(W, ahead, q):
    """the dependence is local: `After` / `Until` / `Window` over the node and `stream` blocks give the slice of the whole
    sink bit for bit, with frames beyond a block's end read for its last windows (`ahead > 0`)"""
    N = 2 * T + 11
    x = halves(N, 2, seed=2)
    back = W - 1 - ahead
    trees = (("array", so.MovingQuantile(so.Signal(x, FS), W, q, ahead=ahead), movrank_ref(x, back, ahead, q)),
             ("map", so.MovingQuantile(so.Amplify(so.Signal(x, FS), 0.25), W, q, ahead=ahead), movrank_ref(np.asfortranarray(x * 0.25), back, ahead, q)))
    for name, tree, want in trees:
        whole = sunk(tree)
        bit_equal(whole, want, name)
        for a, n in ((1, 5), (T - 3, 7), (T, T + 1), (T + 3, T - 1)):
            got = so.sink(tree | so.After(a * so.frames) | so.Until(n * so.frames), so.Array)
            bit_equal(got.reshape(n, -1), whole[a:a + n], f"{name}: After({a}) | Until({n})")
            got = so.sink(tree | so.Window(from_=a * so.frames, to=(a + n) * so.frames), so.Array)
            bit_equal(got.reshape(n, -1), whole[a:a + n], f"{name}: Window({a}, {n})")
        got = so.sink(tree | so.After((T + 1) * so.frames), so.Array)
        bit_equal(got.reshape(N - T - 1, -1), whole[T + 1:], f"{name}: After")
        blocks = np.vstack([np.asarray(b).reshape(len(b), -1) for b in so.stream(tree, 1000, so.Array)])  # (1000 does not divide T)
        bit_equal(blocks, whole, f"{name}: blocks of 1000")


# ---- 6. composites ----------------------------------------------------------------------------------------------------------
def test_under_append_pad_and_mix():
    """two channels and an even first length: the second window of `Append of two` is 16-byte aligned.  Windows at odd frames
    and at every 4-byte phase of a Float32 result, 1 and 3 channels, several readers, windows, blocks and random trees are in
    tests/test_gpu_node_trees.py, against tests/tree_ref.py `evaluate`, which has the node"""
    N = T + 50
    x, y = halves(N, 2, seed=6), halves(700, 2, seed=7)
    xs, ys = so.Signal(x, FS), so.Signal(y, FS)
    for W, ahead, q in ((7, 3, 0.5), (H + 1, 100, 0.9)):
        back = W - 1 - ahead
        med = lambda s: so.MovingQuantile(s, W, q, ahead=ahead)  # noqa: E731
        ref = lambda a: movrank_ref(a, back, ahead, q)  # noqa: E731
        bit_equal(sunk(so.Append(med(xs), med(ys))), np.asfortranarray(np.vstack([ref(x), ref(y)])), "Append of two")
        bit_equal(sunk(med(so.Append(xs, ys))), ref(np.asfortranarray(np.vstack([x, y]))), "over an Append")
        padded = np.asfortranarray(np.vstack([x, np.zeros((300, 2))]))
        bit_equal(sunk(med(xs) | so.Pad(so.zero) | so.Until((N + 300) * so.frames)), np.asfortranarray(np.vstack([ref(x), np.zeros((300, 2))])), "padded")
        bit_equal(sunk(med(xs | so.Pad(so.zero) | so.Until((N + 300) * so.frames))), ref(padded), "over a Pad")
        bit_equal(sunk(so.Mix(xs, med(xs))), np.asfortranarray(x + ref(x)), "Mix(x, .)")


def test_the_hampel_composite():
    """the median and the median absolute deviation: `MovingMedian(|x - MovingMedian(x, 7)|, 7)`, centred, with `elementwise`
    maps (a difference and an absolute value round once or not at all, as NumPy's do)"""
    N = T + 300
    rng = np.random.default_rng(12)
    x = np.asfortranarray(rng.standard_normal((N, 2)) + 20.0 * (rng.random((N, 2)) < 0.01))
    xs = so.Signal(x, FS)
    med = so.MovingMedian(xs, 7, center=True)
    mad = so.MovingMedian(so.OperateOn(so.elementwise(lambda a, b: np.abs(a - b)), xs, med), 7, center=True)
    m = movrank_ref(x, 3, 3, 0.5)
    bit_equal(sunk(med), m, "the median")
    bit_equal(sunk(mad), movrank_ref(np.asfortranarray(np.abs(x - m)), 3, 3, 0.5), "the median absolute deviation")
    click = so.OperateOn(so.elementwise(lambda a, b, d: np.where(np.abs(a - b) > 4.5 * d, b, a)), xs, med, mad)  # the declicker
    bit_equal(sunk(click), np.asfortranarray(np.where(np.abs(x - m) > 4.5 * movrank_ref(np.asfortranarray(np.abs(x - m)), 3, 3, 0.5), m, x)), "the declicked signal")


# ---- 7. consumers -----------------------------------------------------------------------------------------------------------
def test_consumers_behind_the_node():
    """each consumer over the node equals the consumer over the sunk node.  Pointwise maps and `SampleAt` are the same
    operations on the same values whichever way they read them: bit for bit.  `Filt` and `Normpower` choose their chunking
    and reduction order by the plan they are in: the Float64 contract, 1e-8 norm-wise."""
    N = T + 77
    x = halves(N, 2, seed=4)
    xs = so.Signal(x, FS)
    for W, ahead in ((101, 50), (H + 1, 1000)):
        mid = movrank_ref(x, W - 1 - ahead, ahead, 0.5)
        tree = so.MovingMedian(xs, W, ahead=ahead)
        ms = so.Signal(mid, FS)
        bit_equal(sunk(tree), mid)
        half = so.elementwise(lambda v: 0.5 * v + 1.0)
        bit_equal(sunk(so.OperateOn(half, tree)), sunk(so.OperateOn(half, ms)), "Operate: an elementwise closure")
        bit_equal(sunk(so.Amplify(xs, tree)), np.asfortranarray(x * mid), "Amplify(x, .)")
        pos = np.asfortranarray(np.linspace(0.0, N - 1.0, 2000).reshape(-1, 1) + 0.25)
        bit_equal(sunk(so.SampleAt(tree, so.Signal(pos, FS))), sunk(so.SampleAt(ms, so.Signal(pos, FS))), "SampleAt, the node as the table")
        for name, tail in (("Filt(Lowpass)", lambda t: t | so.Filt(so.Lowpass, 1 * so.kHz)), ("Normpower", lambda t: t | so.Normpower)):
            got, want = sunk(tail(tree)), sunk(tail(ms))
            assert np.ptp(want) > 0.1
            close(got, want, f"MovingMedian({W}) | {name}")


# ---- 8. plan reuse and step information ----------------------------------------------------------------------------------
@pytest.mark.parametrize("W,ahead", [(100, 33), (H + 1, 900)])
def test_a_plan_is_reused_after_set_array(W, ahead):
    import torch

    N = T + 3
    back = W - 1 - ahead
    xs = [halves(N, 2, seed=k) for k in range(3)]
    want = [movrank_ref(a, back, ahead, 0.5) for a in xs]
    res = np.zeros((N, 2), order="F")
    p = Plan(so.MovingMedian(so.Signal(xs[0], FS), W, ahead=ahead), res.shape, res.dtype, (1, res.shape[0]), False)
    scratch = p.stats()["scratch_bytes"]
    for k in (0, 1, 1, 2, 0):
        p.set_array(0, xs[k])
        p.execute(res.ctypes.data)
        bit_equal(res, want[k], f"host leaf {k}")
        assert p.stats()["scratch_bytes"] == scratch
    p.close()
    dx = [dev(a) for a in xs]
    out = torch.empty((2, N), dtype=torch.float64, device="cuda").t()
    p = Plan(so.MovingMedian(so.Signal(dx[0], FS), W, ahead=ahead), (N, 2), np.float64, (1, N), True)
    for k in (0, 0, 1, 2, 0):
        p.set_array(0, dx[k])
        p.execute(out.data_ptr())
        p.check()
        bit_equal(out.cpu().numpy(), np.ascontiguousarray(want[k]), f"device leaf {k}")
        s = p.stats()
        assert s["h2d_bytes"] == 0 and s["d2h_bytes"] == 0 and s["scratch_bytes"] <= 4096  # x is read where it lies; nothing besides
    p.close()


def test_step_info_names_the_kernel_and_counts_a_read_and_a_write():
    import torch

    N = 2 * T + 5
    for W in (1, 5, H + 1):
        for dtype, tdtype, esz in ((np.float64, torch.float64, 8), (np.float32, torch.float32, 4)):
            x = dev(halves(N, 3, dtype))
            out = torch.empty((3, N), dtype=tdtype, device="cuda").t()
            p = Plan(so.MovingMedian(so.Signal(x, FS), W), (N, 3), dtype, (1, N), True)
            p.set_profiling(True)
            p.execute(out.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            steps = p.steps()
            p.close()
            assert [s["name"] for s in steps] == ["k_movrank"], steps
            assert steps[0]["algorithmic_bytes"] == 2 * N * 3 * esz and steps[0]["launches"] == 1, (W, steps)
            bit_equal(out.cpu().numpy(), np.ascontiguousarray(movrank_ref(x.cpu().numpy(), W - 1, 0, 0.5)), f"W={W} {np.dtype(dtype).name}")
    # a late window reads the window plus its halo and writes the window, not frames from 0
    x = dev(halves(8 * T, 2))
    a, n, back, ahead = 6 * T + 7, T + 3, 66, 33
    tree = so.MovingMedian(so.Signal(x, FS), 100, ahead=ahead) | so.After(a * so.frames) | so.Until(n * so.frames)
    out = torch.empty((2, n), dtype=torch.float64, device="cuda").t()
    p = Plan(tree, (n, 2), np.float64, (1, n), True)
    p.set_profiling(True)
    p.execute(out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    steps = [s for s in p.steps() if s["name"] == "k_movrank"]
    p.close()
    assert len(steps) == 1 and steps[0]["algorithmic_bytes"] == ((n + back + ahead) + n) * 2 * 8, steps
    bit_equal(out.cpu().numpy(), np.ascontiguousarray(movrank_ref(x.cpu().numpy(), back, ahead, 0.5)[a:a + n]), "the late window")


# ---- 9. malformed node tables -------------------------------------------------------------------------------------------------
def _create(lw, nframes, nch):
    out = K.so_out_desc_t(dtype=K.SO_F64, nch=nch, nframes=nframes, frame_stride=1, chan_stride=nframes, is_device=0)
    plan = C.c_void_p()
    st = K.lib().so_plan_create(lw.nodes, lw.n, lw.root, C.byref(out), 0, C.byref(plan))
    if plan.value:
        K.lib().so_plan_destroy(plan)
    return st, K.last_error() if st else ""


def test_malformed_nodes_are_refused():
    x = so.Signal(halves(64, 3), FS)
    lw = LW.lower(so.MovingQuantile(x, 9, 0.25, ahead=3))
    assert _create(lw, 64, 3)[0] == 0  # the well-formed node
    n = lw.root
    assert lw.nodes[n].kind == K.NODE_MOVRANK == 19
    invalid, unsupported = -1, -3  # include/sigops.h so_status_t: SO_ERR_INVALID, SO_ERR_UNSUPPORTED
    two = (C.c_int32 * 2)(0, 0)
    kids = lw.nodes[n].children
    lw.nodes[n].children = C.cast(two, C.POINTER(C.c_int32))
    lw.nodes[n].n_children = 2
    st, err = _create(lw, 64, 3)
    assert st == invalid and f"node {n}" in err and "Movrank" in err and "one child" in err, err
    lw.nodes[n].n_children = 0
    st, err = _create(lw, 64, 3)
    assert st == invalid and f"node {n}" in err and "Movrank" in err and "one child" in err, err
    lw.nodes[n].children = kids
    lw.nodes[n].n_children = 1
    assert _create(lw, 64, 3)[0] == 0
    for field, bad, good, words in (("l0", -1, 5, "back >= 0"), ("l1", -1, 3, "ahead >= 0"), ("d0", -0.25, 0.25, "q in [0, 1]"),
                                    ("d0", 1.5, 0.0, "q in [0, 1]"), ("d0", float("nan"), 1.0, "q in [0, 1]"), ("d0", float("inf"), 0.5, "q in [0, 1]")):
        setattr(lw.nodes[n], field, bad)
        st, err = _create(lw, 64, 3)
        assert st == invalid and f"node {n}" in err and "Movrank" in err and words in err, (field, err)
        setattr(lw.nodes[n], field, good)
        assert _create(lw, 64, 3)[0] == 0
    # an integer child (the host refuses to build it: the node is made by hand)
    st, err = _create(LW.lower(S.MovingRankSignal(so.Signal(5, FS) | so.Until(64 * so.frames), 2, 1, 0.5)), 64, 1)  # an Int64 constant
    assert st == unsupported and "Movrank" in err and "Float32 or Float64" in err, err
    # a window longer than the one form that is built, on a signal long enough to hold it
    long = so.Signal(halves(3 * H, 1), FS)
    for back, ahead in ((H + 1, 0), (0, H + 1), (H // 2 + 1, H // 2)):
        st, err = _create(LW.lower(S.MovingRankSignal(long, back, ahead, 0.5)), 3 * H, 1)
        assert st == unsupported and "Movrank" in err and f"at most {H + 1} frames" in err, err
    assert _create(LW.lower(S.MovingRankSignal(long, H, 0, 0.5)), 3 * H, 1)[0] == 0
    # ... and a window longer than the signal is the signal: its clipped reach fits
    short = so.Signal(halves(100, 1), FS)
    assert _create(LW.lower(S.MovingRankSignal(short, 5000, 5000, 0.5)), 100, 1)[0] == 0
    bit_equal(sunk(so.MovingMedian(short, 5001, center=True)), movrank_ref(halves(100, 1), 2500, 2500, 0.5), "the whole signal's lower median")
