"""`MovingSum(x, w)`, `MovingMean(x, w)` and `MovingRMS(x, w)` on the device (include/sigops.h SO_NODE_MOVSUM;
csrc/k_movsum.hip), through the public interface and the C-ABI: bit for bit against the definition's array form
(tests/movingsum_ref.py movingsum_ref) -- no tolerance: the summation tree is fixed by the absolute frame numbers, so the
kernel's runs, scans, block totals, dyadic nodes and covers must give the definition's bits, and the division and the
square root are each rounded once.  The definition is held to its scalar restatement, to `np.sum` and to `math.fsum`
without a GPU in tests/test_movingsum_host.py."""
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
import movingsum_ref as M
from moving_ref import moving_ref
from movingsum_ref import B, LENGTHS, LONG_WINDOWS, SHORT_WINDOWS, TILE, aheads, movingsum_ref, same_bits

pytestmark = pytest.mark.gpu
FS = 10 * so.kHz
CTORS = (so.MovingSum, so.MovingMean, so.MovingRMS)
NAMES = ("sum", "mean", "rms")


def bit_equal(got, want, what=""):
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} against {want.dtype} {want.shape}"
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {np.count_nonzero(bad)} samples differ, first at {at}: {got[at]!r} against {want[at]!r}")
    assert same_bits(got, want), f"{what}: a zero of the other sign"


def planar(a):
    a = np.asarray(a)
    return np.asfortranarray(a.reshape(a.shape[0], -1))


def sunk(tree):
    """a sub-tree sunk on its own, planar, frames x channels"""
    return planar(so.sink(tree, so.Array))


def check(x, W, ahead, op=0, what=""):
    got = sunk(CTORS[op](so.Signal(x, FS), W, ahead=ahead))
    bit_equal(got, movingsum_ref(x, W - 1 - ahead, ahead, op), f"{what} {NAMES[op]} N={x.shape[0]} C={x.shape[1]} {x.dtype.name} W={W} ahead={ahead}")
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


def test_the_tests_cross_the_kernels_switches():
    R, Bk, tile, halo = M.kernel_constants()
    assert (R, Bk, tile) == (M.R, B, TILE)
    assert max(SHORT_WINDOWS) - 1 == halo and min(LONG_WINDOWS) - 1 == halo + 1  # the short form's last window, the long form's first


# ---- 1. geometry -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", LENGTHS)
def test_every_length_window_and_offset(N):
    """lengths around a run, a block and a tile and two of several tiles; the short form's windows (1, inside a run, the
    run, two runs, its last) and the long form's (covers of one, two and three nodes over levels 0 .. 2, and longer than the
    signal), each causal, centred and fully ahead; 1 / 3 / 8 channels, the three operations and both sample types taken in
    turn over data whose magnitudes span 2^-60 .. 2^60, so any other order of the additions shows"""
    data = {(Cn, dt): M.wide(N, Cn).astype(dt) for Cn in M.CHANNELS for dt in (np.float64, np.float32)}
    turn = itertools.count()
    for W in SHORT_WINDOWS + LONG_WINDOWS + [N + 5]:
        for ahead in aheads(W):
            k = next(turn)
            Cn, op, dt = M.CHANNELS[k % 3], (k // 3) % 3, (np.float64, np.float32)[(k // 9) % 2]
            check(data[(Cn, dt)], W, ahead, op)
            if op != 0:  # the sum itself wherever a mean or an rms was taken
                check(data[(Cn, np.float64)], W, ahead, 0)


@pytest.mark.parametrize("op", [0, 1, 2])
@pytest.mark.parametrize("Cn", M.CHANNELS)
def test_every_operation_and_channel_count_in_both_forms(op, Cn):
    for N in (TILE + 1, 3 * TILE + 77):
        x = M.signal(N, Cn)
        for W, ahead in ((17, 5), (480, 0), (1025, 1024), (1026, 513), (4097, 4096), (7 * 1024 + 5, 0)):
            check(x, W, ahead, op, "gaussian")


# ---- 2. planted values ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_planted_zeros_infinities_and_nans(dtype):
    """+-0 on both sides of run, segment, block and tile boundaries, +Inf and -Inf three frames apart in one channel (NaN
    exactly where a window holds both), one Inf or NaN in others, a channel of -0.0"""
    N = 3 * TILE + 77
    x = M.planted(N, 6, dtype)
    n = np.arange(N)
    for W, ahead in ((1, 0), (5, 2), (33, 32), (480, 100), (1025, 7), (1026, 1000), (2050, 0), (7 * 1024 + 5, 3000)):
        back = W - 1 - ahead
        for op in (0, 1, 2):
            got = check(x, W, ahead, op, "planted")
            z = got[:, 5]
            assert not z.any() and np.signbit(z).all() == (op != 2)  # -0.0 stays -0.0; its squares are +0.0
        got = check(x, W, ahead, 0, "planted")
        for c in range(5):
            bad = np.flatnonzero(~np.isfinite(x[:, c]))
            holds = [(n - back <= at) & (at <= n + ahead) for at in bad]
            anynf = np.logical_or.reduce(holds)
            assert np.array_equal(~np.isfinite(got[:, c]), anynf), (W, ahead, c)  # an Inf or NaN covers exactly its extent
            if c % 3 == 1:  # +Inf and -Inf: NaN exactly over the frames whose window holds both
                assert len(bad) == 2 and np.array_equal(np.isnan(got[:, c]), holds[0] & holds[1]), (W, ahead, c)


# ---- 3. leaf kinds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,ahead", [(65, 20), (1026, 700)])
def test_leaf_kinds(W, ahead):
    import torch

    N = 2 * TILE + 77
    back = W - 1 - ahead
    for Cn, op in ((1, 0), (3, 2)):
        x = M.wide(N, Cn)
        want = movingsum_ref(x, back, ahead, op)
        tree = lambda leaf: CTORS[op](so.Signal(leaf, FS), W, ahead=ahead)  # noqa: E731
        x32 = x.astype(np.float32)
        want32 = movingsum_ref(x32, back, ahead, op)
        got = so.sink(tree(x32), so.Array)
        assert got.dtype == np.float64  # a Float32 leaf widens
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
        assert got.dtype == torch.float64
        bit_equal(got.cpu().numpy().reshape(N, Cn), np.ascontiguousarray(want32), "a planar Float32 device tensor, device result")
        di = torch.from_numpy(xi).cuda()  # interleaved on the device
        bit_equal(planar(so.sink(tree(di), so.Array)), want, "an interleaved device tensor")
        out = torch.full((Cn, N + 1), 7.0, dtype=torch.float64, device="cuda")[:, 1:].t()  # rows that start 8 bytes off a 16-byte boundary
        so.sink_into(out, tree(dev(x)))
        bit_equal(out.cpu().numpy(), np.ascontiguousarray(want), "sink_into a device tensor, unaligned rows")
        bit_equal(planar(so.sink(tree(dev(x)[1:]), so.Array)), movingsum_ref(x[1:], back, ahead, op), "a device leaf whose rows start 8 bytes off a 16-byte boundary")
        bit_equal(planar(so.sink(tree(dev(x32)[3:]), so.Array)), movingsum_ref(x32[3:], back, ahead, op), "a Float32 device leaf whose rows start 12 bytes off")
    s = so.Signal(np.sin, FS, ω=50 * so.Hz) | so.Until(N * so.frames)
    bit_equal(sunk(so.MovingSum(s, W, ahead=ahead)), movingsum_ref(sunk(s), back, ahead), "a formula")


@pytest.mark.parametrize("W", [129, 1026])
def test_a_sub_tree_as_x(W):
    N = 2 * TILE + 37
    raw = M.signal(N + 1000, 2, seed=1)
    a = (W - 1) // 2
    children = (("Filt", so.Signal(raw, FS) | so.Filt(so.Highpass, 1 * so.kHz)),
                ("ToFramerate", so.Signal(raw, FS) | so.ToFramerate(12 * so.kHz)),
                ("Cumsum", so.Cumsum(so.Signal(raw, FS))),
                ("MovingMax", so.MovingMax(so.Signal(raw, FS), 77, center=True)),
                ("a Float32 MovingMin", so.MovingMin(so.Signal(raw.astype(np.float32), FS), 77)),
                ("a map", so.Amplify(so.Signal(raw, FS), 0.25)))
    for k, (name, child) in enumerate(children):
        mid = sunk(child)  # the child, sunk separately
        assert np.isfinite(mid).all() and np.ptp(mid) > 0.1 and mid.shape[0] > N
        op = k % 3
        bit_equal(sunk(CTORS[op](child, W, center=True)), movingsum_ref(mid, W - 1 - a, a, op), f"{NAMES[op]}({name})")


# ---- 4. absolute alignment: windows and streams ---------------------------------------------------------------------------
@pytest.mark.parametrize("W,ahead", [(100, 33), (1025, 512), (1026, 900), (3 * TILE, 3 * TILE - 1), (7 * 1024 + 5, 2000)])
def test_windows_and_streams_equal_the_whole_sink(W, ahead):
    """the tree is fixed by the frame numbers of x, not by the frames asked for: `After(k)` for offsets that are no multiple
    of a run, a segment, a block or a tile, `Until`, `Window` and `stream` blocks give the slice of the whole sink bit for
    bit, with frames beyond a block's end read for its last windows (`ahead > 0`)"""
    N = 4 * TILE + 11
    x = M.wide(N, 2, seed=2)
    back = W - 1 - ahead
    op = W % 3
    ctor = CTORS[op]
    amp = np.asfortranarray(x * 0.25)
    trees = (("array", ctor(so.Signal(x, FS), W, ahead=ahead), movingsum_ref(x, back, ahead, op)),
             ("formula", so.Signal(np.sin, FS, ω=50 * so.Hz) | so.Until(N * so.frames) | ctor(W, ahead=ahead), None),
             ("map", ctor(so.Amplify(so.Signal(x, FS), 0.25), W, ahead=ahead), movingsum_ref(amp, back, ahead, op)))
    for name, tree, want in trees:
        whole = sunk(tree)
        if want is not None:
            bit_equal(whole, want, name)
        for k in (1, 15, 1000, 1025, 2049):
            got = so.sink(tree | so.After(k * so.frames), so.Array)
            bit_equal(got.reshape(N - k, -1), whole[k:], f"{name}: After({k})")
        for a, n in ((1, 5), (TILE + 3, TILE + 1), (B - 1, 2 * TILE), (3 * TILE + 5, TILE)):
            got = so.sink(tree | so.After(a * so.frames) | so.Until(n * so.frames), so.Array)
            bit_equal(got.reshape(n, -1), whole[a:a + n], f"{name}: After({a}) | Until({n})")
            got = so.sink(tree | so.Window(from_=a * so.frames, to=(a + n) * so.frames), so.Array)
            bit_equal(got.reshape(n, -1), whole[a:a + n], f"{name}: Window({a}, {n})")
        got = so.sink(tree | so.Until((TILE + 3) * so.frames), so.Array)
        bit_equal(got.reshape(TILE + 3, -1), whole[:TILE + 3], f"{name}: Until")
        for bs in (1000, TILE):
            blocks = np.vstack([np.asarray(b).reshape(len(b), -1) for b in so.stream(tree, bs, so.Array)])
            bit_equal(blocks, whole, f"{name}: blocks of {bs}")


@pytest.mark.parametrize("W,ahead", [(100, 33), (1026, 900), (4097, 1000)])
def test_a_stream_over_an_infinite_signal(W, ahead):
    for op in (0, 2):
        tree = so.Signal(np.sin, FS, ω=37 * so.Hz) | CTORS[op](W, ahead=ahead)
        assert S.isknowninf(so.nframes(tree))
        bs = TILE + 5
        whole = sunk(tree | so.Until(3 * bs * so.frames))  # no upper clip: the windows of the last frames read beyond them
        blocks = [np.asarray(b).reshape(len(b), -1) for b in itertools.islice(so.stream(tree, bs, so.Array), 3)]
        assert [len(b) for b in blocks] == [bs] * 3
        bit_equal(np.vstack(blocks), whole, "three blocks of an infinite signal")
        s = sunk(so.Signal(np.sin, FS, ω=37 * so.Hz) | so.Until((3 * bs + ahead) * so.frames))
        bit_equal(whole, movingsum_ref(s, W - 1 - ahead, ahead, op)[:3 * bs], "against the reference over the frames it reads")


def test_a_late_window_computes_its_own_range_only():
    """step information: the stage of a late window reads the window plus its halo and writes the window, not frames from 0"""
    import torch

    N = 40 * TILE
    xh = M.wide(N, 2)
    x = dev(xh)
    for W, ahead in ((100, 33), (1026, 900), (5 * 1024 + 3, 1000)):
        back = W - 1 - ahead
        a, n = 30 * TILE + 7, TILE + 3
        tree = so.MovingMean(so.Signal(x, FS), W, ahead=ahead) | so.After(a * so.frames) | so.Until(n * so.frames)
        out = torch.empty((2, n), dtype=torch.float64, device="cuda").t()
        p = Plan(tree, (n, 2), np.float64, (1, n), True)
        p.set_profiling(True)
        p.execute(out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        steps = [s for s in p.steps() if s["name"] == "k_movsum"]
        p.close()
        assert len(steps) == 1 and steps[0]["algorithmic_bytes"] == ((n + back + ahead) + n) * 2 * 8, steps
        bit_equal(out.cpu().numpy(), np.ascontiguousarray(movingsum_ref(xh, back, ahead, M.MEAN)[a:a + n]), f"the late window W={W}")


# ---- 5. consumers -----------------------------------------------------------------------------------------------------------
def test_consumers_behind_the_node():
    """each consumer over the node equals the consumer over the sunk node.  Pointwise maps and `SampleAt` are the same
    operations on the same values whichever way they read them: bit for bit.  `Filt`, `ToFramerate` and `Normpower`
    choose their chunking, tables and reduction order by the plan they are in: the Float64 contract, 1e-8 norm-wise."""
    N = 3 * TILE + 77
    x = M.signal(N, 2, seed=4)
    xs = so.Signal(x, FS)
    for W, ahead, op in ((101, 50, 1), (1026, 1000, 2)):
        mid = movingsum_ref(x, W - 1 - ahead, ahead, op)
        tree = CTORS[op](xs, W, ahead=ahead)
        ms = so.Signal(mid, FS)
        bit_equal(sunk(tree), mid)
        bit_equal(sunk(so.Mix(xs, tree)), np.asfortranarray(x + mid), "Mix(x, .)")
        bit_equal(sunk(so.Amplify(xs, tree)), np.asfortranarray(x * mid), "Amplify(x, .)")
        half = so.elementwise(lambda v: 0.5 * v + 1.0)
        bit_equal(sunk(so.OperateOn(half, tree)), sunk(so.OperateOn(half, ms)), "an elementwise closure")
        pos = np.asfortranarray(np.linspace(0.0, N - 1.0, 2000).reshape(-1, 1) + 0.25)
        bit_equal(sunk(so.SampleAt(tree, so.Signal(pos, FS))), sunk(so.SampleAt(ms, so.Signal(pos, FS))), "SampleAt, the node as the table")
        for name, tail in (("Filt(Lowpass)", lambda t: t | so.Filt(so.Lowpass, 1 * so.kHz)),
                           ("ToFramerate", lambda t: t | so.ToFramerate(12 * so.kHz)),
                           ("Normpower", lambda t: t | so.Normpower)):
            got, want = sunk(tail(tree)), sunk(tail(ms))
            assert np.ptp(want) > 0.1
            close(got, want, f"{NAMES[op]}({W}) | {name}")


def test_a_look_ahead_limiter_stays_on_the_device():
    """|x| -> peak hold over the next 50 frames -> moving average of the same length -> gain curve, applied to x delayed by
    the look-ahead: the peak and the smoothed envelope bit for bit against the reference forms, and the chain with the nodes
    against the same chain fed the reference's envelope as an array (maps over the same values: bit for bit)"""
    N = 3 * TILE + 77
    rng = np.random.default_rng(11)
    x = np.asfortranarray(rng.standard_normal((N, 2)) * (1.0 + 3.0 * (rng.random((N, 1)) < 0.002)))
    xs = so.Signal(x, FS)
    rect = so.OperateOn(so.elementwise(lambda v: np.abs(v)), xs)
    curve = so.elementwise(lambda e: np.minimum(1.0, 1.5 / np.maximum(e, 1e-9)))

    def chain(env):
        return so.Amplify(so.Delay(xs, 5 * so.ms), so.OperateOn(curve, env))

    peak = so.MovingMax(rect, 51, ahead=5 * so.ms)
    env = so.MovingMean(peak, 51)
    assert (peak.back, peak.ahead, env.back, env.ahead) == (0, 50, 50, 0)
    want_peak = moving_ref(np.asfortranarray(np.abs(x)), 0, 50)
    want_env = movingsum_ref(want_peak, 50, 0, M.MEAN)
    bit_equal(sunk(peak), want_peak, "the peak envelope")
    bit_equal(sunk(env), want_env, "the smoothed envelope")
    got, want = sunk(chain(env)), sunk(chain(so.Signal(want_env, FS)))
    assert np.ptp(want) > 1.0
    bit_equal(got, want, "the limiter")


# ---- 6. plan reuse and step information ----------------------------------------------------------------------------------
@pytest.mark.parametrize("W,ahead", [(100, 33), (1026, 900), (4097, 0)])
def test_a_plan_is_reused_after_set_array(W, ahead):
    import torch

    N = 3 * TILE + 3
    back = W - 1 - ahead
    xs = [M.wide(N, 2, seed=k) for k in range(3)]
    res = np.zeros((N, 2), order="F")
    p = Plan(so.MovingRMS(so.Signal(xs[0], FS), W, ahead=ahead), res.shape, res.dtype, (1, res.shape[0]), False)
    scratch = p.stats()["scratch_bytes"]
    for k in (0, 0, 0, 1, 1, 2, 0):  # three executes of the same input, then others
        p.set_array(0, xs[k])
        p.execute(res.ctypes.data)
        bit_equal(res, movingsum_ref(xs[k], back, ahead, M.RMS), f"host leaf {k}")
        assert p.stats()["scratch_bytes"] == scratch
    p.close()
    dx = [dev(a) for a in xs]
    out = torch.empty((2, N), dtype=torch.float64, device="cuda").t()
    p = Plan(so.MovingSum(so.Signal(dx[0], FS), W, ahead=ahead), (N, 2), np.float64, (1, N), True)
    for k in (0, 0, 0, 1, 1, 2, 2, 0):
        p.set_array(0, dx[k])
        p.execute(out.data_ptr())
        p.check()
        bit_equal(out.cpu().numpy(), np.ascontiguousarray(movingsum_ref(xs[k], back, ahead)), f"device leaf {k}")
        s = p.stats()
        assert s["h2d_bytes"] == 0 and s["d2h_bytes"] == 0 and s["scratch_bytes"] <= 4096  # x is read where it lies; the table
    p.close()


def test_step_info_names_the_kernel_and_counts_a_read_and_a_write():
    import torch

    N = 5 * TILE + 5
    # (W - 1) // B = 1, 2, 4 .. 7 whole blocks at most: the table's levels 0, 0-1, 0-2
    for W, launches in ((100, 1), (1025, 1), (1026, 2), (2 * B + 5, 3), (4 * B + 5, 4), (7 * B + 5, 4)):
        for dtype, esz in ((np.float64, 8), (np.float32, 4)):
            xh = M.signal(N, 3, dtype)
            x = dev(xh)
            out = torch.empty((3, N), dtype=torch.float64, device="cuda").t()
            p = Plan(so.MovingSum(so.Signal(x, FS), W), (N, 3), np.float64, (1, N), True)
            p.set_profiling(True)
            p.execute(out.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            steps = p.steps()
            p.close()
            assert [s["name"] for s in steps] == ["k_movsum"], steps
            assert steps[0]["algorithmic_bytes"] == N * 3 * (esz + 8) and steps[0]["launches"] == launches, (W, steps)
            bit_equal(out.cpu().numpy(), np.ascontiguousarray(movingsum_ref(xh, W - 1, 0)), f"W={W} {np.dtype(dtype).name}")


# ---- 7. malformed node tables -------------------------------------------------------------------------------------------------
def _create(lw, nframes, nch):
    out = K.so_out_desc_t(dtype=K.SO_F64, nch=nch, nframes=nframes, frame_stride=1, chan_stride=nframes, is_device=0)
    plan = C.c_void_p()
    st = K.lib().so_plan_create(lw.nodes, lw.n, lw.root, C.byref(out), 0, C.byref(plan))
    if plan.value:
        K.lib().so_plan_destroy(plan)
    return st, K.last_error() if st else ""


def test_malformed_nodes_are_refused():
    x = so.Signal(M.signal(64, 3), FS)
    lw = LW.lower(so.MovingMean(x, 9, ahead=3))
    assert _create(lw, 64, 3)[0] == 0  # the well-formed node
    n = lw.root
    assert lw.nodes[n].kind == K.NODE_MOVSUM == 16
    invalid, unsupported = -1, -3  # include/sigops.h so_status_t: SO_ERR_INVALID, SO_ERR_UNSUPPORTED
    two = (C.c_int32 * 2)(0, 0)
    kids = lw.nodes[n].children
    lw.nodes[n].children = C.cast(two, C.POINTER(C.c_int32))
    lw.nodes[n].n_children = 2
    st, err = _create(lw, 64, 3)
    assert st == invalid and f"node {n}" in err and "Movsum" in err and "one child" in err, err
    lw.nodes[n].n_children = 0
    st, err = _create(lw, 64, 3)
    assert st == invalid and f"node {n}" in err and "Movsum" in err and "one child" in err, err
    lw.nodes[n].children = kids
    lw.nodes[n].n_children = 1
    assert _create(lw, 64, 3)[0] == 0
    for field, bads, good, words in (("l0", (-1,), 5, "back >= 0"), ("l1", (-1,), 3, "ahead >= 0"), ("i0", (3, -1), 1, "a sum (0), a mean (1) or an rms (2)")):
        for bad in bads:
            setattr(lw.nodes[n], field, bad)
            st, err = _create(lw, 64, 3)
            assert st == invalid and f"node {n}" in err and "Movsum" in err and words in err, (field, err)
        setattr(lw.nodes[n], field, good)
        assert _create(lw, 64, 3)[0] == 0
    for i0 in (0, 2):
        lw.nodes[n].i0 = i0
        assert _create(lw, 64, 3)[0] == 0
    # an integer child (the host refuses to build it: the node is made by hand)
    st, err = _create(LW.lower(S.MovingSumSignal(so.Signal(5, FS) | so.Until(64 * so.frames), 2, 1, 0)), 64, 1)  # an Int64 constant
    assert st == unsupported and "Movsum" in err and "Float32 or Float64" in err, err
