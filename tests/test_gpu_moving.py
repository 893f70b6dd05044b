"""`MovingMax(x, w)` and `MovingMin(x, w)` on the device (include/sigops.h SO_NODE_MOVING; csrc/k_moving.hip), through the
public interface and the C-ABI: bit for bit against the NumPy definition (tests/moving_ref.py moving_ref) -- no tolerance:
maximum and minimum round nothing, so every decomposition the kernel chooses must give the definition's bits.  The
definition is held to its scalar restatement without a GPU in tests/test_moving_host.py."""
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
from moving_ref import halves, kernel_constants, moving_ref, same_bits, spikes

pytestmark = pytest.mark.gpu
FS = 10 * so.kHz
T, H = kernel_constants()  # a workgroup's output frames; W - 1 <= H is the one-launch form


def bit_equal(got, want, what=""):
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} against {want.dtype} {want.shape}"
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} samples differ, first at {np.argwhere(bad)[0]}"
    assert same_bits(got, want), f"{what}: a zero of the other sign"


def planar(a):
    a = np.asarray(a)
    return np.asfortranarray(a.reshape(a.shape[0], -1))


def check(x, W, ahead, is_min=False, what=""):
    ctor = so.MovingMin if is_min else so.MovingMax
    got = planar(so.sink(ctor(so.Signal(x, FS), W, ahead=ahead), so.Array))
    bit_equal(got, moving_ref(x, W - 1 - ahead, ahead, is_min), f"{what} {'min' if is_min else 'max'} N={x.shape[0]} C={x.shape[1]} W={W} ahead={ahead}")
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


def sunk(tree):
    """a sub-tree sunk on its own, planar, frames x channels"""
    return planar(so.sink(tree, so.Array))


def test_the_two_forms_meet_where_the_tests_say():
    assert T >= 64 and T & (T - 1) == 0 and H >= T - 1


# ---- 1. geometry -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, T - 1, T, T + 1, 2 * T + 1, 3 * T + 77])
def test_every_length_window_and_offset(N):
    """lengths around the tile, windows around every switch (1, a lane's run of 16 keys, the halo H and H + 1 between the
    two forms, the tile, the signal's own length and beyond), the window's offset from causal to anti-causal, 1 / 3 / 8
    channels, maximum and minimum; Gaussian data rounded to halves, so ties are common"""
    data = {Cn: halves(N, Cn) for Cn in (1, 3, 8)}
    # (16, 17, 18 and 32, 33, 34: the short form's segments of 8 / 16 / 32 keys -- inside a lane's run of 16, the run itself,
    #  the first that spans two lanes)
    windows = sorted({W for W in (1, 2, 3, 16, 17, 18, 32, 33, 34, 64, 65, H, H + 1, H + 2, T, T + 1, 2 * T + 3, N - 1, N, N + 5, 10 * N) if W >= 1})
    for W in windows:
        for ahead in sorted({0, min(1, W - 1), (W - 1) // 2, W - 1}):
            for Cn in (1, 3, 8):
                for is_min in (False, True):
                    check(data[Cn], W, ahead, is_min)


# ---- 2. the long form's table ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", ["halves", "spikes"])
def test_the_long_form_reads_every_table_level(make):
    """the whole blocks between a window's first and last block number 1, 2-3 and 5-6 (and all of them), so levels 0, 1
    and 2 of the table are read; one spike a block at a random offset shows a wrong block index"""
    N = 9 * T + 5
    x = halves(N, 3) if make == "halves" else spikes(N, 3, T)
    for W in (2 * T + 1, 4 * T + 1, 7 * T, 9 * T + 5):
        for ahead in (0, W // 2, W - 1):
            for is_min in (False, True):
                check(x if not is_min else np.asfortranarray(-x), W, ahead, is_min, make)


# ---- 3. planted values ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_planted_zeros_infinities_and_nans(dtype):
    N = 3 * T + 77
    for W, ahead in ((1, 0), (5, 2), (300, 299), (H + 1, 7), (H + 2, 1000), (2 * T + 3, T)):
        back = W - 1 - ahead
        x = halves(N, 4, dtype, seed=3)
        x[np.abs(x) < 0.75] = 0.0
        for b in (T, 2 * T, 3 * T):  # zeros of both signs on both sides of the tile boundaries
            x[b - 2:b + 2, 0] = (-0.0, 0.0, -0.0, 0.0)
            x[b - 2:b + 2, 1] = (0.0, -0.0, 0.0, -0.0)
        x[:, 2] = -0.0  # a channel of only -0.0
        at = (T - 1, T, 2 * T + 5, N - 1)
        for c in (0, 1, 3):
            x[at[c] // 2, c] = np.inf
            x[at[c] // 2 + 9, c] = -np.inf
            x[at[c], c] = np.nan  # one NaN a channel
        for is_min in (False, True):
            got = check(x, W, ahead, is_min, f"planted {np.dtype(dtype).name}")
            assert got.dtype == dtype
            assert np.signbit(got[:, 2]).all() and not got[:, 2].any()  # all -0.0 stays -0.0
            for c in (0, 1, 3):  # NaN covers exactly the frames whose window holds it, fewer at the edges
                n = np.arange(N)
                assert np.array_equal(np.isnan(got[:, c]), (n >= at[c] - ahead) & (n <= at[c] + back)), (W, ahead, c)


# ---- 4. leaf kinds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,ahead", [(65, 20), (H + 2, 700)])
def test_leaf_kinds(W, ahead):
    import torch

    N = 2 * T + 77
    back = W - 1 - ahead
    for Cn in (1, 3):
        x = halves(N, Cn)
        want = moving_ref(x, back, ahead)
        tree = lambda leaf: so.MovingMax(so.Signal(leaf, FS), W, ahead=ahead)  # noqa: E731
        x32 = halves(N, Cn, np.float32)
        want32 = moving_ref(x32, back, ahead)
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
        bit_equal(planar(so.sink(tree(dev(x)[1:]), so.Array)), moving_ref(x[1:], back, ahead), "a device leaf whose rows start 8 bytes off a 16-byte boundary")
        bit_equal(planar(so.sink(tree(dev(x32)[3:]), so.Array)), moving_ref(x32[3:], back, ahead), "a Float32 device leaf whose rows start 12 bytes off")
    s = so.Signal(np.sin, FS, ω=50 * so.Hz) | so.Until(N * so.frames)
    bit_equal(sunk(so.MovingMax(s, W, ahead=ahead)), moving_ref(sunk(s), back, ahead), "a formula")


@pytest.mark.parametrize("W", [129, H + 2])
def test_a_sub_tree_as_x_and_an_opening(W):
    N = 2 * T + 37
    raw = halves(N + 1000, 2, seed=1)
    children = (("Filt", so.Signal(raw, FS) | so.Filt(so.Highpass, 1 * so.kHz)),
                ("ToFramerate", so.Signal(raw, FS) | so.ToFramerate(12 * so.kHz)),
                ("Cumsum", so.Cumsum(so.Signal(raw, FS))),
                ("Comb", so.Comb(so.Signal(raw, FS), 257, 0.7)),
                ("a map", so.Amplify(so.Signal(raw, FS), 0.25)))
    for name, child in children:
        mid = sunk(child)  # the child, sunk separately
        assert np.isfinite(mid).all() and np.ptp(mid) > 0.1 and mid.shape[0] > N
        bit_equal(sunk(so.MovingMin(child, W, center=True)), moving_ref(mid, W - 1 - (W - 1) // 2, (W - 1) // 2, True), f"MovingMin({name})")
    xs = so.Signal(raw, FS)
    a = (W - 1) // 2
    opening = so.MovingMax(so.MovingMin(xs, W, center=True), W, center=True)
    bit_equal(sunk(opening), moving_ref(moving_ref(raw, W - 1 - a, a, True), W - 1 - a, a, False), "an opening")


# ---- 5. windows and streams -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,ahead", [(100, 33), (H + 2, 900), (3 * T, 3 * T - 1)])
def test_windows_and_streams_equal_the_whole_sink(W, ahead):
    """the dependence is local: `After` / `Until` / `Window` over the node and `stream` blocks give the slice of the whole
    sink bit for bit, with frames beyond a block's end read for its last windows (`ahead > 0`)"""
    N = 4 * T + 11
    x = halves(N, 2, seed=2)
    back = W - 1 - ahead
    trees = (("array", so.MovingMax(so.Signal(x, FS), W, ahead=ahead), moving_ref(x, back, ahead)),
             ("formula", so.Signal(np.sin, FS, ω=50 * so.Hz) | so.Until(N * so.frames) | so.MovingMin(W, ahead=ahead), None),
             ("map", so.MovingMax(so.Amplify(so.Signal(x, FS), 0.25), W, ahead=ahead), moving_ref(np.asfortranarray(x * 0.25), back, ahead)))
    for name, tree, want in trees:
        whole = sunk(tree)
        if want is not None:
            bit_equal(whole, want, name)
        for a, n in ((1, 5), (T + 3, T + 1), (T - 1, 2 * T), (3 * T + 5, T)):
            got = so.sink(tree | so.After(a * so.frames) | so.Until(n * so.frames), so.Array)
            bit_equal(got.reshape(n, -1), whole[a:a + n], f"{name}: After({a}) | Until({n})")
            got = so.sink(tree | so.Window(from_=a * so.frames, to=(a + n) * so.frames), so.Array)
            bit_equal(got.reshape(n, -1), whole[a:a + n], f"{name}: Window({a}, {n})")
        got = so.sink(tree | so.Until((T + 3) * so.frames), so.Array)
        bit_equal(got.reshape(T + 3, -1), whole[:T + 3], f"{name}: Until")
        got = so.sink(tree | so.After((2 * T + 1) * so.frames), so.Array)
        bit_equal(got.reshape(N - 2 * T - 1, -1), whole[2 * T + 1:], f"{name}: After")
        for bs in (1000, T):
            blocks = np.vstack([np.asarray(b).reshape(len(b), -1) for b in so.stream(tree, bs, so.Array)])
            bit_equal(blocks, whole, f"{name}: blocks of {bs}")


@pytest.mark.parametrize("W,ahead", [(100, 33), (H + 2, 900)])
def test_a_stream_over_an_infinite_signal(W, ahead):
    tree = so.Signal(np.sin, FS, ω=37 * so.Hz) | so.MovingMax(W, ahead=ahead)
    assert S.isknowninf(so.nframes(tree))
    bs = T + 5
    whole = sunk(tree | so.Until(3 * bs * so.frames))  # no upper clip: the windows of the last frames read beyond them
    blocks = [np.asarray(b).reshape(len(b), -1) for b in itertools.islice(so.stream(tree, bs, so.Array), 3)]
    assert [len(b) for b in blocks] == [bs] * 3
    bit_equal(np.vstack(blocks), whole, "three blocks of an infinite signal")
    s = sunk(so.Signal(np.sin, FS, ω=37 * so.Hz) | so.Until((3 * bs + ahead) * so.frames))
    bit_equal(whole, moving_ref(s, W - 1 - ahead, ahead)[:3 * bs], "against the reference over the frames it reads")


def test_a_late_window_computes_its_own_range_only():
    """step information: the stage of a late window reads the window plus its halo and writes the window, not frames from 0"""
    import torch

    N = 40 * T
    x = dev(halves(N, 2))
    for W, ahead in ((100, 33), (H + 2, 900)):
        back = W - 1 - ahead
        a, n = 30 * T + 7, T + 3
        tree = so.MovingMax(so.Signal(x, FS), W, ahead=ahead) | so.After(a * so.frames) | so.Until(n * so.frames)
        out = torch.empty((2, n), dtype=torch.float64, device="cuda").t()
        p = Plan(tree, (n, 2), np.float64, (1, n), True)
        p.set_profiling(True)
        p.execute(out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        steps = [s for s in p.steps() if s["name"] == "k_moving"]
        p.close()
        assert len(steps) == 1 and steps[0]["algorithmic_bytes"] == ((n + back + ahead) + n) * 2 * 8, steps
        bit_equal(out.cpu().numpy(), np.ascontiguousarray(moving_ref(x.cpu().numpy(), back, ahead)[a:a + n]), f"the late window W={W}")


# ---- 6. consumers -----------------------------------------------------------------------------------------------------------
def test_consumers_behind_the_node():
    """each consumer over the node equals the consumer over the sunk node.  Pointwise maps and `SampleAt` are the same
    operations on the same values whichever way they read them: bit for bit.  `Filt`, `ToFramerate` and `Normpower`
    choose their chunking, tables and reduction order by the plan they are in: the Float64 contract, 1e-8 norm-wise."""
    N = 3 * T + 77
    x = halves(N, 2, seed=4)
    xs = so.Signal(x, FS)
    for W, ahead in ((101, 50), (H + 2, 1000)):
        mid = moving_ref(x, W - 1 - ahead, ahead)
        tree = so.MovingMax(xs, W, ahead=ahead)
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
            close(got, want, f"MovingMax({W}) | {name}")


def test_a_look_ahead_limiter_stays_on_the_device():
    """|x| -> peak over the next 5 ms -> smoothed -> gain curve, applied to x delayed by the same 5 ms: the chain with the node
    against the same chain fed the reference's peak envelope as an array.  (`ahead` is at most w - 1, so a look-ahead of 5 ms
    = 50 frames takes a window of 51.)"""
    N = 3 * T + 77
    rng = np.random.default_rng(11)
    x = np.asfortranarray(rng.standard_normal((N, 2)) * (1.0 + 3.0 * (rng.random((N, 1)) < 0.002)))
    xs = so.Signal(x, FS)
    rect = so.OperateOn(so.elementwise(lambda v: np.abs(v)), xs)
    curve = so.elementwise(lambda e: np.minimum(1.0, 1.5 / np.maximum(e, 1e-9)))

    def chain(peak):
        gain = so.OperateOn(curve, peak | so.Filt(so.Lowpass, 500 * so.Hz))
        return so.Amplify(so.Delay(xs, 5 * so.ms), gain)

    peak = so.MovingMax(rect, 51, ahead=5 * so.ms)
    assert (peak.back, peak.ahead) == (0, 50)
    env = moving_ref(np.asfortranarray(np.abs(x)), 0, 50)
    bit_equal(sunk(peak), env, "the peak envelope")
    got, want = sunk(chain(peak)), sunk(chain(so.Signal(env, FS)))
    assert np.ptp(want) > 1.0
    close(got, want, "the limiter")


# ---- 7. plan reuse and step information ----------------------------------------------------------------------------------
@pytest.mark.parametrize("W,ahead", [(100, 33), (H + 2, 900)])
def test_a_plan_is_reused_after_set_array(W, ahead):
    import torch

    N = 3 * T + 3
    back = W - 1 - ahead
    xs = [halves(N, 2, seed=k) for k in range(3)]
    res = np.zeros((N, 2), order="F")
    p = Plan(so.MovingMin(so.Signal(xs[0], FS), W, ahead=ahead), res.shape, res.dtype, (1, res.shape[0]), False)
    scratch = p.stats()["scratch_bytes"]
    for k in (0, 1, 1, 2, 0):
        p.set_array(0, xs[k])
        p.execute(res.ctypes.data)
        bit_equal(res, moving_ref(xs[k], back, ahead, True), f"host leaf {k}")
        assert p.stats()["scratch_bytes"] == scratch
    p.close()
    dx = [dev(a) for a in xs]
    out = torch.empty((2, N), dtype=torch.float64, device="cuda").t()
    p = Plan(so.MovingMin(so.Signal(dx[0], FS), W, ahead=ahead), (N, 2), np.float64, (1, N), True)
    for k in (0, 0, 1, 1, 2, 2, 0):
        p.set_array(0, dx[k])
        p.execute(out.data_ptr())
        p.check()
        bit_equal(out.cpu().numpy(), np.ascontiguousarray(moving_ref(xs[k], back, ahead, True)), f"device leaf {k}")
        s = p.stats()
        assert s["h2d_bytes"] == 0 and s["d2h_bytes"] == 0 and s["scratch_bytes"] <= 4096  # x is read where it lies; the table
    p.close()


def test_step_info_names_the_kernel_and_counts_a_read_and_a_write():
    import torch

    N = 5 * T + 5
    for W, launches in ((100, 1), (H + 2, 2), (2 * T + 5, 3), (4 * T + 5, 4)):  # (W - 1) // T = 1, 2, 4 whole blocks at most: table levels 0, 0-1, 0-2
        for dtype, tdtype, esz in ((np.float64, torch.float64, 8), (np.float32, torch.float32, 4)):
            x = dev(halves(N, 3, dtype))
            out = torch.empty((3, N), dtype=tdtype, device="cuda").t()
            p = Plan(so.MovingMax(so.Signal(x, FS), W), (N, 3), dtype, (1, N), True)
            p.set_profiling(True)
            p.execute(out.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            steps = p.steps()
            p.close()
            assert [s["name"] for s in steps] == ["k_moving"], steps
            assert steps[0]["algorithmic_bytes"] == 2 * N * 3 * esz and steps[0]["launches"] == launches, (W, steps)
            bit_equal(out.cpu().numpy(), np.ascontiguousarray(moving_ref(x.cpu().numpy(), W - 1, 0)), f"W={W} {np.dtype(dtype).name}")


# ---- 8. malformed node tables -------------------------------------------------------------------------------------------------
def _create(lw, nframes, nch):
    out = K.so_out_desc_t(dtype=K.SO_F64, nch=nch, nframes=nframes, frame_stride=1, chan_stride=nframes, is_device=0)
    plan = C.c_void_p()
    st = K.lib().so_plan_create(lw.nodes, lw.n, lw.root, C.byref(out), 0, C.byref(plan))
    if plan.value:
        K.lib().so_plan_destroy(plan)
    return st, K.last_error() if st else ""


def test_malformed_nodes_are_refused():
    x = so.Signal(halves(64, 3), FS)
    lw = LW.lower(so.MovingMax(x, 9, ahead=3))
    assert _create(lw, 64, 3)[0] == 0  # the well-formed node
    n = lw.root
    assert lw.nodes[n].kind == K.NODE_MOVING == 15
    invalid, unsupported = -1, -3  # include/sigops.h so_status_t: SO_ERR_INVALID, SO_ERR_UNSUPPORTED
    two = (C.c_int32 * 2)(0, 0)
    kids = lw.nodes[n].children
    lw.nodes[n].children = C.cast(two, C.POINTER(C.c_int32))
    lw.nodes[n].n_children = 2
    st, err = _create(lw, 64, 3)
    assert st == invalid and f"node {n}" in err and "Moving" in err and "one child" in err, err
    lw.nodes[n].n_children = 0
    st, err = _create(lw, 64, 3)
    assert st == invalid and f"node {n}" in err and "Moving" in err and "one child" in err, err
    lw.nodes[n].children = kids
    lw.nodes[n].n_children = 1
    assert _create(lw, 64, 3)[0] == 0
    for field, bad, good, words in (("l0", -1, 5, "back >= 0"), ("l1", -1, 3, "ahead >= 0"), ("i0", 2, 0, "maximum (0) or a minimum (1)")):
        setattr(lw.nodes[n], field, bad)
        st, err = _create(lw, 64, 3)
        assert st == invalid and f"node {n}" in err and "Moving" in err and words in err, (field, err)
        setattr(lw.nodes[n], field, good)
        assert _create(lw, 64, 3)[0] == 0
    # an integer child (the host refuses to build it: the node is made by hand)
    st, err = _create(LW.lower(S.MovingSignal(so.Signal(5, FS) | so.Until(64 * so.frames), 2, 1, False)), 64, 1)  # an Int64 constant
    assert st == unsupported and "Moving" in err and "Float32 or Float64" in err, err
