"""`Cumsum(x)` and `Integrate(x)` on the device (include/sigops.h SO_NODE_CUMSUM; csrc/k_cumsum.hip), through the public
interface and the C-ABI: bit for bit against the NumPy definition (tests/cumsum_ref.py cumsum_ref) -- no tolerance, the
summation tree is specified addition by addition.  The definition is held to its scalar restatement, to itself on every
prefix, to `np.cumsum` and to `math.fsum` without a GPU in tests/test_cumsum_host.py."""
import ctypes as C

import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import _capi as K
from sigops_amd import engine, sharding
from sigops_amd import lowering as LW
from sigops_amd import signals as S
from sigops_amd.engine import Plan
from oracle_bridge import relerr
from comb_ref import comb
from cumsum_ref import CH, CHANNELS, L, LENGTHS, T, cumsum_ref, huge, integrate_ref, planted, same_bits, signal, wide
from sampleat_ref import sampleat_np

pytestmark = pytest.mark.gpu
FS = 10 * so.kHz


def bit_equal(got, want, what=""):
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} samples differ, first at {np.argwhere(bad)[0]}"
    assert same_bits(got, want), f"{what}: a zero of the other sign"


def check(x, what=""):
    got = so.sink(so.Cumsum(so.Signal(x, FS)), so.Array)
    bit_equal(got, cumsum_ref(x), f"{what} N={x.shape[0]} C={x.shape[1]}")
    return got


def dev(a):
    """a planar device tensor [frames x channels]"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t()


def close(got, want, what, tol=1e-8):
    """the project's Float64 contract, norm-wise, the observed value printed"""
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    e = relerr(got, want)
    print(f"worst {what}: {e:.3e}")
    assert e <= tol, f"{what}: {e:.3e}"


def sunk(tree):
    """a sub-tree sunk on its own, planar, frames x channels"""
    mid = so.sink(tree, so.Array)
    return np.asfortranarray(mid.reshape(mid.shape[0], -1))


# ---- 1. geometry and data ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", LENGTHS)
def test_every_length_and_channel_count(N):
    """the smallest shapes that cross each level of the tree, ragged at each level; Gaussian data, magnitudes from 2^-60 to
    2^60 (the order of the additions shows in the bits), values near overflow (Inf, and Inf - Inf, where the tree says)"""
    for Cn in CHANNELS:
        check(signal(N, Cn), "Gaussian")
        check(wide(N, Cn), "2^-60 .. 2^60")
        got = check(huge(N, Cn), "near overflow")
        if N >= T:
            assert np.isinf(got).any()


@pytest.mark.parametrize("N", [L + 1, T + 1, CH + 1, 2 * CH + 1, 3 * CH + 77])
def test_planted_zeros_infinities_and_nans(N):
    for Cn in (1, 3, 8):
        for dtype in (np.float64, np.float32):
            x = planted(N, Cn, dtype)
            got = check(x, f"planted {np.dtype(dtype).name}")
            if Cn >= 3:
                assert np.signbit(got[:, Cn - 1]).all() and not got[:, Cn - 1].any()  # all -0.0 stays -0.0
    x = signal(N, 2)
    a, b = N // 3, (2 * N) // 3
    x[a, 0], x[b, 0], x[b, 1] = np.inf, -np.inf, np.nan
    got = check(x, "+Inf then -Inf; a NaN")
    assert np.isfinite(got[:a, 0]).all() and (got[a:b, 0] == np.inf).all() and np.isnan(got[b:, 0]).all()
    assert np.isfinite(got[:b, 1]).all() and np.isnan(got[b:, 1]).all()


# ---- 2. leaf kinds -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [T + L + 3, 2 * CH + T + 5])
def test_leaf_kinds(N):
    import torch

    for Cn in (1, 3):
        x = signal(N, Cn)
        want = cumsum_ref(x)
        tree = lambda leaf: so.Cumsum(so.Signal(leaf, FS))  # noqa: E731
        x32 = signal(N, Cn, np.float32)
        want32 = cumsum_ref(x32)
        got = so.sink(tree(x32), so.Array)
        assert got.dtype == np.float64
        bit_equal(got, want32, "a Float32 array")
        xi = np.ascontiguousarray(x)  # frames x channels, C order: frame stride = channels
        assert xi.strides == (8 * Cn, 8)
        bit_equal(so.sink(tree(xi), so.Array), want, "an interleaved host array")
        big = np.asfortranarray(np.random.default_rng(5).standard_normal((2 * N, 2 * Cn)))
        big[::2, ::2] = x
        bit_equal(so.sink(tree(big[::2, ::2]), so.Array), want, "a strided view")
        big32 = np.zeros((N, 2 * Cn), dtype=np.float32)  # C order, every second column
        big32[:, ::2] = x32
        bit_equal(so.sink(tree(big32[:, ::2]), so.Array), want32, "a strided Float32 view")
        got, fs = so.sink(tree(dev(x)), "torch")
        assert fs == 10_000.0 and got.is_cuda
        bit_equal(got.cpu().numpy(), np.ascontiguousarray(want), "a planar device tensor, device result")
        bit_equal(so.sink(tree(dev(x32)), so.Array), want32, "a planar Float32 device tensor")
        di = torch.from_numpy(xi).cuda()  # interleaved on the device
        bit_equal(so.sink(tree(di), so.Array), want, "an interleaved device tensor")
        out = torch.full((Cn, N + 1), 7.0, dtype=torch.float64, device="cuda")[:, 1:].t()  # rows that start 8 bytes off a 16-byte boundary
        so.sink_into(out, tree(dev(x)))
        bit_equal(out.cpu().numpy(), np.ascontiguousarray(want), "sink_into a device tensor, unaligned rows")
        bit_equal(so.sink(tree(dev(x)[1:]), so.Array), cumsum_ref(x[1:]), "a device leaf whose rows start 8 bytes off a 16-byte boundary")
        res = np.zeros((N, Cn), order="F")
        so.sink_into(res, tree(x))
        bit_equal(res, want, "sink_into a host array")


# ---- 3. a sub-tree as x ----------------------------------------------------------------------------------------------------
def test_a_sub_tree_as_x():
    N = CH + T + 37
    raw = signal(N + 1000, 2)
    pos = np.asfortranarray(np.linspace(0.0, N + 998.0, N).reshape(-1, 1) + 3.0 * np.sin(np.arange(N) / 50.0).reshape(-1, 1))
    square = so.elementwise(lambda v: v * v - 0.5)
    children = (("Signal(sin) | Until", so.Signal(np.sin, FS, ω=50 * so.Hz) | so.Until(N * so.frames)),
                ("a traced elementwise map", so.OperateOn(square, so.Signal(raw, FS))),
                ("a map", so.Amplify(so.Signal(raw, FS), 0.25)),
                ("SampleAt", so.SampleAt(so.Signal(raw, FS), so.Signal(pos, FS))),
                ("Comb", so.Comb(so.Signal(raw, FS), 257, 0.7)),
                ("Filt", so.Signal(raw, FS) | so.Filt(so.Highpass, 1 * so.kHz)),
                ("ToFramerate", so.Signal(raw, FS) | so.ToFramerate(12 * so.kHz)))
    for name, child in children:
        mid = sunk(child)  # the child, sunk separately
        assert np.isfinite(mid).all() and np.ptp(mid) > 0.1 and mid.shape[0] > CH
        bit_equal(so.sink(so.Cumsum(child), so.Array), cumsum_ref(mid), f"Cumsum({name})")
    bit_equal(so.sink(so.Comb(so.Signal(raw, FS), 257, 0.7) | so.Cumsum, so.Array), cumsum_ref(comb(raw, 257, 0.7)), "Cumsum(Comb), against comb_ref")


def test_a_double_integrator_and_integrate():
    x = signal(2 * CH + 77, 2)
    xs = so.Signal(x, FS)
    bit_equal(so.sink(xs | so.Cumsum | so.Cumsum, so.Array), cumsum_ref(cumsum_ref(x)), "Cumsum(Cumsum(x))")
    bit_equal(so.sink(xs | so.Integrate, so.Array), integrate_ref(x, 10_000.0), "Integrate")
    bit_equal(so.sink(xs | so.Integrate | so.Integrate, so.Array), integrate_ref(integrate_ref(x, 10_000.0), 10_000.0), "Integrate twice")
    x32 = signal(CH + 5, 1, np.float32)
    bit_equal(so.sink(so.Integrate(so.Signal(x32, 44.1 * so.kHz)), so.Array), integrate_ref(x32, 44_100.0), "Integrate(Float32)")


# ---- 4. windows and streams --------------------------------------------------------------------------------------------------
def test_windows_and_streams_equal_the_whole_sink():
    """the tree depends on the frame index only: `After` / `Until` over the node and blocks of a size that does not divide
    1024 give the slice of the whole sink bit for bit, for array, formula and map children"""
    N = 2 * CH + T + 11
    x = signal(N, 2)
    trees = (("array", so.Cumsum(so.Signal(x, FS)), cumsum_ref(x)),
             ("formula", so.Signal(np.sin, FS, ω=50 * so.Hz) | so.Until(N * so.frames) | so.Cumsum, None),
             ("map", so.Cumsum(so.Amplify(so.Signal(x, FS), 0.25)), cumsum_ref(np.asfortranarray(x * 0.25))))
    for name, tree, want in trees:
        whole = so.sink(tree, so.Array)
        whole = whole.reshape(whole.shape[0], -1)
        if want is not None:
            bit_equal(whole, want, name)
        for a, n in ((1, 5), (L + 3, 2 * T + 1), (T - 1, CH), (CH + 5, CH + T + 2)):
            got = so.sink(tree | so.After(a * so.frames) | so.Until(n * so.frames), so.Array)
            bit_equal(got.reshape(n, -1), whole[a:a + n], f"{name}: After({a}) | Until({n})")
        got = so.sink(tree | so.Until((CH + 3) * so.frames), so.Array)
        bit_equal(got.reshape(CH + 3, -1), whole[:CH + 3], f"{name}: Until")
        got = so.sink(tree | so.After((CH + T + 1) * so.frames), so.Array)
        bit_equal(got.reshape(N - CH - T - 1, -1), whole[CH + T + 1:], f"{name}: After")
        for bs in (7000, 16385):  # (neither divides 1024 nor is divided by it)
            blocks = np.vstack([np.asarray(b).reshape(len(b), -1) for b in so.stream(tree, bs, so.Array)])
            bit_equal(blocks, whole, f"{name}: blocks of {bs}")


def test_windows_and_streams_over_a_filtered_child():
    """the node adds nothing to what its child does: a `Filt` chunks its input by the frames asked of it, so a window's
    filter output differs from the whole sink's in the last bits (K2's own contract, the Float64 one), and the sum above
    it carries exactly that (tests/test_gpu_comb.py says the same of `Comb`)"""
    N = CH + T + 11
    x = signal(N, 2)
    tree = so.Cumsum(so.Signal(x, FS) | so.Filt(so.Highpass, 1 * so.kHz))
    whole = so.sink(tree, so.Array)
    assert np.ptp(whole) > 0.1
    close(so.sink(tree | so.After((T - 1) * so.frames) | so.Until(CH * so.frames), so.Array), np.asfortranarray(whole[T - 1:T - 1 + CH]), "a window over Cumsum(Filt)")
    for bs in (7000,):
        close(np.asfortranarray(np.vstack([b for b in so.stream(tree, bs, so.Array)])), whole, f"blocks of {bs} over Cumsum(Filt)")


# ---- 5. consumers ------------------------------------------------------------------------------------------------------------
def test_consumers_behind_the_node():
    """each consumer over the node equals the consumer over the sunk node.  `Operate` (a pointwise map) is the same
    operation on the same values whichever way it reads them: bit for bit.  `Filt`, `ToFramerate` and `Normpower` choose
    their chunking, tables and reduction order by the plan they are in: the Float64 contract, 1e-8 norm-wise."""
    x = signal(2 * CH + 77, 2)
    x -= x.mean(axis=0)  # (a sum that stays near 0: a random walk)
    xs = so.Signal(x, FS)
    mid = cumsum_ref(x)
    tree = so.Cumsum(xs)
    bit_equal(so.sink(tree, so.Array), mid)
    got = so.sink(so.Mix(xs, tree), so.Array)
    bit_equal(got, so.sink(so.Mix(xs, so.Signal(mid, FS)), so.Array), "Cumsum | Operate(+): Mix(x, .)")
    bit_equal(got, np.asfortranarray(x + mid), "Mix(x, .) against NumPy")
    half = so.elementwise(lambda v: 0.5 * v + 1.0)
    bit_equal(so.sink(so.OperateOn(half, tree), so.Array), so.sink(so.OperateOn(half, so.Signal(mid, FS)), so.Array), "Cumsum | Operate(elementwise)")
    for name, tail in (("Filt(Highpass)", lambda t: t | so.Filt(so.Highpass, 1 * so.kHz)),
                       ("ToFramerate", lambda t: t | so.ToFramerate(12 * so.kHz)),
                       ("Normpower", lambda t: t | so.Normpower)):
        got = so.sink(tail(tree), so.Array)
        want = so.sink(tail(so.Signal(mid, FS)), so.Array)
        assert np.ptp(want) > 0.1
        close(got, want, f"Cumsum | {name}")


# ---- 6. the reason for the feature -----------------------------------------------------------------------------------------
def test_a_wavetable_oscillator_through_a_frequency_trajectory():
    """`SampleAt(table, Cumsum(f), wrap=True)`: a 2048-entry sine table read at the running sum of a frequency trajectory
    (in table entries per frame) of 40 000 frames"""
    n, size = 40_000, 2048
    table = np.sin(2 * np.pi * np.arange(size) / size).reshape(-1, 1)
    hz = 220.0 * np.exp2(np.linspace(0.0, 2.0, n)) * (1.0 + 0.01 * np.sin(2 * np.pi * 5.0 * np.arange(n) / 10_000.0))  # a sweep with vibrato
    f = np.asfortranarray((hz * size / 10_000.0).reshape(-1, 1))
    tree = so.SampleAt(so.Signal(table, FS), so.Cumsum(so.Signal(f, FS)), wrap=True)
    got = so.sink(tree, so.Array)
    phase = cumsum_ref(f)
    assert phase[-1, 0] > 1000 * size  # many wraps
    want = sampleat_np(table, phase, wrap=True)
    bit_equal(got.reshape(n, 1), want, "the oscillator")
    assert np.ptp(got) > 1.9


def test_brown_noise_from_device_noise():
    n = 20_000
    white = so.Signal(so.randn, FS, rng=so.DeviceRNG(1, 0)) | so.Until(n * so.frames)
    w = sunk(white)
    assert w.shape == (n, 1) and abs(w.std() - 1.0) < 0.05
    got = so.sink(white | so.Cumsum, so.Array)
    bit_equal(got.reshape(n, 1), cumsum_ref(w), "Cumsum over device noise")


# ---- 7. plan reuse and step information ----------------------------------------------------------------------------------
def test_a_plan_is_reused_after_set_array():
    import torch

    N = 2 * CH + T + 3
    xs = [signal(N, 2, seed=k) for k in range(3)]
    res = np.zeros((N, 2), order="F")
    p = Plan(so.Cumsum(so.Signal(xs[0], FS)), res.shape, res.dtype, (1, res.shape[0]), False)
    scratch = p.stats()["scratch_bytes"]
    for k in (0, 1, 1, 2, 0):
        p.set_array(0, xs[k])
        p.execute(res.ctypes.data)
        bit_equal(res, cumsum_ref(xs[k]), f"host leaf {k}")
        assert p.stats()["scratch_bytes"] == scratch
    p.close()
    dx = [dev(a) for a in xs]
    out = torch.empty((2, N), dtype=torch.float64, device="cuda").t()
    p = Plan(so.Cumsum(so.Signal(dx[0], FS)), (N, 2), np.float64, (1, N), True)
    for k in (0, 0, 0, 1, 1, 2, 2, 2):
        p.set_array(0, dx[k])
        p.execute(out.data_ptr())
        p.check()
        bit_equal(out.cpu().numpy(), np.ascontiguousarray(cumsum_ref(xs[k])), f"device leaf {k}")
        s = p.stats()
        assert s["h2d_bytes"] == 0 and s["d2h_bytes"] == 0 and s["scratch_bytes"] <= 4096  # x is read where it lies; the chunk totals
    p.close()


def test_step_info_names_the_kernel_and_counts_two_reads_and_a_write():
    import torch

    for N, launches in ((2 * CH + 5, 3), (CH, 1)):
        for dtype, esz in ((np.float64, 8), (np.float32, 4)):
            x = dev(signal(N, 3, dtype))
            out = torch.empty((3, N), dtype=torch.float64, device="cuda").t()
            p = Plan(so.Cumsum(so.Signal(x, FS)), (N, 3), np.float64, (1, N), True)
            p.set_profiling(True)
            p.execute(out.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            steps = p.steps()
            p.close()
            assert [s["name"] for s in steps] == ["k_cumsum"], steps
            assert steps[0]["algorithmic_bytes"] == N * 3 * (2 * esz + 8) and steps[0]["launches"] == launches, steps


# ---- 8. malformed node tables and refusals -------------------------------------------------------------------------------
def _create(lw, nframes, nch):
    out = K.so_out_desc_t(dtype=K.SO_F64, nch=nch, nframes=nframes, frame_stride=1, chan_stride=nframes, is_device=0)
    plan = C.c_void_p()
    st = K.lib().so_plan_create(lw.nodes, lw.n, lw.root, C.byref(out), 0, C.byref(plan))
    if plan.value:
        K.lib().so_plan_destroy(plan)
    return st, K.last_error() if st else ""


def test_malformed_nodes_are_refused():
    x = so.Signal(signal(64, 3), FS)
    lw = LW.lower(so.Cumsum(x))
    assert _create(lw, 64, 3)[0] == 0  # the well-formed node
    n = lw.root
    assert lw.nodes[n].kind == K.NODE_CUMSUM == 14
    invalid, length, unsupported = -1, -2, -3  # include/sigops.h so_status_t: SO_ERR_INVALID, SO_ERR_LENGTH, SO_ERR_UNSUPPORTED
    two = (C.c_int32 * 2)(0, 0)
    kids = lw.nodes[n].children
    lw.nodes[n].children = C.cast(two, C.POINTER(C.c_int32))
    lw.nodes[n].n_children = 2
    st, err = _create(lw, 64, 3)
    assert st == invalid and f"node {n}" in err and "Cumsum" in err and "one child" in err, err
    lw.nodes[n].n_children = 0
    st, err = _create(lw, 64, 3)
    assert st == invalid and "Cumsum" in err and "one child" in err, err
    lw.nodes[n].children = kids
    lw.nodes[n].n_children = 1
    assert _create(lw, 64, 3)[0] == 0
    # an infinite child and an integer child (the host refuses to build them: the nodes are made by hand)
    st, err = _create(LW.lower(S.CumsumSignal(so.Signal(np.sin, FS, ω=5 * so.Hz))), 64, 1)
    assert st == length and "Cumsum" in err and "finite length" in err, err
    st, err = _create(LW.lower(S.CumsumSignal(so.Signal(5, FS) | so.Until(64 * so.frames))), 64, 1)  # an Int64 constant
    assert st == unsupported and "Cumsum" in err and "Float32 or Float64" in err, err


def test_blockstream_and_shards_refuse_the_node_by_name():
    x = so.Signal(signal(4096, 2), FS)
    with pytest.raises(so.ErrorException, match="BlockStream: Cumsum"):
        engine._streamable(so.Cumsum(x) | so.Filt(so.Lowpass, 1 * so.kHz))
    with pytest.raises(so.ErrorException, match="BlockStream: Cumsum"):
        engine._streamable(so.Mix(so.Integrate(x), 1.0))
    for make in (lambda: sharding.shard_time(so.Cumsum(x), 0, 2), lambda: sharding.shard_channels(so.Integrate(x), 1, 2),
                 lambda: sharding.shard_append(so.Append(so.Cumsum(x), x), 0, 2)):
        with pytest.raises(so.ErrorException, match="Cumsum / Integrate over several GPUs is not built"):
            make()
