"""`Recur(a, b)`, `OnePole`, `Smooth` and `PeakDecay` on the device (include/sigops.h SO_NODE_RECUR; csrc/k_recur.hip), through the
public interface and the C-ABI: bit for bit against the NumPy definition (tests/recur_ref.py recur_ref) -- no tolerance,
the tree of the scan is specified operation by operation.  The definition is held to its scalar restatement, to itself
on every prefix, to `cumsum_ref` and to the sequential loop without a GPU in tests/test_recur_host.py."""
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
from moving_ref import moving_ref
from recur_ref import CH, CHANNELS, COEFS, L, LENGTHS, T, coef, planted, recur_ref, same_bits, signal, wide

pytestmark = pytest.mark.gpu
FS = 10 * so.kHz
OPS = [0, 1]


def bit_equal(got, want, what=""):
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} samples differ, first at {np.argwhere(bad)[0]}"
    assert same_bits(got, want), f"{what}: a zero of the other sign"


def node(op, a, b):
    """the node over signals (or a number a): Recur for op 0, PeakDecay(r=) for op 1"""
    return so.Recur(a, b) if op == 0 else so.PeakDecay(b, r=a)


def sig(x):
    return x if isinstance(x, (int, float)) else so.Signal(x, FS)


def check(op, a, b, what=""):
    got = so.sink(node(op, sig(a), so.Signal(b, FS)), so.Array)
    bit_equal(got.reshape(b.shape), recur_ref(a, b, op), f"{what} op={op} N={b.shape[0]} C={b.shape[1]}")
    return got.reshape(b.shape)


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
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("N", LENGTHS)
def test_every_length_channel_count_and_coefficient(N, op):
    """the smallest shapes that cross each level of the tree, ragged at each level; a constant a, a row for every channel
    and a row per channel, from U[0,1], U[-1,1], 0.999 and U[0.99,1]; Gaussian b and magnitudes from 2^-60 to 2^60 (the
    order of the operations shows in the bits); Float32 and Float64 b"""
    for Cn in CHANNELS:
        g, w = signal(N, Cn), wide(N, Cn)
        if op == 1:
            g, w = np.abs(g), np.abs(w)
        check(op, 0.999, g, "constant a")
        check(op, -0.75 if op == 0 else 0.5, w, "constant a, 2^-60 .. 2^60")
        for k, kind in enumerate(COEFS):
            b = (g, w)[k % 2]
            check(op, coef(kind, N, 1), b, f"one row of {kind}")
            if Cn > 1:
                check(op, coef(kind, N, Cn), b, f"a row per channel of {kind}")
        b32 = signal(N, Cn, np.float32)
        check(op, coef("u01", N, 1), b32, "Float32 b")
        check(op, 0.5, b32, "Float32 b, constant a")


@pytest.mark.parametrize("op", OPS)
def test_a_constant_runs_the_multiplications_of_a_row(op):
    for N in (L + 1, 2 * CH + T + 5):
        b = wide(N, 3)
        for a in (0.999, 1.0, 0.0, -0.5 if op == 0 else 0.5):  # (PeakDecay takes a constant r in [0, 1])
            got = check(op, a, b, f"constant {a}")
            bit_equal(check(op, np.full((N, 1), a), b, f"a row of {a}"), got, "row against constant")


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("N", [L + 1, T + 1, CH + 1, 2 * CH + 1, 3 * CH + 77])
def test_planted_zeros_infinities_and_nans(N, op):
    """+-0, +-Inf and NaN at run, tile and chunk boundaries, in b and in a"""
    for Cn in (1, 3, 8):
        a = coef("u099", N, Cn)
        for dtype in (np.float64, np.float32):
            b = planted(signal(N, Cn, dtype))
            got = check(op, a, b, f"planted b {np.dtype(dtype).name}")
            if Cn >= 3:
                assert np.signbit(got[:, Cn - 1]).all() and not got[:, Cn - 1].any()  # all -0.0 stays -0.0 under a > 0
        check(op, planted(a, zeros=True), np.abs(signal(N, Cn)) + 0.1, "planted a")
        check(op, planted(coef("u11", N, 1), kinds=(np.nan,)), signal(N, Cn), "planted a, one row")
        check(op, planted(a, kinds=(np.inf, -np.inf), zeros=False), planted(signal(N, Cn), kinds=()), "Inf in a over zeros in b")
    b = np.abs(signal(N, 2)) + 0.1
    i, j = N // 3, (2 * N) // 3
    b[i, 0], b[j, 0], b[j, 1] = np.inf, -np.inf, np.nan
    got = check(op, 0.9999, b, "+Inf then -Inf; a NaN")
    assert np.isfinite(got[:i, 0]).all() and (got[i:j, 0] == np.inf).all()
    assert np.isnan(got[j:, 0]).all() if op == 0 else (got[j:, 0] == np.inf).all()
    assert np.isfinite(got[:j, 1]).all() and np.isnan(got[j:, 1]).all()


def test_an_infinity_meets_an_underflowed_product_as_the_definition_says():
    N = CH + 2 * T
    b = np.ones((N, 1), order="F")
    b[3] = np.inf
    for op in OPS:
        got = check(op, 0.5, b, "0.5^1075 = 0 times Inf")
        assert (got[3:CH + 1074] == np.inf).all() and np.isnan(got[CH + 1074:]).all()


@pytest.mark.parametrize("N", [1, L + 1, T + 5, CH + T + 3, 3 * CH + 77])
def test_a_coefficient_of_one_is_cumsum_on_the_same_device(N):
    for x in (wide(N, 3), planted(signal(N, 3)), signal(N, 2, np.float32)):
        want = so.sink(so.Cumsum(so.Signal(x, FS)), so.Array)
        bit_equal(so.sink(so.Recur(1.0, so.Signal(x, FS)), so.Array), want, "Recur(1.0, x) against Cumsum(x)")
        bit_equal(so.sink(so.Recur(so.Signal(np.ones((N, 1)), FS), so.Signal(x, FS)), so.Array), want, "Recur(ones, x) against Cumsum(x)")


# ---- 2. leaf kinds -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("N", [T + L + 3, 2 * CH + T + 5])
def test_leaf_kinds_for_both_inputs(N, op):
    import torch

    for Cn in (1, 3):
        b, b32 = signal(N, Cn), signal(N, Cn, np.float32)
        a1, an = coef("u099", N, 1), coef("u01", N, Cn)
        a32 = an.astype(np.float32)
        want, want32, want1 = recur_ref(an, b, op), recur_ref(an, b32, op), recur_ref(a1, b, op)
        tree = lambda la, lb: node(op, so.Signal(la, FS), so.Signal(lb, FS))  # noqa: E731
        got = so.sink(tree(an, b32), so.Array)
        assert got.dtype == np.float64
        bit_equal(got, want32, "a Float32 b")
        bit_equal(so.sink(tree(a32, b), so.Array), recur_ref(a32, b, op), "a Float32 a")
        bi, ai = np.ascontiguousarray(b), np.ascontiguousarray(an)  # frames x channels, C order: frame stride = channels
        assert bi.strides == (8 * Cn, 8)
        bit_equal(so.sink(tree(an, bi), so.Array), want, "an interleaved b")
        bit_equal(so.sink(tree(ai, b), so.Array), want, "an interleaved a")
        bit_equal(so.sink(tree(ai, bi), so.Array), want, "both interleaved")
        big = np.asfortranarray(np.random.default_rng(5).standard_normal((2 * N, 2 * Cn)))
        big[::2, ::2] = b
        biga = np.asfortranarray(np.zeros((2 * N, 2 * Cn)))
        biga[::2, ::2] = an
        bit_equal(so.sink(tree(an, big[::2, ::2]), so.Array), want, "a strided b")
        bit_equal(so.sink(tree(biga[::2, ::2], b), so.Array), want, "a strided a")
        big32 = np.zeros((N, 2 * Cn), dtype=np.float32)  # C order, every second column
        big32[:, ::2] = b32
        bit_equal(so.sink(tree(an, big32[:, ::2]), so.Array), want32, "a strided Float32 b")
        got, fs = so.sink(tree(dev(an), dev(b)), "torch")
        assert fs == 10_000.0 and got.is_cuda
        bit_equal(got.cpu().numpy(), np.ascontiguousarray(want), "planar device tensors, device result")
        bit_equal(so.sink(tree(dev(a1), dev(b32)), so.Array), recur_ref(a1, b32, op), "a device row for every channel, Float32 device b")
        bit_equal(so.sink(tree(dev(a32), dev(b)), so.Array), recur_ref(a32, b, op), "a Float32 device a")
        bit_equal(so.sink(tree(torch.from_numpy(ai).cuda(), torch.from_numpy(bi).cuda()), so.Array), want, "interleaved device tensors")
        out = torch.full((Cn, N + 1), 7.0, dtype=torch.float64, device="cuda")[:, 1:].t()  # rows that start 8 bytes off a 16-byte boundary
        so.sink_into(out, tree(dev(a1), dev(b)))
        bit_equal(out.cpu().numpy(), np.ascontiguousarray(want1), "sink_into a device tensor, unaligned rows")
        bit_equal(so.sink(tree(dev(an), dev(b)[1:]), so.Array), recur_ref(an[:N - 1], b[1:], op), "a device b whose rows start 8 bytes off a 16-byte boundary")
        bit_equal(so.sink(tree(dev(an)[1:], dev(b)[:N - 1]), so.Array), recur_ref(an[1:], b[:N - 1], op), "a device a whose rows start 8 bytes off a 16-byte boundary")
        res = np.zeros((N, Cn), order="F")
        so.sink_into(res, tree(a1, b))
        bit_equal(res, want1, "sink_into a host array")
        bit_equal(so.sink(tree(coef("u01", N + 1000, Cn), b), so.Array), recur_ref(coef("u01", N + 1000, Cn), b, op), "an a longer than b")


# ---- 3. sub-trees as inputs ------------------------------------------------------------------------------------------------
def test_sub_trees_as_inputs():
    N = CH + T + 37
    raw = signal(N + 1000, 2)
    rawa = coef("u01", N + 1000, 2)
    half = so.elementwise(lambda v: 0.5 * v + 0.25)
    children = (("Signal(sin) | Until", so.Signal(np.sin, FS, ω=50 * so.Hz) | so.Until(N * so.frames)),
                ("a traced elementwise map", so.OperateOn(half, so.Signal(rawa, FS))),
                ("a map", so.Amplify(so.Signal(raw, FS), 0.25)),
                ("Filt", so.Signal(raw, FS) | so.Filt(so.Highpass, 1 * so.kHz)),
                ("ToFramerate", so.Signal(raw, FS) | so.ToFramerate(12 * so.kHz)),
                ("Cumsum", so.Cumsum(so.Amplify(so.Signal(raw, FS), 1e-3))),
                ("MovingMax", so.MovingMax(so.Signal(rawa, FS), 33)),
                ("Recur", so.Recur(0.9, so.Signal(raw, FS))))
    for name, child in children:
        mid = sunk(child)  # the child, sunk separately; every form below asks it for the same frames, all of them
        n, ch = mid.shape
        assert np.isfinite(mid).all() and np.ptp(mid) > 0 and n > CH
        other_b, other_a = signal(n, 2), coef("u099", n, ch)
        for op in OPS:
            got = so.sink(node(op, 0.99, child), so.Array)
            bit_equal(got.reshape(n, ch), recur_ref(0.99, mid, op), f"b = {name}, constant a, op {op}")
            got = so.sink(node(op, so.Signal(other_a, child.fs * so.Hz), child), so.Array)
            bit_equal(got.reshape(n, ch), recur_ref(other_a, mid, op), f"b = {name}, op {op}")
            got = so.sink(node(op, child, so.Signal(other_b, child.fs * so.Hz)), so.Array)
            bit_equal(got, recur_ref(mid, other_b, op), f"a = {name}, op {op}")
    other_b = signal(N, 2)
    a_inf = so.OperateOn(so.elementwise(lambda v: 0.9 + 0.09 * v), so.Signal(np.sin, FS, ω=3 * so.Hz))  # an infinite formula as a
    mid = sunk(a_inf | so.Until(N * so.frames))
    bit_equal(so.sink(so.Recur(a_inf, so.Signal(other_b, FS)), so.Array), recur_ref(mid, other_b), "an infinite formula as a")
    x = signal(2 * CH + 77, 2)
    bit_equal(so.sink(so.Signal(x, FS) | so.Recur(0.9) | so.Recur(0.8), so.Array), recur_ref(0.8, recur_ref(0.9, x)), "Recur(Recur(x))")
    shared = so.Signal(x, FS) | so.Recur(0.9)  # one node read as a and as b of another
    mid = recur_ref(0.9, x)
    bit_equal(so.sink(so.Recur(so.OperateOn(so.elementwise(lambda v: 0.01 * v), shared), shared), so.Array),
              recur_ref(np.asfortranarray(0.01 * mid), mid), "one Recur as both inputs of another")


# ---- 4. windows and streams --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
def test_windows_and_streams_equal_the_whole_sink(op):
    """the tree depends on the frame index only: `After` / `Until` over the node and blocks of a size that does not divide
    1024 give the slice of the whole sink bit for bit, for array, formula and map inputs"""
    N = 2 * CH + T + 11
    b, a = signal(N, 2), coef("u099", N, 1)
    tone = so.Signal(np.sin, FS, ω=50 * so.Hz) | so.Until(N * so.frames)
    trees = (("arrays", node(op, so.Signal(a, FS), so.Signal(b, FS)), recur_ref(a, b, op)),
             ("constant a", node(op, 0.999, so.Signal(b, FS)), recur_ref(0.999, b, op)),
             ("formula b", node(op, so.Signal(a, FS), tone), None),
             ("map a", node(op, so.Amplify(so.Signal(a, FS), 0.5), so.Signal(b, FS)), recur_ref(np.asfortranarray(a * 0.5), b, op)))
    for name, tree, want in trees:
        whole = so.sink(tree, so.Array)
        whole = whole.reshape(whole.shape[0], -1)
        if want is not None:
            bit_equal(whole, want, name)
        for s, n in ((1, 5), (L + 3, 2 * T + 1), (T - 1, CH), (CH + 5, CH + T + 2)):
            got = so.sink(tree | so.After(s * so.frames) | so.Until(n * so.frames), so.Array)
            bit_equal(got.reshape(n, -1), whole[s:s + n], f"{name}: After({s}) | Until({n})")
        got = so.sink(tree | so.Until((CH + 3) * so.frames), so.Array)
        bit_equal(got.reshape(CH + 3, -1), whole[:CH + 3], f"{name}: Until")
        got = so.sink(tree | so.After((CH + T + 1) * so.frames), so.Array)
        bit_equal(got.reshape(N - CH - T - 1, -1), whole[CH + T + 1:], f"{name}: After")
        for bs in (7000, 16385):  # (neither divides 1024 nor is divided by it)
            blocks = np.vstack([np.asarray(blk).reshape(len(blk), -1) for blk in so.stream(tree, bs, so.Array)])
            bit_equal(blocks, whole, f"{name}: blocks of {bs}")


# ---- 5. consumers ------------------------------------------------------------------------------------------------------------
def test_consumers_behind_the_node():
    """each consumer over the node equals the consumer over the sunk node.  `Operate` (a pointwise map) and `SampleAt` are
    the same operations on the same values whichever way they read them: bit for bit.  `Filt`, `ToFramerate` and
    `Normpower` choose their chunking, tables and reduction order by the plan they are in: 1e-8 norm-wise."""
    N = 2 * CH + 77
    x = signal(N, 2)
    xs = so.Signal(x, FS)
    mid = recur_ref(0.99, x)
    tree = so.Recur(0.99, xs)
    bit_equal(so.sink(tree, so.Array), mid)
    got = so.sink(so.Mix(xs, tree), so.Array)
    bit_equal(got, so.sink(so.Mix(xs, so.Signal(mid, FS)), so.Array), "Recur | Operate(+): Mix(x, .)")
    bit_equal(got, np.asfortranarray(x + mid), "Mix(x, .) against NumPy")
    half = so.elementwise(lambda v: 0.5 * v + 1.0)
    bit_equal(so.sink(so.OperateOn(half, tree), so.Array), so.sink(so.OperateOn(half, so.Signal(mid, FS)), so.Array), "Recur | Operate(elementwise)")
    pos = so.Signal(np.asfortranarray(np.linspace(0.0, N - 2.0, 5000).reshape(-1, 1)), FS)
    bit_equal(so.sink(so.SampleAt(tree, pos), so.Array), so.sink(so.SampleAt(so.Signal(mid, FS), pos), so.Array), "SampleAt over Recur")
    env = so.PeakDecay(so.Signal(np.abs(x), FS), r=0.999)  # an envelope as the positions' source: SampleAt(x, n - 3 env)
    envm = recur_ref(0.999, np.abs(x), 1)
    rel = lambda e: so.OperateOn(so.elementwise(lambda v: -3.0 * v), e)  # noqa: E731
    bit_equal(so.sink(so.SampleAt(xs, rel(env), relative=True), so.Array), so.sink(so.SampleAt(xs, rel(so.Signal(envm, FS)), relative=True), so.Array),
              "SampleAt at positions from PeakDecay")
    for name, tail in (("Filt(Highpass)", lambda t: t | so.Filt(so.Highpass, 1 * so.kHz)),
                       ("ToFramerate", lambda t: t | so.ToFramerate(12 * so.kHz)),
                       ("Normpower", lambda t: t | so.Normpower)):
        got = so.sink(tail(tree), so.Array)
        want = so.sink(tail(so.Signal(mid, FS)), so.Array)
        assert np.ptp(want) > 0.1
        close(got, want, f"Recur | {name}")


# ---- 6. the wrappers and the reason for the feature ----------------------------------------------------------------------
def test_onepole_smooth_and_peakdecay_with_constants():
    import math

    N = CH + T + 5
    x, x32 = signal(N, 2), signal(N, 2, np.float32)
    a = math.exp(-2.0 * math.pi * 300.0 / 10_000.0)
    bit_equal(so.sink(so.OnePole(so.Signal(x, FS), 300 * so.Hz), so.Array), recur_ref(a, np.asfortranarray(x * (1.0 - a))), "OnePole")
    bit_equal(so.sink(so.Signal(x32, FS) | so.OnePole(300.0), so.Array), recur_ref(a, np.asfortranarray(x32.astype(np.float64) * (1.0 - a))), "OnePole(Float32)")
    a = math.exp(-1.0 / (0.002 * 10_000.0))
    bit_equal(so.sink(so.Smooth(so.Signal(x, FS), 2 * so.ms), so.Array), recur_ref(a, np.asfortranarray(x * (1.0 - a))), "Smooth")
    bit_equal(so.sink(so.Smooth(so.Signal(x, FS), 0), so.Array), recur_ref(0.0, x), "Smooth(0)")
    assert np.array_equal(so.sink(so.Smooth(so.Signal(x, FS), 0), so.Array), x)  # x itself (but for the sign of a zero)
    r = math.exp(-1.0 / (0.05 * 10_000.0))
    bit_equal(so.sink(so.PeakDecay(so.Signal(np.abs(x), FS), 50 * so.ms), so.Array), recur_ref(r, np.abs(x), 1), "PeakDecay")
    bit_equal(so.sink(so.Signal(x, FS) | so.PeakDecay(r=1.0), so.Array), np.asfortranarray(np.maximum.accumulate(x, axis=0)), "PeakDecay(r=1): the running maximum")


def test_onepole_and_smooth_with_a_signal_coefficient():
    """`a` and `(1 - a) x` are traced maps: the node is held to recur_ref fed with the two sub-trees sunk on their own"""
    N = CH + T + 5
    x = signal(N, 2)
    xs = so.Signal(x, FS)
    fc = so.Signal(np.asfortranarray(200.0 + 150.0 * np.sin(np.arange(N) / 300.0).reshape(-1, 1)), FS)
    tau = so.Signal(np.asfortranarray(np.abs(signal(N, 2)) * 1e-3), FS)  # a time constant per channel
    tau_inf = so.OperateOn(so.elementwise(lambda v: 1e-3 + 5e-4 * v), so.Signal(np.sin, FS, ω=2 * so.Hz))
    for name, y in (("OnePole(fc signal)", so.OnePole(xs, fc)), ("Smooth(tau per channel)", so.Smooth(xs, tau)), ("Smooth(infinite tau)", so.Smooth(xs, tau_inf))):
        assert isinstance(y, so.RecurSignal) and y.coef is not None
        a = sunk(y.coef | so.Until(N * so.frames))
        b = sunk(y.signal)
        assert (a >= 0).all() and (a < 1).all() and np.ptp(a) > 1e-3
        bit_equal(so.sink(y, so.Array), recur_ref(a, b), name)
        close(b, np.asfortranarray((1.0 - a) * x), f"{name}: b against (1 - a) x", 1e-15)
    a = sunk(so.OnePole(xs, fc).coef)
    close(a, np.exp(-2.0 * np.pi * sunk(fc) / 10_000.0), "a against exp(-2 pi fc / fs)", 1e-15)


def test_a_limiter_side_chain():
    """|x| -> MovingMax -> PeakDecay -> Smooth: the gain computer of a look-ahead limiter, every stage on the device"""
    N = 2 * CH + 333
    x = signal(N, 2)
    chain = so.OperateOn(so.elementwise(np.abs), so.Signal(x, FS)) | so.MovingMax(48, ahead=47) | so.PeakDecay(20 * so.ms) | so.Smooth(1 * so.ms)
    import math

    peak = moving_ref(np.abs(x), 0, 47)
    env = recur_ref(math.exp(-1.0 / (0.02 * 10_000.0)), peak, 1)
    a = math.exp(-1.0 / (0.001 * 10_000.0))
    want = recur_ref(a, np.asfortranarray(env * (1.0 - a)))
    got = so.sink(chain, so.Array)
    bit_equal(got, want, "the side-chain")
    assert (got[2000:] > 0).all() and got.max() < np.abs(x).max()


# ---- 7. plan reuse and step information ----------------------------------------------------------------------------------
def test_a_plan_is_reused_after_set_array_on_each_input():
    import torch

    N = 2 * CH + T + 3
    bs = [signal(N, 2, seed=k) for k in range(3)]
    as_ = [coef("u099", N, 2, seed=k) for k in range(3)]
    res = np.zeros((N, 2), order="F")
    p = Plan(so.Recur(so.Signal(as_[0], FS), so.Signal(bs[0], FS)), res.shape, res.dtype, (1, res.shape[0]), False)
    scratch = p.stats()["scratch_bytes"]
    for i, k in ((0, 0), (0, 1), (1, 1), (2, 1), (2, 0), (0, 0)):
        p.set_array(0, as_[i])
        p.set_array(1, bs[k])
        p.execute(res.ctypes.data)
        bit_equal(res, recur_ref(as_[i], bs[k]), f"host leaves a{i} b{k}")
        assert p.stats()["scratch_bytes"] == scratch
    p.close()
    da, db = [dev(v) for v in as_], [dev(v) for v in bs]
    out = torch.empty((2, N), dtype=torch.float64, device="cuda").t()
    p = Plan(so.PeakDecay(so.Signal(db[0], FS), r=so.Signal(da[0], FS)), (N, 2), np.float64, (1, N), True)
    for i, k in ((0, 0), (0, 0), (1, 0), (1, 2), (2, 2), (2, 1)):
        p.set_array(0, da[i])
        p.set_array(1, db[k])
        p.execute(out.data_ptr())
        p.check()
        bit_equal(out.cpu().numpy(), np.ascontiguousarray(recur_ref(as_[i], bs[k], 1)), f"device leaves a{i} b{k}")
        s = p.stats()
        assert s["h2d_bytes"] == 0 and s["d2h_bytes"] == 0 and s["scratch_bytes"] <= 4096  # both read where they lie; the chunk totals
    p.close()


def test_step_info_names_the_kernel_and_counts_its_bytes():
    import torch

    for N, launches in ((2 * CH + 5, 3), (CH, 1)):
        for dtype, esz in ((np.float64, 8), (np.float32, 4)):
            b = dev(signal(N, 3, dtype))
            out = torch.empty((3, N), dtype=torch.float64, device="cuda").t()
            for a, abytes in ((0.5, 0), (so.Signal(dev(coef("u01", N, 1)), FS), 16), (so.Signal(dev(coef("u01", N, 3)), FS), 48)):
                p = Plan(so.Recur(a, so.Signal(b, FS)), (N, 3), np.float64, (1, N), True)
                p.set_profiling(True)
                p.execute(out.data_ptr(), torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                steps = p.steps()
                p.close()
                assert [s["name"] for s in steps] == ["k_recur"], steps
                assert steps[0]["algorithmic_bytes"] == N * (3 * (2 * esz + 8) + abytes) and steps[0]["launches"] == launches, steps


# ---- 8. malformed node tables and refusals -------------------------------------------------------------------------------
def _create(lw, nframes, nch):
    out = K.so_out_desc_t(dtype=K.SO_F64, nch=nch, nframes=nframes, frame_stride=1, chan_stride=nframes, is_device=0)
    plan = C.c_void_p()
    st = K.lib().so_plan_create(lw.nodes, lw.n, lw.root, C.byref(out), 0, C.byref(plan))
    if plan.value:
        K.lib().so_plan_destroy(plan)
    return st, K.last_error() if st else ""


def test_malformed_nodes_are_refused():
    b = so.Signal(signal(64, 3), FS)
    invalid, length, unsupported = -1, -2, -3  # include/sigops.h so_status_t: SO_ERR_INVALID, SO_ERR_LENGTH, SO_ERR_UNSUPPORTED
    lw = LW.lower(so.Recur(0.5, b))
    assert _create(lw, 64, 3)[0] == 0  # the well-formed nodes
    assert _create(LW.lower(so.PeakDecay(b, r=so.Signal(coef("u01", 64, 1), FS))), 64, 3)[0] == 0
    n = lw.root
    assert lw.nodes[n].kind == K.NODE_RECUR == 17
    for bad in (2, -1):
        lw.nodes[n].i0 = bad
        st, err = _create(lw, 64, 3)
        assert st == invalid and f"node {n}" in err and "Recur" in err and "affine (0) or max-decay (1)" in err, err
    lw.nodes[n].i0 = 0
    for bad in (np.inf, np.nan):
        lw.nodes[n].d0 = bad
        st, err = _create(lw, 64, 3)
        assert st == invalid and "Recur" in err and "finite constant a" in err, err
    lw.nodes[n].d0 = 0.5
    three = (C.c_int32 * 3)(0, 0, 0)
    kids = lw.nodes[n].children
    lw.nodes[n].children = C.cast(three, C.POINTER(C.c_int32))
    for count in (3, 0):
        lw.nodes[n].n_children = count
        st, err = _create(lw, 64, 3)
        assert st == invalid and "Recur" in err and "one child" in err and "or two" in err, err
    lw.nodes[n].children = kids
    lw.nodes[n].n_children = 1
    assert _create(lw, 64, 3)[0] == 0
    # what the host refuses to build: the nodes are made by hand
    st, err = _create(LW.lower(S.RecurSignal(so.Signal(coef("u01", 64, 2), FS), b, 0)), 64, 3)
    assert st == invalid and "Recur" in err and "2 channels: 1 or b's 3" in err, err
    st, err = _create(LW.lower(S.RecurSignal(0.5, so.Signal(np.sin, FS, ω=5 * so.Hz), 0)), 64, 1)
    assert st == length and "Recur" in err and "finite length" in err, err
    st, err = _create(LW.lower(S.RecurSignal(so.Signal(coef("u01", 10, 1), FS), b, 1)), 64, 3)
    assert st == length and "Recur" in err and "10 frames, fewer than b's 64" in err, err
    st, err = _create(LW.lower(S.RecurSignal(0.5, so.Signal(5, FS) | so.Until(64 * so.frames), 0)), 64, 1)  # an Int64 constant
    assert st == unsupported and "Recur" in err and "Float32 or Float64 signal b" in err, err
    st, err = _create(LW.lower(S.RecurSignal(so.Signal(5, FS), b, 0)), 64, 3)
    assert st == unsupported and "Recur" in err and "Float32 or Float64 signal a" in err, err


def test_blockstream_and_shards_refuse_the_node_by_name():
    x = so.Signal(signal(4096, 2), FS)
    for tree in (so.Recur(0.5, x), so.OnePole(x, 1 * so.kHz), so.Smooth(x, 1 * so.ms), so.PeakDecay(x, 1 * so.ms)):
        with pytest.raises(so.ErrorException, match="BlockStream: Recur"):
            engine._streamable(tree | so.Filt(so.Lowpass, 1 * so.kHz))
        with pytest.raises(so.ErrorException, match="BlockStream: Recur"):
            engine._streamable(so.Mix(tree, 1.0))
    for make in (lambda: sharding.shard_time(so.Recur(0.5, x), 0, 2), lambda: sharding.shard_channels(so.Smooth(x, 1 * so.ms), 1, 2),
                 lambda: sharding.shard_append(so.Append(so.PeakDecay(x, r=0.5), x), 0, 2)):
        with pytest.raises(so.ErrorException, match="Recur / OnePole / Smooth / PeakDecay over several GPUs is not built"):
            make()
