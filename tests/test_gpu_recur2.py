"""`Recur2(a1, a2, b)`, `Resonator` and `Sweep` on the device (include/sigops.h SO_NODE_RECUR2; csrc/k_recur2.hip), through the
public interface and the C-ABI: bit for bit against the NumPy definition (tests/recur2_ref.py recur2_ref) -- no tolerance,
the tree of the scan is specified operation by operation.  The definition is held to its scalar restatement, to itself on
every prefix and to the sequential loops without a GPU in tests/test_recur2_host.py."""
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
from tree_ref import evaluate
from recur2_ref import (CH, CHANNELS, COEFS, L, LENGTHS, T, coef, delayed, inf_example, overflow_example, planted, recur2_ref, resonator_coefs,
                        same_bits, signal, sweep_coefs, sweep_input, wide)

pytestmark = pytest.mark.gpu
FS = 10 * so.kHz


def bit_equal(got, want, what=""):
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} samples differ, first at {np.argwhere(bad)[0]}"
    assert same_bits(got, want), f"{what}: a zero of the other sign"


def sig(x):
    return x if isinstance(x, (int, float)) else so.Signal(x, FS)


def check(a1, a2, b, what=""):
    got = so.sink(so.Recur2(sig(a1), sig(a2), so.Signal(b, FS)), so.Array)
    bit_equal(got.reshape(b.shape), recur2_ref(a1, a2, b), f"{what} N={b.shape[0]} C={b.shape[1]}")
    return got.reshape(b.shape)


def dev(a):
    """a planar device tensor [frames x channels]"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t()


def close(got, want, what, tol=1e-8):
    """the project's Float64 contract, norm-wise, the observed value printed"""
    got = np.asarray(got).reshape(want.shape)
    assert got.dtype == want.dtype
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
def test_every_length_channel_count_and_coefficient_form(N):
    """the smallest shapes that cross each level of the tree, ragged at each level, and the + 2 lengths at which a boundary
    falls between the two frames of the state; constants, one row for every channel and a row per channel, from stable
    resonator pairs and from U[-1, 1] x U[-0.5, 0.5]; Gaussian b and magnitudes from 2^-60 to 2^60; Float32 and Float64 b"""
    for Cn in CHANNELS:
        g, w = signal(N, Cn), wide(N, Cn)
        check(1.8, -0.9, g, "constants")
        check(-0.75, 0.3, w, "constants, 2^-60 .. 2^60")
        for k, kind in enumerate(COEFS):
            b = (g, w)[k % 2]
            a1, a2 = coef(kind, N, 1)
            check(a1, a2, b, f"one row each of {kind}")
            if Cn > 1:
                n1, n2 = coef(kind, N, Cn)
                check(n1, n2, (w, g)[k % 2], f"a row per channel each of {kind}")
                check(a1, n2, b, f"one row and a row per channel of {kind}")
        b32 = signal(N, Cn, np.float32)
        check(*coef("reson", N, 1), b32, "Float32 b")
        check(0.5, 0.25, b32, "Float32 b, constants")


def test_a_constant_runs_the_operations_of_a_row():
    for N in (L + 2, 2 * CH + T + 5):
        b = wide(N, 3)
        for c1, c2 in ((1.9, -0.95), (1.0, 0.0), (0.0, 0.0), (-0.5, 0.25)):
            got = check(c1, c2, b, f"constants {c1}, {c2}")
            bit_equal(check(np.full((N, 1), c1), np.full((N, 3), c2), b, "rows of them"), got, "rows against constants")
            bit_equal(check(c1, np.full((N, 1), c2), b, "a constant next to a row"), got, "the mixed form against constants")
            bit_equal(check(np.full((N, 3), c1), c2, b, "a row next to a constant"), got, "the mixed form against constants")


@pytest.mark.parametrize("N", [L + 2, T + 2, CH + 2, 2 * CH + 2, 3 * CH + 77])
def test_planted_zeros_infinities_and_nans(N):
    """+-0, +-Inf and NaN at run, tile and chunk boundaries and one frame after each, in b and in each coefficient"""
    for Cn in (1, 3, 8):
        a1, a2 = coef("reson", N, Cn)
        for dtype in (np.float64, np.float32):
            check(a1, a2, planted(signal(N, Cn, dtype)), f"planted b {np.dtype(dtype).name}")
        check(0.5, 0.25, planted(signal(N, Cn)), "planted b, constants")
        check(planted(a1), a2, np.abs(signal(N, Cn)) + 0.1, "planted a1")
        check(a1, planted(a2), np.abs(signal(N, Cn)) + 0.1, "planted a2")
        one1, one2 = coef("u1h", N, 1)
        check(planted(one1, kinds=(np.nan,)), one2, signal(N, Cn), "planted a1, one row")
        check(one1, planted(one2, kinds=(np.inf,)), planted(signal(N, Cn), kinds=()), "Inf in a2 over zeros in b")
    b = np.abs(signal(N, 2)) + 0.1
    i, j = N // 3, (2 * N) // 3
    b[i, 0], b[j, 1] = np.inf, np.nan
    got = check(0.5, 0.25, b, "an Inf; a NaN")
    assert np.isfinite(got[:i, 0]).all() and not np.isfinite(got[i:, 0]).any()
    assert np.isfinite(got[:j, 1]).all() and np.isnan(got[j:, 1]).all()


def test_the_two_pinned_non_finite_examples():
    a1, a2, b = inf_example()
    got = check(a1, a2, np.asfortranarray(b.reshape(-1, 1)), "an Inf meets an underflowed product")[:, 0]
    assert (got[3:2 * L] == np.inf).all() and np.isnan(got[2 * L:]).all()
    a1, a2, b = overflow_example()
    got = check(a1, a2, np.asfortranarray(b.reshape(-1, 1)), "poles at 2 +- sqrt 3")[:, 0]
    assert not got[:T + 34 * L].any() and np.isnan(got[T + 34 * L:]).all()


# ---- 2. leaf kinds -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [T + L + 3, 2 * CH + T + 5])
def test_leaf_kinds_for_all_three_inputs(N):
    import torch

    for Cn in (1, 3):
        b, b32 = signal(N, Cn), signal(N, Cn, np.float32)
        a1, a2 = coef("reson", N, Cn)
        r1, r2 = coef("u1h", N, 1)
        want, want32, want1 = recur2_ref(a1, a2, b), recur2_ref(a1, a2, b32), recur2_ref(r1, r2, b)
        tree = lambda x1, x2, xb: so.Recur2(so.Signal(x1, FS), so.Signal(x2, FS), so.Signal(xb, FS))  # noqa: E731
        got = so.sink(tree(a1, a2, b32), so.Array)
        assert got.dtype == np.float64
        bit_equal(got, want32, "a Float32 b")
        f1, f2 = a1.astype(np.float32), a2.astype(np.float32)
        bit_equal(so.sink(tree(f1, a2, b), so.Array), recur2_ref(f1, a2, b), "a Float32 a1")
        bit_equal(so.sink(tree(a1, f2, b), so.Array), recur2_ref(a1, f2, b), "a Float32 a2")
        inter = [np.ascontiguousarray(v) for v in (a1, a2, b)]  # frames x channels, C order: frame stride = channels
        assert inter[2].strides == (8 * Cn, 8)
        for k in range(3):
            args = [a1, a2, b]
            args[k] = inter[k]
            bit_equal(so.sink(tree(*args), so.Array), want, f"input {k} C-ordered")
        bit_equal(so.sink(tree(*inter), so.Array), want, "all three C-ordered")
        for k in range(3):  # every second row and column of a larger array
            big = np.asfortranarray(np.random.default_rng(5).standard_normal((2 * N, 2 * Cn)))
            big[::2, ::2] = (a1, a2, b)[k]
            args = [a1, a2, b]
            args[k] = big[::2, ::2]
            bit_equal(so.sink(tree(*args), so.Array), want, f"input {k} strided")
        got, fs = so.sink(tree(dev(a1), dev(a2), dev(b)), "torch")
        assert fs == 10_000.0 and got.is_cuda
        bit_equal(got.cpu().numpy(), np.ascontiguousarray(want), "planar device tensors, device result")
        bit_equal(so.sink(tree(dev(r1), dev(r2), dev(b32)), so.Array), recur2_ref(r1, r2, b32), "device rows for every channel, Float32 device b")
        bit_equal(so.sink(tree(dev(f1), dev(a2), dev(b)), so.Array), recur2_ref(f1, a2, b), "a Float32 device a1")
        bit_equal(so.sink(tree(*[torch.from_numpy(v).cuda() for v in inter]), so.Array), want, "C-ordered device tensors")
        out = torch.full((Cn, N + 1), 7.0, dtype=torch.float64, device="cuda")[:, 1:].t()  # rows that start 8 bytes off a 16-byte boundary
        so.sink_into(out, tree(dev(r1), dev(r2), dev(b)))
        bit_equal(out.cpu().numpy(), np.ascontiguousarray(want1), "sink_into a device tensor, unaligned rows")
        bit_equal(so.sink(tree(dev(a1), dev(a2), dev(b)[1:]), so.Array), recur2_ref(a1[:N - 1], a2[:N - 1], b[1:]), "an unaligned device b")
        bit_equal(so.sink(tree(dev(a1)[1:], dev(a2), dev(b)[:N - 1]), so.Array), recur2_ref(a1[1:], a2[:N - 1], b[:N - 1]), "an unaligned device a1")
        bit_equal(so.sink(tree(dev(a1), dev(a2)[1:], dev(b)[:N - 1]), so.Array), recur2_ref(a1[:N - 1], a2[1:], b[:N - 1]), "an unaligned device a2")
        res = np.zeros((N, Cn), order="F")
        so.sink_into(res, tree(r1, r2, b))
        bit_equal(res, want1, "sink_into a host array")
        l1, l2 = coef("reson", N + 1000, Cn)
        bit_equal(so.sink(tree(l1, l2, b), so.Array), recur2_ref(l1, l2, b), "coefficients longer than b")
        tone = so.Signal(np.sin, FS, ω=50 * so.Hz)  # a formula, as each input in turn
        m = sunk(tone | so.Until(N * so.frames))
        half = so.OperateOn(so.elementwise(lambda v: 0.5 * v), tone)
        mh = sunk(half | so.Until(N * so.frames))
        bit_equal(so.sink(so.Recur2(so.Signal(r1, FS), so.Signal(r2, FS), tone | so.Until(N * so.frames)), so.Array), recur2_ref(r1, r2, m), "a formula b")
        bit_equal(so.sink(so.Recur2(tone, so.Signal(r2, FS), so.Signal(b, FS)), so.Array), recur2_ref(m, r2, b), "a formula a1")
        bit_equal(so.sink(so.Recur2(so.Signal(r1, FS), half, so.Signal(b, FS)), so.Array), recur2_ref(r1, mh, b), "a formula a2")


# ---- 3. sub-trees as inputs ------------------------------------------------------------------------------------------------
def test_sub_trees_as_inputs():
    N = CH + T + 37
    raw = signal(N + 1000, 2)
    rawa = coef("u1h", N + 1000, 2)[0]
    half = so.elementwise(lambda v: 0.5 * v + 0.25)
    children = (("a traced elementwise map", so.OperateOn(half, so.Signal(rawa, FS))),
                ("Filt", so.Signal(raw, FS) | so.Filt(so.Highpass, 1 * so.kHz)),
                ("ToFramerate", so.Signal(raw, FS) | so.ToFramerate(12 * so.kHz)),
                ("Cumsum", so.Cumsum(so.Amplify(so.Signal(raw, FS), 1e-3))),
                ("Recur", so.Recur(0.9, so.Amplify(so.Signal(raw, FS), 0.05))))
    for name, child in children:
        mid = sunk(child)  # the child, sunk separately; every form below asks it for the same frames, all of them
        n, ch = mid.shape
        assert np.isfinite(mid).all() and np.ptp(mid) > 0 and n > CH
        ob = signal(n, 2)
        o1, o2 = coef("u1h", n, ch)
        rate = child.fs * so.Hz
        got = so.sink(so.Recur2(1.2, -0.5, child), so.Array)
        bit_equal(got.reshape(n, ch), recur2_ref(1.2, -0.5, mid), f"b = {name}, constants")
        got = so.sink(so.Recur2(so.Signal(o1, rate), so.Signal(o2, rate), child), so.Array)
        bit_equal(got.reshape(n, ch), recur2_ref(o1, o2, mid), f"b = {name}")
        scaled = so.OperateOn(so.elementwise(lambda v: 0.01 * v), child) if name in ("Cumsum", "Filt", "ToFramerate") else child
        ms = sunk(scaled)
        bit_equal(so.sink(so.Recur2(scaled, so.Signal(o2, rate), so.Signal(ob, rate)), so.Array), recur2_ref(ms, o2, ob), f"a1 = {name}")
        bit_equal(so.sink(so.Recur2(so.Signal(o1, rate), scaled, so.Signal(ob, rate)), so.Array), recur2_ref(o1, ms, ob), f"a2 = {name}")
    x = signal(2 * CH + 77, 2)
    bit_equal(so.sink(so.Signal(x, FS) | so.Recur2(0.9, -0.5) | so.Recur2(0.2, 0.1), so.Array), recur2_ref(0.2, 0.1, recur2_ref(0.9, -0.5, x)), "Recur2(Recur2(x))")
    shared = so.Signal(x, FS) | so.Recur2(0.9, -0.5)  # one node read as a coefficient and as b of another
    mid = recur2_ref(0.9, -0.5, x)
    bit_equal(so.sink(so.Recur2(so.OperateOn(so.elementwise(lambda v: 0.01 * v), shared), -0.25, shared), so.Array),
              recur2_ref(np.asfortranarray(0.01 * mid), -0.25, mid), "one Recur2 as two inputs of another")


# ---- 4. windows and streams --------------------------------------------------------------------------------------------------
def test_windows_and_streams_equal_the_whole_sink():
    """the tree depends on the frame index only: `After` / `Until` over the node and blocks of a size that does not divide
    1024 give the slice of the whole sink bit for bit; the window that starts at CH + 1 is entered by a state whose two
    frames lie in two chunks"""
    N = 2 * CH + T + 11
    b = signal(N, 2)
    a1, a2 = coef("reson", N, 1)
    tone = so.Signal(np.sin, FS, ω=50 * so.Hz) | so.Until(N * so.frames)
    trees = (("arrays", so.Recur2(so.Signal(a1, FS), so.Signal(a2, FS), so.Signal(b, FS)), recur2_ref(a1, a2, b)),
             ("constants", so.Recur2(1.8, -0.9, so.Signal(b, FS)), recur2_ref(1.8, -0.9, b)),
             ("formula b", so.Recur2(so.Signal(a1, FS), -0.5, tone), None),
             ("map a1", so.Recur2(so.Amplify(so.Signal(a1, FS), 0.5), so.Signal(a2, FS), so.Signal(b, FS)), recur2_ref(np.asfortranarray(a1 * 0.5), a2, b)))
    for name, tree, want in trees:
        whole = so.sink(tree, so.Array)
        whole = whole.reshape(whole.shape[0], -1)
        if want is not None:
            bit_equal(whole, want, name)
        for s, n in ((1, 5), (2, 3), (L + 3, 2 * T + 1), (T - 1, CH), (CH + 1, T + 2), (CH + 5, CH + T + 2)):
            got = so.sink(tree | so.After(s * so.frames) | so.Until(n * so.frames), so.Array)
            bit_equal(got.reshape(n, -1), whole[s:s + n], f"{name}: After({s}) | Until({n})")
        got = so.sink(tree | so.Until((CH + 1) * so.frames), so.Array)
        bit_equal(got.reshape(CH + 1, -1), whole[:CH + 1], f"{name}: Until")
        got = so.sink(tree | so.After((CH + 1) * so.frames), so.Array)
        bit_equal(got.reshape(N - CH - 1, -1), whole[CH + 1:], f"{name}: After(CH + 1)")
        blocks = np.vstack([np.asarray(blk).reshape(len(blk), -1) for blk in so.stream(tree, 13000, so.Array)])  # three blocks
        bit_equal(blocks, whole, f"{name}: three blocks of 13000")


# ---- 5. consumers, and the structural algebra --------------------------------------------------------------------------------
def test_consumers_behind_the_node():
    """each consumer over the node equals the consumer over the sunk node.  Maps and `SampleAt` are the same operations on
    the same values whichever way they read them: bit for bit.  `Filt`, `ToFramerate` and `Normpower` choose their
    chunking, tables and reduction order by the plan they are in: 1e-8 norm-wise."""
    N = 2 * CH + 77
    x = signal(N, 2)
    xs = so.Signal(x, FS)
    mid = recur2_ref(1.2, -0.5, x)
    tree = so.Recur2(1.2, -0.5, xs)
    bit_equal(so.sink(tree, so.Array), mid)
    got = so.sink(so.Mix(xs, tree), so.Array)
    bit_equal(got, so.sink(so.Mix(xs, so.Signal(mid, FS)), so.Array), "Recur2 | Operate(+): Mix(x, .)")
    bit_equal(got, np.asfortranarray(x + mid), "Mix(x, .) against NumPy")
    half = so.elementwise(lambda v: 0.5 * v + 1.0)
    bit_equal(so.sink(so.OperateOn(half, tree), so.Array), so.sink(so.OperateOn(half, so.Signal(mid, FS)), so.Array), "Recur2 | Operate(elementwise)")
    pos = so.Signal(np.asfortranarray(np.linspace(0.0, N - 2.0, 5000).reshape(-1, 1)), FS)
    bit_equal(so.sink(so.SampleAt(tree, pos), so.Array), so.sink(so.SampleAt(so.Signal(mid, FS), pos), so.Array), "SampleAt over Recur2")
    for name, tail in (("Filt(Highpass)", lambda t: t | so.Filt(so.Highpass, 1 * so.kHz)),
                       ("ToFramerate", lambda t: t | so.ToFramerate(12 * so.kHz)),
                       ("Normpower", lambda t: t | so.Normpower)):
        got = so.sink(tail(tree), so.Array)
        want = so.sink(tail(so.Signal(mid, FS)), so.Array)
        assert np.ptp(want) > 0.1
        close(got, want, f"Recur2 | {name}")


def test_the_node_under_and_over_append_pad_and_mix():
    """written when tests/tree_ref.py `evaluate` knew the structural nodes and not this one, and kept as it was: under them
    the node is replaced by an array of its definition's values, over them the child is evaluated and handed to the
    definition.  `evaluate` has the node now, and tests/test_gpu_node_trees.py holds it to the whole composite matrix: windows
    at odd frames of every result form, 1 and 3 channels, several readers, windows, blocks and random trees"""
    n = CH + T + 9
    x, z = signal(n, 2), signal(700, 2, seed=3)
    a1, a2 = coef("reson", n + 700, 1)
    node = lambda: so.Recur2(so.Signal(a1[:n], FS), so.Signal(a2[:n], FS), so.Signal(x, FS))  # noqa: E731
    mid = so.Signal(recur2_ref(a1[:n], a2[:n], x), FS)
    zs = so.Signal(z, FS)
    under = (("Append(z, node)", lambda v: so.Append(zs, v)), ("Append(node, z)", lambda v: so.Append(v, zs)),
             ("Append(node, node)", lambda v: so.Append(v, v)),
             ("Pad(node, 0) | Until", lambda v: so.Pad(v, so.zero) | so.Until((n + 500) * so.frames)),
             ("Pad(node, lastframe) | Until", lambda v: so.Pad(v, so.lastframe) | so.Until((n + 500) * so.frames)),
             ("Mix(node, z)", lambda v: so.Mix(v, zs)), ("Mix(z, node, node)", lambda v: so.Mix(zs, v, v)),
             ("Amplify(node, z)", lambda v: so.Amplify(v, zs)),
             ("Append(z, node) | After | Until", lambda v: so.Append(zs, v) | so.After(300 * so.frames) | so.Until((CH + 500) * so.frames)))
    for name, make in under:
        bit_equal(so.sink(make(node()), so.Array), evaluate(make(mid)), name)
    xs = so.Signal(x, FS)
    over = (("b = Append(z, x)", so.Append(zs, xs)), ("b = Pad(z, 1) | Until", so.Pad(zs, so.one) | so.Until((n + 700) * so.frames)),
            ("b = Mix(x, z)", so.Mix(xs, zs)), ("b = Append(x, z) | After", so.Append(xs, zs) | so.After(5 * so.frames)))
    for name, child in over:
        m = evaluate(child)
        k = m.shape[0]
        bit_equal(so.sink(so.Recur2(so.Signal(a1, FS), so.Signal(a2, FS), child), so.Array), recur2_ref(a1[:k], a2[:k], m), name)
        bit_equal(so.sink(so.Recur2(0.9, -0.5, child), so.Array), recur2_ref(0.9, -0.5, m), name + ", constants")
    ca = so.Append(so.Signal(a1[:700], FS), so.Signal(a1[700:n], FS))  # a coefficient of two pieces
    bit_equal(so.sink(so.Recur2(ca, so.Signal(a2, FS), xs), so.Array), recur2_ref(a1[:n], a2[:n], x), "a1 = Append of two arrays")
    bit_equal(so.sink(so.Recur2(so.Signal(a1, FS), so.Mix(so.Signal(a2, FS), 0.01), xs), so.Array), recur2_ref(a1[:n], np.asfortranarray(a2[:n] + 0.01), x), "a2 = Mix")


# ---- 6. the wrappers ---------------------------------------------------------------------------------------------------------
def test_delay_by_whole_frames_is_a_bit_copy():
    """what `Sweep` builds its taps from: `Delay(x, k)` of Float64 and of Float32 data, zeros of both signs, infinities and NaNs
    included, is x delayed by k frames, widened to Float64, with +0.0 in front"""
    for dtype in (np.float64, np.float32):
        x = planted(signal(CH + 5, 3, dtype))
        for k in (1, 2):
            bit_equal(so.sink(so.Delay(so.Signal(x, FS), k), so.Array), np.asfortranarray(delayed(x, k).astype(np.float64)), f"Delay({k}) {np.dtype(dtype).name}")


def test_resonator_and_sweep_with_constants():
    """only `math` on the host forms the coefficients: bit for bit against the NumPy formulas fed to recur2_ref"""
    N = CH + T + 5
    x, x32 = signal(N, 2), signal(N, 2, np.float32)
    a1, a2, g = resonator_coefs(440.0, 20.0, 10_000.0)
    bit_equal(so.sink(so.Resonator(so.Signal(x, FS), 440 * so.Hz, 20 * so.Hz), so.Array), recur2_ref(a1, a2, np.asfortranarray(x * g)), "Resonator")
    bit_equal(so.sink(so.Signal(x32, FS) | so.Resonator(440.0, 20.0), so.Array), recur2_ref(a1, a2, np.asfortranarray(x32.astype(np.float64) * g)), "Resonator(Float32)")
    for kind, name in ((so.Lowpass, "lowpass"), (so.Highpass, "highpass"), (so.Bandpass, "bandpass")):
        for q in (0.5 ** 0.5, 8.0):
            a1, a2, c0, c1, c2 = sweep_coefs(name, 300.0, q, 10_000.0)
            bit_equal(so.sink(so.Sweep(so.Signal(x, FS), kind, 300 * so.Hz, q), so.Array), recur2_ref(a1, a2, sweep_input(x, c0, c1, c2)), f"Sweep {name} q={q}")
        bit_equal(so.sink(so.Signal(x32, FS) | so.Sweep(kind, 300.0, q=8.0), so.Array), recur2_ref(a1, a2, sweep_input(x32, c0, c1, c2)), f"Sweep {name} (Float32)")


def test_resonator_and_sweep_with_signal_arguments():
    """device `exp`, `sin` and `cos` form the coefficients: the node is held to recur2_ref fed with its three sub-trees sunk
    on their own, bit for bit, and to the NumPy formulas to 1e-8"""
    N = CH + T + 5
    x = signal(N, 2)
    xs = so.Signal(x, FS)
    fcv = np.asfortranarray(300.0 + 200.0 * np.sin(np.arange(N) / 300.0).reshape(-1, 1))
    qv = np.asfortranarray(1.0 + 0.5 * np.abs(signal(N, 2)))  # a resonance per channel
    bwv = np.asfortranarray(10.0 + 5.0 * np.abs(signal(N, 1, seed=2)))
    fc, q, bw = so.Signal(fcv, FS), so.Signal(qv, FS), so.Signal(bwv, FS)
    fc_inf = so.OperateOn(so.elementwise(lambda v: 400.0 + 100.0 * v), so.Signal(np.sin, FS, ω=2 * so.Hz))
    fci = sunk(fc_inf | so.Until(N * so.frames))
    # (each case compiles three traced maps; every wrapper, response and argument form is met once)
    cases = [("Resonator(fc signal)", so.Resonator(xs, fc, 20 * so.Hz), resonator_coefs(fcv, 20.0, 10_000.0)),
             ("Resonator(infinite fc, bw signal)", so.Resonator(xs, fc_inf, bw), resonator_coefs(fci, bwv, 10_000.0)),
             ("Sweep lowpass(fc, q signals)", so.Sweep(xs, so.Lowpass, fc, q), sweep_coefs("lowpass", fcv, qv, 10_000.0)),
             ("Sweep highpass(fc signal)", so.Sweep(xs, so.Highpass, fc, 2.0), sweep_coefs("highpass", fcv, 2.0, 10_000.0)),
             ("Sweep bandpass(q signal)", so.Sweep(xs, so.Bandpass, 300.0, q), sweep_coefs("bandpass", 300.0, qv, 10_000.0))]
    for name, y, formula in cases:
        assert isinstance(y, so.Recur2Signal) and y.coefs is not None
        m1, m2, mb = sunk(y.coefs[0] | so.Until(N * so.frames)), sunk(y.coefs[1] | so.Until(N * so.frames)), sunk(y.signal)
        got = so.sink(y, so.Array)
        bit_equal(got, recur2_ref(m1, m2, mb), name)
        a1, a2 = formula[:2]  # (numbers, one row or a row per channel: recur2_ref takes each)
        b = np.asfortranarray(formula[2] * x) if len(formula) == 3 else sweep_input(x, *formula[2:])
        close(got, recur2_ref(a1, a2, b), f"{name} against the NumPy formulas")


def test_constant_coefficients_against_filt_with_the_same_biquad():
    """`Recur2` with the cookbook low-pass's a1, a2 over the feed-forward taps against `Filt` with the same `Biquad` on the
    device, to 1e-8"""
    N = 2 * CH + 77
    x = signal(N, 2)
    a1, a2, c0, c1, c2 = sweep_coefs("lowpass", 1000.0, 2.0, 10_000.0)
    got = so.sink(so.Sweep(so.Signal(x, FS), so.Lowpass, 1 * so.kHz, 2.0), so.Array)
    want = so.sink(so.Signal(x, FS) | so.Filt(so.Biquad(c0, c1, c2, -a1, -a2)), so.Array)
    assert np.ptp(want) > 0.1
    close(got, want, "Sweep against Filt(Biquad)")


# ---- 7. plan reuse and step information ----------------------------------------------------------------------------------
def test_a_plan_is_reused_after_set_array_on_each_input():
    import torch

    N = 2 * CH + T + 3
    bs = [signal(N, 2, seed=k) for k in range(3)]
    cs = [coef("reson", N, 2, seed=k) for k in range(3)]
    res = np.zeros((N, 2), order="F")
    p = Plan(so.Recur2(so.Signal(cs[0][0], FS), so.Signal(cs[0][1], FS), so.Signal(bs[0], FS)), res.shape, res.dtype, (1, res.shape[0]), False)
    scratch = p.stats()["scratch_bytes"]
    for i, j, k in ((0, 0, 0), (1, 0, 0), (1, 2, 0), (1, 2, 1), (2, 1, 1), (0, 0, 0)):
        p.set_array(0, cs[i][0])
        p.set_array(1, cs[j][1])
        p.set_array(2, bs[k])
        p.execute(res.ctypes.data)
        bit_equal(res, recur2_ref(cs[i][0], cs[j][1], bs[k]), f"host leaves a1 {i} a2 {j} b {k}")
        assert p.stats()["scratch_bytes"] == scratch
    p.close()
    d1, d2, db = [dev(v[0]) for v in cs], [dev(v[1]) for v in cs], [dev(v) for v in bs]
    out = torch.empty((2, N), dtype=torch.float64, device="cuda").t()
    p = Plan(so.Recur2(so.Signal(d1[0], FS), so.Signal(d2[0], FS), so.Signal(db[0], FS)), (N, 2), np.float64, (1, N), True)
    for i, j, k in ((0, 0, 0), (0, 0, 0), (1, 0, 0), (1, 1, 2), (2, 0, 2), (2, 2, 1)):
        p.set_array(0, d1[i])
        p.set_array(1, d2[j])
        p.set_array(2, db[k])
        p.execute(out.data_ptr())
        p.check()
        bit_equal(out.cpu().numpy(), np.ascontiguousarray(recur2_ref(cs[i][0], cs[j][1], bs[k])), f"device leaves a1 {i} a2 {j} b {k}")
        s = p.stats()
        assert s["h2d_bytes"] == 0 and s["d2h_bytes"] == 0 and s["scratch_bytes"] <= 4096  # all read where they lie; the chunk composites
    p.close()


def test_step_info_names_the_kernel_and_counts_its_bytes():
    import torch

    for N, launches in ((2 * CH + 5, 3), (CH, 1)):
        for dtype, esz in ((np.float64, 8), (np.float32, 4)):
            b = dev(signal(N, 3, dtype))
            out = torch.empty((3, N), dtype=torch.float64, device="cuda").t()
            one, per = coef("reson", N, 1), coef("reson", N, 3)
            for a1, a2, abytes in ((0.5, 0.25, 0), (so.Signal(dev(one[0]), FS), so.Signal(dev(one[1]), FS), 32),
                                   (so.Signal(dev(per[0]), FS), so.Signal(dev(one[1]), FS), 64), (so.Signal(dev(per[0]), FS), so.Signal(dev(per[1]), FS), 96)):
                p = Plan(so.Recur2(a1, a2, so.Signal(b, FS)), (N, 3), np.float64, (1, N), True)
                p.set_profiling(True)
                p.execute(out.data_ptr(), torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                steps = p.steps()
                p.close()
                assert [s["name"] for s in steps] == ["k_recur2"], steps
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
    one = so.Signal(coef("u1h", 64, 1)[0], FS)
    invalid, length, unsupported = -1, -2, -3  # include/sigops.h so_status_t: SO_ERR_INVALID, SO_ERR_LENGTH, SO_ERR_UNSUPPORTED
    lw = LW.lower(so.Recur2(0.5, 0.25, b))
    assert _create(lw, 64, 3)[0] == 0  # the well-formed nodes
    assert _create(LW.lower(so.Recur2(one, 0.25, b)), 64, 3)[0] == 0
    n = lw.root
    assert lw.nodes[n].kind == K.NODE_RECUR2 == 18
    for field in ("d0", "d1"):
        for bad in (np.inf, np.nan):
            setattr(lw.nodes[n], field, bad)
            st, err = _create(lw, 64, 3)
            assert st == invalid and f"node {n}" in err and "Recur2" in err and "finite constants a1 and a2" in err, err
        setattr(lw.nodes[n], field, 0.5)
    four = (C.c_int32 * 4)(0, 0, 0, 0)
    kids = lw.nodes[n].children
    lw.nodes[n].children = C.cast(four, C.POINTER(C.c_int32))
    for count in (2, 4, 0):
        lw.nodes[n].n_children = count
        st, err = _create(lw, 64, 3)
        assert st == invalid and "Recur2" in err and "one child" in err and "or three" in err, err
    lw.nodes[n].children = kids
    lw.nodes[n].n_children = 1
    assert _create(lw, 64, 3)[0] == 0
    # what the host refuses to build: the nodes are made by hand
    two = so.Signal(coef("u1h", 64, 2)[0], FS)
    st, err = _create(LW.lower(S.Recur2Signal(two, one, b)), 64, 3)
    assert st == invalid and "Recur2" in err and "a1 have 2 channels: 1 or b's 3" in err, err
    st, err = _create(LW.lower(S.Recur2Signal(one, two, b)), 64, 3)
    assert st == invalid and "Recur2" in err and "a2 have 2 channels: 1 or b's 3" in err, err
    st, err = _create(LW.lower(S.Recur2Signal(0.5, 0.25, so.Signal(np.sin, FS, ω=5 * so.Hz))), 64, 1)
    assert st == length and "Recur2" in err and "finite length" in err, err
    short = so.Signal(coef("u1h", 10, 1)[0], FS)
    st, err = _create(LW.lower(S.Recur2Signal(short, one, b)), 64, 3)
    assert st == length and "Recur2" in err and "a1 have 10 frames, fewer than b's 64" in err, err
    st, err = _create(LW.lower(S.Recur2Signal(one, short, b)), 64, 3)
    assert st == length and "Recur2" in err and "a2 have 10 frames, fewer than b's 64" in err, err
    st, err = _create(LW.lower(S.Recur2Signal(0.5, 0.25, so.Signal(5, FS) | so.Until(64 * so.frames))), 64, 1)  # an Int64 constant
    assert st == unsupported and "Recur2" in err and "Float32 or Float64 signal b" in err, err
    st, err = _create(LW.lower(S.Recur2Signal(so.Signal(5, FS), one, b)), 64, 3)
    assert st == unsupported and "Recur2" in err and "Float32 or Float64 signal a1" in err, err
    st, err = _create(LW.lower(S.Recur2Signal(one, so.Signal(5, FS), b)), 64, 3)
    assert st == unsupported and "Recur2" in err and "Float32 or Float64 signal a2" in err, err


def test_blockstream_and_shards_refuse_the_node_by_name():
    x = so.Signal(signal(4096, 2), FS)
    for tree in (so.Recur2(0.5, 0.25, x), so.Resonator(x, 1 * so.kHz, 10 * so.Hz), so.Sweep(x, so.Lowpass, 1 * so.kHz)):
        with pytest.raises(so.ErrorException, match="BlockStream: Recur2"):
            engine._streamable(tree | so.Filt(so.Lowpass, 1 * so.kHz))
        with pytest.raises(so.ErrorException, match="BlockStream: Recur2"):
            engine._streamable(so.Mix(tree, 1.0))
    for make in (lambda: sharding.shard_time(so.Recur2(0.5, 0.25, x), 0, 2), lambda: sharding.shard_channels(so.Resonator(x, 1 * so.kHz, 10.0), 1, 2),
                 lambda: sharding.shard_append(so.Append(so.Recur2(0.5, 0.25, x), x), 0, 2)):
        with pytest.raises(so.ErrorException, match="Recur2 / Resonator / Sweep over several GPUs is not built"):
            make()
