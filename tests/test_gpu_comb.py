"""`Comb(x, d, g)` and `Allpass(x, d, g)` on the device (include/sigops.h SO_NODE_COMB; csrc/k_comb.hip), through the public
interface and the C-ABI: bit for bit against the NumPy definition (tests/comb_ref.py comb_ref) -- no tolerance, the
arithmetic is specified operation by operation.  The definition is held to its scalar restatement, to closed forms and to
`scipy.signal.lfilter` without a GPU in tests/test_comb_host.py."""
import ctypes as C

import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import _capi as K
from sigops_amd import lowering as LW
from sigops_amd import signals as S
from sigops_amd.engine import Plan
from oracle_bridge import relerr
from comb_ref import CHANNELS, DELAYS, FORMS, allpass, comb, comb_ref, lengths, planted, same_bits, signal, unroll

pytestmark = pytest.mark.gpu
FS = 10 * so.kHz
U = unroll()


def bit_equal(got, want, what=""):
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} samples differ, first at {np.argwhere(bad)[0]}"
    assert same_bits(got, want), f"{what}: a zero of the other sign"


def node(x, D, b0, bD, a):
    """the tree of the node (b0, bD, a) over the signal x, through the public constructors"""
    return so.Comb(x, D, a, feedforward=bD, direct=b0)


def check(x, D, b0, bD, a, what=""):
    got = so.sink(node(so.Signal(x, FS), D, b0, bD, a), so.Array)
    bit_equal(got, comb_ref(x, D, b0, bD, a), f"{what} D={D} N={x.shape[0]} C={x.shape[1]} ({b0}, {bD}, {a})")
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


# ---- 1. geometry -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DELAYS)
def test_every_delay_length_and_channel_count(D):
    """a wave, a workgroup, two workgroups plus one; lengths around the first recursion and around the ends of the
    kernel's unrolled loop"""
    for N in lengths(D, U):
        for Cn in CHANNELS:
            x = signal(N, Cn)
            check(x, D, 1.0, 0.0, 0.7, "comb")
            got = so.sink(so.Allpass(so.Signal(x, FS), D, 0.6), so.Array)
            bit_equal(got, allpass(x, D, 0.6), f"allpass D={D} N={N} C={Cn}")


def test_a_delay_longer_than_the_signal():
    x = signal(100, 3)
    for D in (100, 101, 5000, 1 << 40):
        check(x, D, 0.9, -0.35, 0.5, "long delay")


# ---- 2. coefficient forms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,b0,bD,a", FORMS)
def test_coefficient_forms(name, b0, bD, a):
    for D, N, Cn in ((1, 40, 3), (65, (U + 1) * 65 + 1, 3), (257, (2 * U + 1) * 257 + 3, 1), (1000, 4001, 8)):
        check(signal(N, Cn), D, b0, bD, a, name)
        check(signal(N, Cn, np.float32), D, b0, bD, a, name + " Float32")


def test_a_gain_above_one_runs_into_overflow_like_the_loop():
    for D, N in ((2, 200), (65, 65 * 40 + 7)):
        for g in (1e20, -1e20, -7.5e15):
            x = signal(N, 3)
            got = check(x, D, 1.0, 0.0, g, "overflow")
            assert np.isinf(got).any() and np.isfinite(got[:D]).all()
            got = check(planted(N, 3, D), D, 1.0, 0.0, g, "overflow, planted")
            assert np.isnan(got).any() and np.isinf(got).any()
            check(planted(N, 3, D), D, -g, 1.0, g, "overflow, all terms")


# ---- 3. planted values ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 64, 257])
def test_planted_zeros_infinities_and_nans(D):
    N = (U + 3) * D + 5
    for Cn in (1, 3):
        for dtype in (np.float64, np.float32):
            x = planted(N, Cn, D, dtype)
            for name, b0, bD, a in FORMS:
                check(x, D, b0, bD, a, f"planted {name}")


def test_an_inf_exactly_d_frames_before_a_finite_sample():
    D = 64
    x = signal(10 * D, 2)
    x[3 * D + 5, 0] = np.inf
    x[4 * D + 5, 0] = 1.25
    x[2 * D + 9, 1] = -np.inf
    got = check(x, D, 1.0, 0.0, 0.5, "the plain comb")  # bD == 0 is not multiplied: 0 * Inf never arises
    assert not np.isnan(got).any() and np.isinf(got[3 * D + 5::D, 0]).all() and np.isfinite(got[:3 * D + 5, 0]).all()
    got = check(x, D, 1.0, -1.0, 1.0, "feed-forward and feedback")  # Inf - Inf: the NaN the loop gives too
    assert np.isnan(got[4 * D + 5, 0])


# ---- 4. leaf kinds -------------------------------------------------------------------------------------------------------
def test_leaf_kinds():
    import torch

    D, N = 65, (U + 1) * 65 + 7
    for Cn in (1, 3):
        x = signal(N, Cn)
        want = comb_ref(x, D, 0.9, -0.35, 0.5)
        tree = lambda leaf: node(so.Signal(leaf, FS), D, 0.9, -0.35, 0.5)  # noqa: E731
        x32 = signal(N, Cn, np.float32)
        got = so.sink(tree(x32), so.Array)
        assert got.dtype == np.float64
        bit_equal(got, comb_ref(x32, D, 0.9, -0.35, 0.5), "a Float32 array")
        xi = np.ascontiguousarray(x)  # frames x channels, C order: frame stride = channels
        assert xi.strides == (8 * Cn, 8)
        bit_equal(so.sink(tree(xi), so.Array), want, "an interleaved host array")
        big = np.asfortranarray(np.random.default_rng(5).standard_normal((2 * N, 2 * Cn)))
        big[::2, ::2] = x
        bit_equal(so.sink(tree(big[::2, ::2]), so.Array), want, "a strided view")
        big32 = np.zeros((N, 2 * Cn), dtype=np.float32)  # C order, every second column
        big32[:, ::2] = x32
        bit_equal(so.sink(tree(big32[:, ::2]), so.Array), comb_ref(x32, D, 0.9, -0.35, 0.5), "a strided Float32 view")
        got, fs = so.sink(tree(dev(x)), "torch")
        assert fs == 10_000.0 and got.is_cuda
        bit_equal(got.cpu().numpy(), np.ascontiguousarray(want), "a planar device tensor, device result")
        bit_equal(so.sink(tree(dev(x32)), so.Array), comb_ref(x32, D, 0.9, -0.35, 0.5), "a planar Float32 device tensor")
        di = torch.from_numpy(xi).cuda()  # interleaved on the device
        bit_equal(so.sink(tree(di), so.Array), want, "an interleaved device tensor")


# ---- 5. a sub-tree as x ----------------------------------------------------------------------------------------------------
def test_a_sub_tree_as_x():
    raw = signal(6000, 2)
    pos = np.asfortranarray(np.linspace(0.0, 5999.0, 5000).reshape(-1, 1) + 3.0 * np.sin(np.arange(5000) / 50.0).reshape(-1, 1))
    children = (("Signal(sin) | Until", so.Signal(np.sin, FS, ω=50 * so.Hz) | so.Until(5000 * so.frames)),
                ("Filt", so.Signal(raw, FS) | so.Filt(so.Lowpass, 1 * so.kHz)),
                ("ToFramerate", so.Signal(raw, FS) | so.ToFramerate(12 * so.kHz)),
                ("SampleAt", so.SampleAt(so.Signal(raw, FS), so.Signal(pos, FS))),
                ("a map", so.Amplify(so.Signal(raw, FS), 0.25)))
    for name, child in children:
        mid = so.sink(child, so.Array)  # the child, sunk separately
        mid = np.asfortranarray(mid.reshape(mid.shape[0], -1))
        assert np.isfinite(mid).all() and np.ptp(mid) > 0.1
        for D in (7, 257):
            bit_equal(so.sink(so.Comb(child, D, 0.7), so.Array), comb(mid, D, 0.7), f"Comb({name}) D={D}")
            bit_equal(so.sink(so.Allpass(child, D, -0.5), so.Array), allpass(mid, D, -0.5), f"Allpass({name}) D={D}")


# ---- 6. nesting ------------------------------------------------------------------------------------------------------------
def test_nesting_and_a_schroeder_reverberator():
    x = signal(20_000, 2)
    xs = so.Signal(x, FS)
    bit_equal(so.sink(so.Comb(so.Comb(xs, 113, 0.6), 337, -0.5), so.Array), comb(comb(x, 113, 0.6), 337, -0.5), "Comb(Comb(x))")
    bit_equal(so.sink(xs | so.Allpass(347, 0.7) | so.Allpass(113, 0.7), so.Array), allpass(allpass(x, 347, 0.7), 113, 0.7), "two allpasses")
    combs = ((1687, 0.773), (1601, 0.802), (2053, 0.753), (2251, 0.733))
    for D, g in combs:
        bit_equal(so.sink(so.Comb(xs, D, g), so.Array), comb(x, D, g), f"comb {D}")
    mix = so.Mix(*[so.Comb(xs, D, g) for D, g in combs])
    m = so.sink(mix, so.Array)
    close(m, np.asfortranarray(sum(comb(x, D, g) for D, g in combs)), "the Mix of four combs")  # (K1's summation order is its own)
    rev = mix | so.Allpass(347, 0.7) | so.Allpass(113, 0.7)
    bit_equal(so.sink(rev, so.Array), allpass(allpass(m, 347, 0.7), 113, 0.7), "the allpasses behind the Mix")


# ---- 7. windows and streams --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 257])
def test_windows_and_streams_equal_the_whole_sink(D):
    """starts and lengths that are no multiples of D; blocks of 1000, D and D + 1 frames"""
    N = 20 * D + 11
    x = signal(N, 2)
    xs = so.Signal(x, FS)
    for tree, want in ((so.Comb(xs, D, 0.7), comb(x, D, 0.7)), (so.Allpass(so.Comb(xs, 113, -0.5), D, 0.6), allpass(comb(x, 113, -0.5), D, 0.6))):
        whole = so.sink(tree, so.Array)
        bit_equal(whole, want)
        for a, n in ((1, 5), (D + 3, 2 * D + 1), (3 * D - 1, D), (7 * D + 5, 9 * D + 2)):
            bit_equal(so.sink(tree | so.After(a * so.frames) | so.Until(n * so.frames), so.Array), whole[a:a + n], f"After({a}) | Until({n})")
        bit_equal(so.sink(tree | so.Until((5 * D + 3) * so.frames), so.Array), whole[:5 * D + 3], "Until")
        bit_equal(so.sink(tree | so.After((6 * D + 1) * so.frames), so.Array), whole[6 * D + 1:], "After")
        for bs in (1000, D, D + 1):
            bit_equal(np.vstack([b for b in so.stream(tree, bs, so.Array)]), whole, f"blocks of {bs}")


def test_windows_and_streams_over_a_filtered_child():
    """the node adds nothing to what its child does: a `Filt` chunks its input by the frames asked of it, so a window's
    filter output differs from the whole sink's in the last bits (K2's own contract, the Float64 one), and the comb above
    it carries exactly that"""
    D = 64
    x = signal(20 * D + 11, 2)
    tree = so.Allpass(so.Signal(x, FS) | so.Filt(so.Lowpass, 1 * so.kHz), D, 0.6)
    whole = so.sink(tree, so.Array)
    assert np.ptp(whole) > 0.1
    close(so.sink(tree | so.After((3 * D - 1) * so.frames) | so.Until(D * so.frames), so.Array), np.asfortranarray(whole[3 * D - 1:4 * D - 1]), "a window")
    for bs in (1000, D, D + 1):
        close(np.asfortranarray(np.vstack([b for b in so.stream(tree, bs, so.Array)])), whole, f"blocks of {bs}")


# ---- 8. consumers ------------------------------------------------------------------------------------------------------------
def test_consumers_behind_the_node():
    x = signal(30_000, 2)
    xs = so.Signal(x, FS)
    mid = comb(x, 257, 0.7)
    tree = so.Comb(xs, 257, 0.7)
    bit_equal(so.sink(tree, so.Array), mid)
    for name, tail in (("Filt(Highpass)", lambda t: t | so.Filt(so.Highpass, 1 * so.kHz)),
                       ("ToFramerate", lambda t: t | so.ToFramerate(12 * so.kHz)),
                       ("Normpower", lambda t: t | so.Normpower),
                       ("Mix(x, .)", lambda t: so.Mix(xs, t))):
        got = so.sink(tail(tree), so.Array)
        want = so.sink(tail(so.Signal(mid, FS)), so.Array)
        assert np.ptp(want) > 0.1
        close(got, want, f"Comb | {name}")


# ---- 9. plan reuse -------------------------------------------------------------------------------------------------------
def test_a_plan_is_reused_after_set_array():
    import torch

    D, N = 65, (U + 2) * 65 + 3
    xs = [signal(N, 2, seed=k) for k in range(3)]
    res = np.zeros((N, 2), order="F")
    p = Plan(so.Allpass(so.Signal(xs[0], FS), D, 0.6), res.shape, res.dtype, (1, res.shape[0]), False)
    scratch = p.stats()["scratch_bytes"]
    for k in (0, 1, 1, 2, 0):
        p.set_array(0, xs[k])
        p.execute(res.ctypes.data)
        bit_equal(res, allpass(xs[k], D, 0.6), f"host leaf {k}")
        assert p.stats()["scratch_bytes"] == scratch
    p.close()
    dx = [dev(a) for a in xs]
    out = torch.empty((2, N), dtype=torch.float64, device="cuda").t()
    p = Plan(so.Comb(so.Signal(dx[0], FS), D, 0.7), (N, 2), np.float64, (1, N), True)
    for k in (0, 0, 0, 1, 1, 2, 2, 2):
        p.set_array(0, dx[k])
        p.execute(out.data_ptr())
        p.check()
        bit_equal(out.cpu().numpy(), np.ascontiguousarray(comb(xs[k], D, 0.7)), f"device leaf {k}")
        s = p.stats()
        assert s["h2d_bytes"] == 0 and s["d2h_bytes"] == 0 and s["scratch_bytes"] <= 4096  # x is read where it lies
    p.close()


# ---- 10. malformed node tables -------------------------------------------------------------------------------------------
def _create(lw, nframes, nch):
    out = K.so_out_desc_t(dtype=K.SO_F64, nch=nch, nframes=nframes, frame_stride=1, chan_stride=nframes, is_device=0)
    plan = C.c_void_p()
    st = K.lib().so_plan_create(lw.nodes, lw.n, lw.root, C.byref(out), 0, C.byref(plan))
    if plan.value:
        K.lib().so_plan_destroy(plan)
    return st, K.last_error() if st else ""


def test_malformed_nodes_are_refused():
    x = so.Signal(signal(64, 3), FS)
    lw = LW.lower(so.Comb(x, 7, 0.5))
    assert _create(lw, 64, 3)[0] == 0  # the well-formed node
    n = lw.root
    assert lw.nodes[n].kind == K.NODE_COMB
    invalid, length, unsupported = -1, -2, -3  # include/sigops.h so_status_t: SO_ERR_INVALID, SO_ERR_LENGTH, SO_ERR_UNSUPPORTED
    two = (C.c_int32 * 2)(0, 0)
    kids = lw.nodes[n].children
    lw.nodes[n].children = C.cast(two, C.POINTER(C.c_int32))
    lw.nodes[n].n_children = 2
    st, err = _create(lw, 64, 3)
    assert st == invalid and f"node {n}" in err and "Comb" in err and "one child" in err, err
    lw.nodes[n].n_children = 0
    st, err = _create(lw, 64, 3)
    assert st == invalid and "Comb" in err and "one child" in err, err
    lw.nodes[n].children = kids
    lw.nodes[n].n_children = 1
    for d in (0, -5):
        lw.nodes[n].l0 = d
        st, err = _create(lw, 64, 3)
        assert st == invalid and f"node {n}" in err and "Comb" in err and "at least one frame" in err, err
    lw.nodes[n].l0 = 7
    for field in ("d0", "d1", "d2"):
        for v in (np.inf, -np.inf, np.nan):
            keep = getattr(lw.nodes[n], field)
            setattr(lw.nodes[n], field, v)
            st, err = _create(lw, 64, 3)
            assert st == invalid and "Comb" in err and "finite coefficients" in err, err
            setattr(lw.nodes[n], field, keep)
    assert _create(lw, 64, 3)[0] == 0
    # an infinite child and an integer child (the host refuses to build them: the nodes are made by hand)
    st, err = _create(LW.lower(S.CombSignal(so.Signal(np.sin, FS, ω=5 * so.Hz), 7, 1.0, 0.0, 0.5)), 64, 1)
    assert st == length and "Comb" in err and "finite length" in err, err
    st, err = _create(LW.lower(S.CombSignal(so.Signal(5, FS) | so.Until(64 * so.frames), 7, 1.0, 0.0, 0.5)), 64, 1)  # an Int64 constant
    assert st == unsupported and "Comb" in err and "Float32 or Float64" in err, err
