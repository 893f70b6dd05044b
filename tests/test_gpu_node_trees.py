"""The device-only nodes (`SampleAt` linear, cubic and sinc, `Comb` / `Allpass`, `Cumsum`, `MovingMax` / `MovingMin`,
`MovingSum` / `MovingMean` / `MovingRMS`, `Recur` / `PeakDecay`, `Recur2`, `MovingMedian` / `MovingQuantile`) next to the
planner's structural algebra: under a root `Append` (window aliasing:
`Plan::try_window_alias`, the `win_off` term of `stage_out()`), behind `Pad`, `ToChannels`, `Mix` and `Amplify` of unequal
lengths (the maps `m.sf == 0` and `m.sc == 0` that `Plan::use_stage` merges), over `Append` / `Pad` / `Mix` (a child of several
pieces, `Plan::second_input`), read by several parents (`S.lo`, a union of ranges), and windows and `stream` blocks of such
trees.  Every result is compared bit for bit, -0.0 included, with tests/tree_ref.py `evaluate`, which calls the families'
own NumPy definitions and never the engine; the one exception, the `Append` that mixes a filter, a `Cumsum` and a
resampler, states its tolerance.  The random trees' generator and its statistics are held without a GPU in
tests/test_tree_ref_host.py.

A stage that writes its window of the result itself meets destinations its own file never gives it, and the kernels of the
three newest families choose their store path by the destination's alignment: k_movrank stores vectors of 16 bytes or single
samples (`vy`), k_recur2's scan has an instantiation for unaligned rows, and the cubic and sinc `SampleAt` shift their pairs of
frames by one in a row that starts 8 bytes off a 16-byte boundary.  So the root `Append`s here put windows at odd frames of
Float64 results, at every 4-byte phase of Float32 results, and into device results of 1, 2 and 3 channels with an odd
number of frames, whose rows alternate in alignment.

`Pad(node, cycle)` and `Pad(node, mirror)` are refused by design (an indexing pad reads an array leaf, here as in the
reference): the test pins the refusal, and the two pad kinds run under the nodes instead."""
import os

import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import signals as S
from oracle_bridge import relerr
from comb_ref import DELAYS
from cumsum_ref import CH, L, T, cumsum_ref
from moving_ref import same_bits
from movingsum_ref import B, TILE
from recur2_ref import coef
from tree_ref import FS, SEEDS, SEEDS_ALL, evaluate, random_trees

pytestmark = pytest.mark.gpu
fr = so.frames


def bit_equal(got, want, what=""):
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} against {want.dtype} {want.shape}"
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} samples differ, first at {np.argwhere(bad)[0]}"
    assert same_bits(got, want), f"{what}: a zero of the other sign"


def data(n, c, seed=0, dtype=np.float64):
    """normal samples, zeros of both signs at the kernels' boundaries"""
    x = np.random.default_rng(1000 * n + 10 * c + seed).standard_normal((n, c)).astype(dtype)
    for k, at in enumerate((0, L - 1, L, T - 1, T, TILE, CH - 1, CH)):
        if at < n:
            x[at, k % c] = (-0.0, 0.0)[k % 2]
    return np.asfortranarray(x)


def sig(n, c, seed=0, dtype=np.float64):
    return so.Signal(data(n, c, seed, dtype), FS)


def row(n, c, lo, hi, seed=0):
    return so.Signal(np.asfortranarray(np.random.default_rng(3000 * n + c + seed).uniform(lo, hi, (n, c))), FS)


def reson(n, c=1, seed=0):
    """`Recur2`'s two coefficient rows: n frames of stable resonator pairs (tests/recur2_ref.py `coef`)"""
    return tuple(so.Signal(a, FS) for a in coef("reson", n, c, seed))


def positions(ntable, n, c=1, seed=0):
    p = np.random.default_rng(77 * n + c + seed).uniform(-2.0, ntable + 1.0, (n, c))
    p[:min(n, 4), 0] = (0.0, ntable - 1.0, -0.0, ntable - 0.5)[:min(n, 4)]
    return so.Signal(np.asfortranarray(p), FS)


# one way to build each node over a finite Float64 or Float32 signal x: (name, constructor)
NODES = [
    ("SampleAt", lambda x: so.SampleAt(x, positions(S.nframes(x), S.nframes(x) + 3), left=-1.5, right=2.0)),
    ("Comb", lambda x: so.Comb(x, DELAYS[4], 0.7, feedforward=-0.35)),
    ("Allpass", lambda x: so.Allpass(x, DELAYS[-1], 0.6)),
    ("Cumsum", lambda x: so.Cumsum(x)),
    ("MovingMax", lambda x: so.MovingMax(x, 33, center=True)),
    ("MovingMin", lambda x: so.MovingMin(x, B + 2, ahead=B // 2)),           # the three-launch form
    ("MovingSum", lambda x: so.MovingSum(x, 480)),
    ("MovingMean", lambda x: so.MovingMean(x, 2 * TILE + 1, center=True)),   # long: whole segments in the middle
    ("MovingRMS", lambda x: so.MovingRMS(x, 17, ahead=16)),
    ("Recur", lambda x: so.Recur(row(S.nframes(x), 1, -1.0, 1.0), x)),
    ("PeakDecay", lambda x: so.PeakDecay(x, r=0.999)),
    ("Recur2", lambda x: so.Recur2(1.8, -0.9, x)),
    ("Recur2-rows", lambda x: so.Recur2(*reson(S.nframes(x)), x)),           # three inputs: a1 and a2 mono
    ("MovingMedian", lambda x: so.MovingMedian(x, 5, center=True)),
    ("MovingQuantile", lambda x: so.MovingQuantile(x, 257, 0.9, ahead=100)),
    ("SampleAt-cubic", lambda x: so.SampleAt(x, positions(S.nframes(x), S.nframes(x) + 3), left=-1.5, right=2.0, interp="cubic")),
    ("SampleAt-sinc", lambda x: so.SampleAt(x, positions(S.nframes(x), S.nframes(x) + 3), left=-1.5, right=2.0, interp="sinc")),
]
NAMES = [n for n, _ in NODES]
MAKE = dict(NODES)
SIX = ["SampleAt", "Comb", "Cumsum", "MovingMax", "MovingSum", "Recur"]
NINE = SIX + ["Recur2-rows", "MovingQuantile", "SampleAt-cubic"]


def check(tree, what):
    want = evaluate(tree)
    bit_equal(so.sink(tree, so.Array), want, what)
    return want


def no_alias(f):
    os.environ["SIGOPS_NO_WINDOW_ALIAS"] = "1"
    try:
        return f()
    finally:
        os.environ.pop("SIGOPS_NO_WINDOW_ALIAS", None)


def launches(tree, n, c, dtype=np.float64):
    """the launches of one execute of the tree into a planar device result (tests/test_gpu_window_alias.py test_fewer_launches)"""
    import torch

    out = torch.empty((c, n), dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")
    p = so.Plan(tree, (n, c), dtype, (1, n), True, device=0)
    p.execute(out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    k = p.stats()["n_launches"]
    p.close()
    return k, out.t().cpu().numpy()


def every_result_form(tree, what):
    """the five result forms of case (a); -> (launches with aliasing, without)"""
    import torch

    want = evaluate(tree)
    n, c = want.shape
    assert want.dtype == np.float64
    planar = (("a planar host result", lambda: so.sink(tree, so.Array)),
              ("a planar device result", lambda: so.sink(tree, "torch")[0].cpu().numpy()),
              ("a device result whose rows start 8 bytes off a 16-byte boundary",
               lambda: so.sink_into(torch.full((c, n + 1), 7.0, dtype=torch.float64, device="cuda")[:, 1:].t(), tree).cpu().numpy()))
    for name, run in planar:
        got = run()
        bit_equal(got, want, f"{what}: {name}")
        bit_equal(no_alias(run), got, f"{what}: {name}, without window aliasing")
    res32 = np.zeros((n, c), dtype=np.float32, order="F")
    so.sink_into(res32, tree)
    bit_equal(res32, np.asfortranarray(want.astype(np.float32)), f"{what}: a Float32 result")
    inter = np.zeros((n, c))  # C order: frame stride = channels
    so.sink_into(inter, tree)
    bit_equal(inter, np.ascontiguousarray(want), f"{what}: an interleaved host result")
    (k_alias, got), (k_plain, ref) = launches(tree, n, c), no_alias(lambda: launches(tree, n, c))
    bit_equal(got, np.ascontiguousarray(want), f"{what}: the plan whose launches are counted")
    bit_equal(ref, got, f"{what}: the same plan without window aliasing")
    print(f"{what}: n_launches {k_alias} with window aliasing, {k_plain} without")
    assert k_alias < k_plain, f"{what}: {k_alias} launches with window aliasing, {k_plain} without: nothing was aliased"
    return k_alias, k_plain


def six_family_append(c):
    """one child per family, odd and even lengths: the windows start at 1028 (the `SampleAt` has the length of its positions,
    three frames more than its table), 3077, 20488, 24661 and 25684"""
    lens = (T + 1, TILE + 1, CH + T + 3, 2 * TILE + 77, T - 1, CH + 1)
    return so.Append(*[MAKE[name](sig(n, c, k)) for k, (name, n) in enumerate(zip(SIX, lens))])


def nine_family_append(c):
    """one child per family of tests/tree_ref.py `FAMILIES`.  The first child has an odd length and every other an even one, so
    every window after the first starts at an odd frame, 8 bytes off a 16-byte boundary in a Float64 result: 1025, 3073, 4097,
    8271, 9295, 10321, 27731, 31905 (a `SampleAt` has the length of its positions, three frames more than its table).  The
    result has 48293 frames, an odd count: in a device result of two or three channels the rows alternate in alignment"""
    lens = (T - 2, TILE, T, 2 * TILE + 78, T, T + 2, CH + T + 2, 2 * TILE + 78, CH + 1)
    kids = [MAKE[name](sig(n, c, k)) for k, (name, n) in enumerate(zip(NINE, lens))]
    at = np.cumsum([S.nframes(k) for k in kids])
    assert list(at[:-1]) == [1025, 3073, 4097, 8271, 9295, 10321, 27731, 31905] and at[-1] == 48293
    return so.Append(*kids)


def float32_result_forms(tree, what):
    """a tree of Float32 nodes into a planar Float32 host result and a planar Float32 device result, each with and without
    window aliasing, and the launch count of both plans"""
    want = evaluate(tree)
    assert want.dtype == np.float32
    n, c = want.shape
    run = lambda: so.sink(tree, so.Array)  # noqa: E731
    got = run()
    bit_equal(got, want, f"{what}: a Float32 host result")
    bit_equal(no_alias(run), got, f"{what}: a Float32 host result, without window aliasing")
    (k_alias, dev), (k_plain, ref) = launches(tree, n, c, np.float32), no_alias(lambda: launches(tree, n, c, np.float32))
    bit_equal(dev, np.ascontiguousarray(want), f"{what}: a Float32 device result")
    bit_equal(ref, dev, f"{what}: a Float32 device result, without window aliasing")
    print(f"{what}: n_launches {k_alias} with window aliasing, {k_plain} without")
    assert k_alias < k_plain, f"{what}: {k_alias} launches with window aliasing, {k_plain} without: nothing was aliased"


def four_float32_windows(makers, c):
    """a root `Append` of four Float32 nodes of T + 1, TILE + 1, L + 1 and CH + T + 3 frames: the second, third and fourth
    windows start at frames 1025, 3074 and 3091, which in a Float32 result are 4, 8 and 12 bytes off a 16-byte boundary"""
    lens = (T + 1, TILE + 1, L + 1, CH + T + 3)
    assert [(4 * k) % 16 for k in np.cumsum(lens)[:3]] == [4, 8, 12]
    return so.Append(*[make(sig(n, c, k, np.float32)) for k, (make, n) in enumerate(zip(makers, lens))])


# ---- (a) a root Append whose children are nodes: window aliasing ----------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_a_root_append_of_two_nodes_in_every_result_form(name):
    for c in (1, 2, 3):
        tree = so.Append(MAKE[name](sig(T + 1, c)), MAKE[name](sig(CH + T + 3, c, 1)))
        every_result_form(tree, f"Append({name}, {name}) C={c}")


@pytest.mark.parametrize("c", [1, 2, 3])
def test_a_root_append_of_six_families_in_every_result_form(c):
    every_result_form(six_family_append(c), f"Append of six families C={c}")


def test_a_root_append_of_float32_extrema_into_a_float32_result():
    for c in (1, 2, 3):
        tree = so.Append(so.MovingMax(sig(T + 1, c, 0, np.float32), 33, center=True), so.MovingMin(sig(CH + T + 3, c, 1, np.float32), B + 2, ahead=5))
        want = evaluate(tree)
        assert want.dtype == np.float32
        run = lambda: so.sink(tree, so.Array)  # noqa: E731
        got = run()
        bit_equal(got, want, f"Float32 extrema C={c}")
        bit_equal(no_alias(run), got, f"Float32 extrema C={c}, without window aliasing")
        n = want.shape[0]
        (k_alias, dev), (k_plain, _) = launches(tree, n, c, np.float32), no_alias(lambda: launches(tree, n, c, np.float32))
        bit_equal(dev, np.ascontiguousarray(want), f"Float32 extrema C={c}, a device result")
        print(f"Float32 extrema C={c}: n_launches {k_alias} with window aliasing, {k_plain} without")
        assert k_alias < k_plain


@pytest.mark.parametrize("c", [1, 2, 3])
def test_a_root_append_of_nine_families_in_every_result_form(c):
    every_result_form(nine_family_append(c), f"Append of nine families C={c}")


RANKS32 = (lambda x: so.MovingMedian(x, 5, center=True), lambda x: so.MovingQuantile(x, 257, 0.9, ahead=100),
           lambda x: so.MovingQuantile(x, 33, 0.1), lambda x: so.MovingMedian(x, 1025, center=True))
EXTREMA32 = (lambda x: so.MovingMax(x, 33, center=True), lambda x: so.MovingMin(x, B + 2, ahead=5),
             lambda x: so.MovingMin(x, 3, ahead=2), lambda x: so.MovingMax(x, 2 * TILE + 1, center=True))


@pytest.mark.parametrize("c", [1, 2, 3])
def test_float32_moving_ranks_at_every_4_byte_phase_of_a_float32_result(c):
    """k_movrank stores four Float32 at a time where the destination allows (`vy`), one at a time where it does not: windows
    4, 8 and 12 bytes off a 16-byte boundary; the 17 frames of the third child are shorter than its window of 257"""
    float32_result_forms(four_float32_windows(RANKS32, c), f"four Float32 moving ranks C={c}")


@pytest.mark.parametrize("c", [1, 2, 3])
def test_float32_extrema_at_every_4_byte_phase_of_a_float32_result(c):
    float32_result_forms(four_float32_windows(EXTREMA32, c), f"four Float32 extrema C={c}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_largest_rank_window_at_an_odd_offset(dtype):
    """1025 frames, the longest window that is built, behind an array of T + 1 frames: the rank stage writes its window of the
    result from frame 1025 on.  Short inputs: the definition sorts every window"""
    for c in (1, 3):
        for name, make in (("MovingQuantile(1025, 0.25, ahead=900)", lambda x: so.MovingQuantile(x, 1025, 0.25, ahead=900)),
                           ("MovingMedian(1025, center)", lambda x: so.MovingMedian(x, 1025, center=True))):
            tree = so.Append(sig(T + 1, c, 0, dtype), make(sig(TILE + 77, c, 1, dtype)))
            what = f"Append(array, {name}) {np.dtype(dtype).name} C={c}"
            want = check(tree, what)
            bit_equal(no_alias(lambda: so.sink(tree, so.Array)), want, what + ", without window aliasing")
            n = want.shape[0]
            (k_alias, dev), (k_plain, ref) = launches(tree, n, c, dtype), no_alias(lambda: launches(tree, n, c, dtype))
            bit_equal(dev, np.ascontiguousarray(want), what + ": a device result")
            bit_equal(ref, dev, what + ": a device result, without window aliasing")
            print(f"{what}: n_launches {k_alias} with window aliasing, {k_plain} without")


def test_both_sinc_forms_at_an_odd_offset():
    """the `SampleAt` entries of `NODES` have even lengths (their table's and three frames more), so the second window of
    their root `Append` is aligned.  Here the sinc window starts at frame 1025 and the result has an odd number of frames, so
    the rows of a device result alternate in alignment and the pairs shift by one frame in every other row: 2 x 65538 frames
    of positions reach the form that keeps the tap table in LDS (131072 frames x channels and more), and 64 taps are more
    than that form takes"""
    for name, n, kw in (("16 taps in LDS", 4 * CH + 2, {}), ("64 taps", TILE + 2, {"taps": 64}), ("10 taps, cutoff 0.5, wrap", TILE + 2, {"taps": 10, "cutoff": 0.5, "wrap": True})):
        tree = so.Append(so.Cumsum(sig(T + 1, 2)), so.SampleAt(sig(4097, 2, 1), positions(4097, n, 2), left=-1.5, right=2.0, interp="sinc", **kw))
        assert S.nframes(tree) % 2 == 1
        every_result_form(tree, f"Append(Cumsum, SampleAt sinc, {name}) C=2")


def test_old_and_new_stages_aliased_in_one_result():
    """a filter, a `Cumsum` and a resampler under one `Append`: the `Cumsum` window bit for bit, the other two within the
    project's Float64 bound, 1e-8 norm-wise, of the same children sunk alone"""
    for c in (1, 2):
        x, y, z = data(5001, c), data(CH + T + 3, c, 1), data(4001, c, 2)
        kids = (so.Signal(x, FS) | so.Filt(so.Lowpass, 1 * so.kHz), so.Cumsum(so.Signal(y, FS)), so.Signal(z, 8 * so.kHz) | so.ToFramerate(FS))
        tree = so.Append(*kids)
        alone = [so.sink(k, so.Array) for k in kids]
        run = lambda: so.sink(tree, so.Array)  # noqa: E731
        got = run()
        bit_equal(no_alias(run), got, "without window aliasing")
        at = np.cumsum([0] + [a.shape[0] for a in alone])
        assert got.shape == (at[-1], c) and at[1] % 2 == 1
        bit_equal(np.asfortranarray(got[at[1]:at[2]]), cumsum_ref(y), "the Cumsum window")
        for k, name in ((0, "Filt"), (2, "ToFramerate")):
            e = relerr(got[at[k]:at[k + 1]], alone[k])
            print(f"{name} window against the child sunk alone: {e:.3e}")
            assert np.ptp(alone[k]) > 0.1 and e <= 1e-8, f"{name}: {e:.3e}"
        k_alias, k_plain = launches(tree, at[-1], c)[0], no_alias(lambda: launches(tree, at[-1], c))[0]
        print(f"Filt, Cumsum, ToFramerate C={c}: n_launches {k_alias} with window aliasing, {k_plain} without")
        assert k_alias < k_plain


def test_an_aliased_plan_is_executed_again_and_after_set_array():
    import torch

    c = 2
    tree = six_family_append(c)
    want = evaluate(tree)
    n = want.shape[0]
    res = np.zeros((n, c), order="F")
    p = so.Plan(tree, (n, c), np.float64, (1, n), False)
    for k in range(3):
        res[:] = np.nan
        p.execute(res.ctypes.data)
        bit_equal(res, want, f"a host result, execute {k}")
    first = p.lowered.array_nodes[0][1]  # an array leaf of the SampleAt child
    new = np.asfortranarray(first.data[::-1])
    p.set_array(0, new)
    p.execute(res.ctypes.data)
    p.close()
    first.data = new
    bit_equal(res, evaluate(tree), "a host result after set_array")
    p = so.Plan(tree, (n, c), np.float64, (1, n + 1), True)
    for k in range(3):
        out = torch.full((c, n + 1), np.nan, dtype=torch.float64, device="cuda")
        p.execute(out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        p.check()
        bit_equal(out[:, :n].t().cpu().numpy(), np.ascontiguousarray(evaluate(tree)), f"a device result, execute {k}")
    p.close()


# ---- (b) structural operators behind a node --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_structural_operators_behind_a_node(name):
    make = MAKE[name]
    for n, c in ((T + 1, 2), (CH + T + 3, 1)):
        node = make(sig(n, c))
        N = S.nframes(node)
        for p in (so.lastframe, so.zero, 2.5):
            for k in (1, N + 3):
                check(so.Pad(node, p) | so.Until((N + k) * fr), f"Pad({name}, {getattr(p, '__name__', p)}) | Until(n + {k}) n={n} C={c}")
        for p in (so.cycle, so.mirror):  # refused by design: an indexing pad reads an array leaf
            with pytest.raises(so.ErrorException, match="indexing pad function"):
                so.sink(so.Pad(node, p) | so.Until((N + 1) * fr), so.Array)
    mono = make(sig(CH + 1, 1, 2))
    N = S.nframes(mono)
    check(so.ToChannels(mono, 3), f"ToChannels({name}, 3)")
    check(so.Mix(mono, sig(N - T - 1, 2, 3)), f"Mix({name} mono, a shorter stereo array)")
    check(so.Mix(sig(N + L + 1, 2, 3), mono), f"Mix(a longer stereo array, {name} mono)")
    check(so.Mix(make(sig(T + 1, 2, 4)), make(sig(CH + T + 3, 2, 5))), f"Mix({name}, {name}) of unequal lengths")
    check(so.Amplify(make(sig(TILE + 1, 3, 6)), sig(TILE - L - 1, 3, 7)), f"Amplify({name}, a shorter array)")


# ---- (c) structural operators under a node ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_structural_operators_under_a_node(name):
    make = MAKE[name]
    for c in (1, 3):
        check(make(so.Append(sig(T + 1, c), sig(CH + 3, c, 1))), f"{name}(Append) C={c}")
        check(make(so.Append(sig(L + 1, c, 0, np.float32), sig(TILE + 1, c, 1, np.float32))), f"{name}(Append of Float32) C={c}")
        check(make(so.Pad(sig(T + 1, c, 2), so.mirror) | so.Until((2 * T + L + 3) * fr)), f"{name}(Pad(mirror) | Until) C={c}")
        check(make(so.Pad(sig(TILE - 1, c, 2), so.cycle) | so.After(3 * fr) | so.Until((TILE + T + 1) * fr)), f"{name}(Pad(cycle) | After | Until) C={c}")
        check(make(so.Pad(sig(T + 1, c, 2), so.lastframe) | so.Until((T + L + 2) * fr)), f"{name}(Pad(lastframe) | Until) C={c}")
        check(make(so.Mix(sig(T + 1, c, 3), sig(CH + 3, c, 4))), f"{name}(Mix) of unequal lengths C={c}")
        check(make(so.Amplify(sig(TILE + 1, c, 3), sig(T - 1, 1, 4))), f"{name}(Amplify) of unequal lengths, one mono C={c}")
    check(make(so.ToChannels(sig(CH + 1, 1, 5), 2)), f"{name}(ToChannels(mono, 2))")


def test_second_inputs_of_several_pieces():
    for c in (1, 2):
        b = so.Pad(sig(T + 1, c), so.lastframe) | so.Until((CH + 3) * fr)
        a = so.Append(row(T - 1, 1, 0.0, 1.0), row(CH, 1, 0.9, 1.0, 1), row(5, 1, 0.0, 1.0, 2))
        check(so.Recur(a, b), f"Recur(a = Append, b = Pad | Until) C={c}")
        check(so.PeakDecay(b, r=so.Append(row(CH + 1, c, 0.0, 1.0), row(L + 1, c, 0.99, 1.0, 1))), f"PeakDecay(r = Append of {c} channels, b = Pad | Until)")
        n, npos = T + 1 + CH + 3, CH + T + 3
        ramp = so.Signal(np.asfortranarray(np.linspace(-1.0, n, npos).reshape(-1, 1)), FS)
        small = so.Signal(np.asfortranarray(np.random.default_rng(5 + c).uniform(-2.0, 2.0, (npos - T - 1, c))), FS)
        check(so.SampleAt(so.Append(sig(T + 1, c, 1), sig(CH + 3, c, 2)), so.Mix(ramp, small), left=-1.0, right=3.0),
              f"SampleAt(table = Append, pos = Mix(ramp, a small array)) C={c}")


def test_a_seam_inside_one_window_and_a_delay_longer_than_the_first_child():
    for c in (1, 3):
        for w in (33, B + 2):
            x = so.Append(sig(T + 5, c), sig(TILE + 1, c, 1))  # the seam at T + 5 lies inside the windows of the frames around it
            check(so.MovingMax(x, w, center=True), f"MovingMax over a seam, w={w} C={c}")
            check(so.MovingSum(x, w, center=True), f"MovingSum over a seam, w={w} C={c}")
        for D in (DELAYS[6], DELAYS[-1]):
            x = so.Append(sig(D - 3, c), sig(CH + 1, c, 1))
            check(so.Comb(x, D, 0.7), f"Comb, D={D} longer than the first child C={c}")
            check(so.Allpass(x, D, -0.6), f"Allpass, D={D} longer than the first child C={c}")


def test_a_seam_inside_one_rank_window():
    for c in (1, 3):
        for dtype in (np.float64, np.float32):
            x = so.Append(sig(T + 5, c, 0, dtype), sig(TILE + 1, c, 1, dtype))  # the seam at T + 5 lies inside the windows around it
            for w in (33, 1025):
                check(so.MovingMedian(x, w, center=True), f"MovingMedian over a seam, w={w} {np.dtype(dtype).name} C={c}")


def test_the_three_inputs_of_a_recur2_of_several_pieces():
    """`Recur2` reads a1 and a2 through `Stage::side[0]` and `side[1]`: each of the three inputs of several pieces"""
    for c in (1, 2, 3):
        n = CH + 3
        u1, u2 = coef("u1h", n + L, 1, c)
        a1 = so.Append(so.Signal(u1[:T - 1], FS), so.Signal(u1[T - 1:CH], FS), so.Signal(u1[CH:], FS))  # longer than b
        a2 = so.Pad(so.Signal(u2[:T + 1], FS), 0.25) | so.Until(n * fr)
        b = so.Mix(sig(T + 1, c), sig(n, c, 1))
        want = check(so.Recur2(a1, a2, b), f"Recur2(a1 = Append, a2 = Pad | Until, b = Mix of unequal lengths) C={c}")
        assert np.isfinite(want).all() and np.ptp(want) > 0.1
        r1, r2 = coef("reson", n, c, c)
        a1 = so.Append(so.Signal(r1[:CH + 1], FS), so.Signal(r1[CH + 1:], FS))
        a2 = so.Append(so.Signal(r2[:L + 1], FS), so.Signal(r2[L + 1:], FS))
        b = so.Pad(sig(T + 1, c), so.lastframe) | so.Until(n * fr)
        want = check(so.Recur2(a1, a2, b), f"Recur2(a1, a2 = Append of {c} channels, b = Pad | Until)")
        assert np.isfinite(want).all() and np.ptp(want) > 0.1


def test_one_node_read_as_two_inputs_of_its_parent():
    for c in (1, 2):
        x = np.abs(data(CH + T + 3, c)) + 1e-3
        n = so.Cumsum(so.Signal(np.asfortranarray(x / x.sum(axis=0)), FS))  # rises from 0 to 1
        want = check(so.Recur2(so.Amplify(n, 0.999), -0.25, n), f"Recur2(a1 = 0.999 n, a2 = -0.25, b = n), n a Cumsum C={c}")
        assert np.isfinite(want).all()
        for name in ("MovingMedian", "Recur2", "Cumsum"):
            t = MAKE[name](sig(CH + 1, c, 1))
            pos = positions(CH + 1, CH + T + 3, c)
            check(so.Mix(so.SampleAt(t, pos, left=-1.5, right=2.0, interp="cubic"), t), f"Mix(SampleAt cubic(table = t, pos), t), t a {name} C={c}")
            check(so.Mix(so.SampleAt(t, pos, wrap=True, interp="sinc", taps=10, cutoff=0.5), t | so.After(T * fr)), f"Mix(SampleAt sinc(table = t, pos), t | After), t a {name} C={c}")


# ---- (d) one node, several readers -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_one_node_read_by_several_parents(name):
    for c, pairs in ((2, ((L, T + 1), (T - 1, TILE), (TILE + 1, L - 1))), (1, ((T, L + 1), (TILE, T - 1), (L + 1, TILE + 1)))):
        n = MAKE[name](sig(CH + T + 3, c))
        for k, j in pairs:
            check(so.Append(n | so.After(k * fr), n | so.Until(j * fr)), f"Append({name} | After({k}), {name} | Until({j})) C={c}")
            check(so.Mix(n, n | so.After(k * fr)), f"Mix({name}, {name} | After({k})) C={c}")
        check(so.Append(n | so.Until(100 * fr), n | so.After(5000 * fr) | so.Until(100 * fr)), f"{name}: two readers far apart C={c}")
        check(so.Amplify(n | so.After((CH + 1) * fr), n | so.Until(T * fr)), f"{name}: Amplify of its end and its start C={c}")


def test_a_cumsum_as_both_inputs_of_a_recur():
    for c in (1, 2):
        x = np.abs(data(CH + T + 3, c)) + 1e-3
        n = so.Cumsum(so.Signal(np.asfortranarray(x / x.sum(axis=0)), FS))  # rises from 0 to 1
        check(so.Recur(so.Amplify(n, 0.999), n), f"Recur(a = 0.999 n, b = n), n a Cumsum C={c}")
        check(so.PeakDecay(n, r=so.Mix(so.Amplify(n, -0.5), 1.0)), f"PeakDecay(r = 1 - n / 2, b = n), n a Cumsum C={c}")


# ---- (e) windows and blocks of composite trees -------------------------------------------------------------------------------
def _composite(which):
    if which == "six families under Append":
        return six_family_append(2)
    if which == "Pad behind Cumsum":
        n = CH + T + 3
        return so.Pad(so.Cumsum(sig(n, 2)), so.lastframe) | so.Until((2 * n + 3) * fr)
    if which == "Comb over Append":
        return so.Comb(so.Append(sig(CH + 1, 1), sig(CH + T + 77, 1, 1)), DELAYS[-1], 0.7)
    if which == "MovingSum over Mix":
        return so.MovingMean(so.Mix(sig(CH + 1, 3), sig(2 * CH + T + 77, 1, 1)), B + 2, center=True)
    if which == "nine families under Append":
        return nine_family_append(2)
    if which == "MovingMedian over Mix":
        return so.MovingMedian(so.Mix(sig(CH + 1, 3), sig(2 * CH + T + 77, 1, 1)), 257, center=True)
    n = so.Recur(row(CH + 2 * T, 1, -1.0, 1.0), sig(CH + 2 * T, 2))
    return so.Append(n | so.After(T * fr), n | so.Until((CH + T + 3) * fr))


@pytest.mark.parametrize("which", ["six families under Append", "Pad behind Cumsum", "Comb over Append", "MovingSum over Mix", "Recur read twice",
                                   "nine families under Append", "MovingMedian over Mix"])
def test_windows_and_blocks_of_composite_trees(which):
    """the (s, m) pairs of tests/test_gpu_recur.py test_windows_and_streams_equal_the_whole_sink: (T - 1, CH) and (CH + 5,
    CH + T + 2) straddle the seams of every tree here (an `Append`'s, a `Pad`'s start, the end of `Mix`'s shorter operand)"""
    tree = _composite(which)
    whole = check(tree, which)
    N = whole.shape[0]
    assert 2 * CH + T + 7 <= N <= 3 * CH + 77
    for s, m in ((1, 5), (L + 3, 2 * T + 1), (T - 1, CH), (CH + 5, CH + T + 2)):
        got = so.sink(tree | so.After(s * fr) | so.Until(m * fr), so.Array)
        bit_equal(got, np.asfortranarray(whole[s:s + m]), f"{which}: After({s}) | Until({m})")
    bit_equal(so.sink(tree | so.Until((CH + 3) * fr), so.Array), np.asfortranarray(whole[:CH + 3]), f"{which}: Until")
    bit_equal(so.sink(tree | so.After((CH + T + 1) * fr), so.Array), np.asfortranarray(whole[CH + T + 1:]), f"{which}: After")
    for bs in (7000, 16385):
        blocks = np.vstack([np.asarray(blk) for blk in so.stream(tree, bs, so.Array)])
        bit_equal(np.asfortranarray(blocks), whole, f"{which}: blocks of {bs}")


# ---- random trees ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS + SEEDS_ALL)
def test_random_node_trees(seed):
    """every tree of the seed: the whole sink, one random window and one `stream` with an odd block size, bit for bit.  No
    tree is skipped and no refusal is caught: the generator (tests/tree_ref.py) leaves out what is refused by design.  The
    trees of `SEEDS` hold the six families the generator began with, those of `SEEDS_ALL` all nine"""
    rng = np.random.default_rng(1000 + seed)
    for i, (nch, tree) in enumerate(random_trees(seed)):
        what = f"seed {seed}, tree {i}"
        whole = check(tree, what)
        N = whole.shape[0]
        s = int(rng.integers(0, N))
        m = int(rng.integers(1, N - s + 1))
        win = tree | so.Until(m * fr) if s == 0 else tree | so.After(s * fr) | so.Until(m * fr)
        bit_equal(so.sink(win, so.Array), np.asfortranarray(whole[s:s + m]), f"{what}: After({s}) | Until({m})")
        bs = (N // int(rng.integers(1, 4)) + 1) | 1  # odd: up to four blocks
        blocks = np.vstack([np.asarray(blk) for blk in so.stream(tree, bs, so.Array)])
        bit_equal(np.asfortranarray(blocks), whole, f"{what}: blocks of {bs}")
