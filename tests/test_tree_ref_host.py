"""The composite-tree evaluator (tests/tree_ref.py) without a GPU: its structural part -- `Until`, `After`, every pad kind,
`Append`, `ToChannels`, `Mix` and `Amplify` with signals of unequal length, numbers and mono broadcast -- equals the CPU
oracle bit for bit on seeded random trees, and the random trees tests/test_gpu_node_trees.py runs are finite, hold every
family of device-only node and every placement the planner treats on its own.  No rule had to leave the grammar: the
oracle agrees on all of them.  The trees of the first five seeds are pinned by digest (tests/golden/tree_seeds.json), and
the branches of `Recur2`, the moving ranks and the cubic and sinc `SampleAt` are held to direct calls of their definitions."""
import json
import os
from collections import Counter

import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import signals as S
from oracle_bridge import oracle_sink
from cumsum_ref import L, T
from moving_ref import same_bits
from movingmedian_ref import movrank_ref
from recur2_ref import coef, recur2_ref
from sampleat_interp_ref import sampleat_interp
from sampleat_ref import sampleat_np
from tree_ref import FAMILIES, FS, SEEDS, SEEDS_ALL, SIX, census, digest, evaluate, placed, random_trees, walk

PLACEMENTS = ("under_root_append", "over_append_or_pad", "pad_behind_node", "two_readers")
NEW = ("Recur2", "MovingRank", "SampleAtFir")  # the families that joined the grammar after the first six


def bit_equal(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} samples differ, first at {np.argwhere(bad)[0]}"
    assert same_bits(got, want), f"{what}: a zero of the other sign"


def sig(n, c, dtype=np.float64, seed=0):
    x = np.random.default_rng(100 * n + c + seed).standard_normal((n, c)).astype(dtype)
    x[n // 2, 0] = -0.0
    return so.Signal(np.asfortranarray(x), FS)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_every_pad_kind_equals_the_oracle(dtype):
    for n in (1, 2, 7):
        for c in (1, 3):
            x = sig(n, c, dtype)
            for p in (so.zero, so.one, 2.5, -0.0, so.lastframe, so.cycle, so.mirror):
                for k in (1, n, n + 3, 4 * n + 1):
                    tree = so.Pad(x, p) | so.Until((n + k) * so.frames)
                    bit_equal(evaluate(tree), oracle_sink(tree), f"Pad({p}) n={n} k={k}")
                    tree = so.Pad(x, p) | so.After((n + 1) * so.frames) | so.Until(k * so.frames)
                    bit_equal(evaluate(tree), oracle_sink(tree), f"Pad({p}) | After n={n} k={k}")
            tree = so.Pad(so.Append(x, sig(3, c, dtype, 1)) | so.After(1 * so.frames), so.lastframe) | so.Until((n + 9) * so.frames)
            bit_equal(evaluate(tree), oracle_sink(tree), "lastframe behind Append | After")


def test_mix_and_amplify_of_unequal_lengths_numbers_and_mono_equal_the_oracle():
    a, b, m = sig(9, 2), sig(5, 2, seed=1), sig(7, 1, seed=2)
    b.data[4, 1] = -0.0  # under the longer operand's frames: -0.0 + 0.0 = +0.0, -0.0 * 1.0 = -0.0
    for op in (so.Mix, so.Amplify):
        for tree in (op(a, b), op(b, a), op(a, m), op(m, b), op(a, 2.5), op(a, -0.0), op(m, 0.5), op(op(a, b), m),
                     op(b | so.After(2 * so.frames), a | so.Until(4 * so.frames)), op(so.ToChannels(m, 2), 1.0),
                     so.Append(op(m, m | so.After(3 * so.frames)), m)):
            got = evaluate(tree)
            bit_equal(got, oracle_sink(tree), op.__name__)
            assert got.shape == (S.nframes(tree), tree.nch)
    z = so.Signal(np.full((4, 1), -0.0), FS)
    got = evaluate(so.Mix(z, z | so.Until(2 * so.frames)))  # the shorter operand is extended with +0.0 and the sum is taken there too
    assert np.signbit(got[:2]).all() and not np.signbit(got[2:]).any()
    assert np.signbit(evaluate(so.Amplify(z, z | so.Until(2 * so.frames)))[2:]).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_random_structural_trees_equal_the_oracle(seed):
    pads, maps, mono, unequal = Counter(), Counter(), 0, 0
    for nch, tree in random_trees(seed, 40, nodes=False):
        want = oracle_sink(tree)
        got = evaluate(tree)
        assert got.shape == (S.nframes(tree), nch)
        bit_equal(got, want, f"seed {seed}")
        for x, _ in walk(tree):
            if isinstance(x, S.PaddedSignal):
                pads["number" if isinstance(x.pad, float) else x.pad.__name__] += 1
            if isinstance(x, S.MapSignal):
                maps[x.fn] += 1
                mono += x.fn == S.ASNCHANNELS
                unequal += x.fn in (S.ADD, S.MUL) and len({S.nframes(c) for c in x.signals if not isinstance(c, S.NumberSig)}) > 1
    assert set(pads) == {"zero", "one", "number", "lastframe", "cycle", "mirror"}, pads
    assert maps[S.ADD] and maps[S.MUL] and mono and unequal >= 5, (maps, mono, unequal)


def test_the_gpu_seeds_are_finite_and_cover_every_family_and_placement():
    fams, places = Counter(), Counter()
    for seed in SEEDS:
        for nch, tree in random_trees(seed):
            f, p = census(tree)
            assert f, "a tree without a device-only node"
            fams.update(f)
            places.update(p)
            for x, _ in walk(tree):  # no Float32 arithmetic: it is outside the grammar
                if isinstance(x, S.MapSignal) and x.fn in (S.ADD, S.MUL):
                    assert all(c.dtype == S.F64 for c in x.signals), "arithmetic on a Float32 signal"
            got = evaluate(tree)
            assert got.shape == (S.nframes(tree), nch) and got.shape[0] >= 1
            assert np.isfinite(got).all(), f"seed {seed}: a value that is not finite"
    print(dict(fams), dict(places))
    assert set(fams) == {"SampleAt", "Comb", "Cumsum", "Moving", "MovingSum", "Recur"}, fams
    assert all(places[p] >= 5 for p in PLACEMENTS), places


def test_the_seeds_of_all_families_are_finite_and_cover_every_family_placement_and_kind():
    """the same conditions on the trees of `SEEDS_ALL`, and for the three families that joined the grammar last: each in at
    least five trees and in every placement, a Float32 moving rank, `Recur2` with rows and with constants, every `interp`"""
    fams, places, where = Counter(), Counter(), Counter()
    f32_ranks, long_ranks, rows, constants, interps = 0, 0, 0, 0, Counter()
    for seed in SEEDS_ALL:
        for nch, tree in random_trees(seed):
            f, p = census(tree)
            assert f, "a tree without a device-only node"
            fams.update(f)
            places.update(p)
            where.update(placed(tree))
            for x, _ in walk(tree):
                if isinstance(x, S.MapSignal) and x.fn in (S.ADD, S.MUL):
                    assert all(c.dtype == S.F64 for c in x.signals), "arithmetic on a Float32 signal"
                if isinstance(x, S.MovingRankSignal):
                    f32_ranks += x.dtype == S.F32
                    long_ranks += x.back + x.ahead + 1 > 257
                if isinstance(x, S.Recur2Signal):
                    rows += x.coefs is not None
                    constants += x.coefs is None
                    assert x.coefs is None or all(isinstance(c, S.AbstractSignal) for c in x.coefs)
                if isinstance(x, S.SampleAtSignal):
                    interps[(x.interp, x.taps, x.cutoff)] += 1
            got = evaluate(tree)  # (a refusal of the evaluator is an AssertionError: none is caught)
            assert got.shape == (S.nframes(tree), nch) and got.shape[0] >= 1
            assert np.isfinite(got).all(), f"seed {seed}: a value that is not finite"
    print("trees that hold the family:", dict(fams))
    print("trees that hold the placement:", dict(places))
    print("trees that hold (family, placement):", {f"{f} {p}": where[f, p] for f in NEW for p in PLACEMENTS})
    print(f"Float32 moving ranks {f32_ranks}, windows above 257 frames {long_ranks}, Recur2 with rows {rows}, with constants {constants}")
    print("SampleAt kinds (interp, taps, cutoff):", dict(interps))
    assert set(fams) == set(FAMILIES) and len(FAMILIES) == 9, fams
    assert all(places[p] >= 5 for p in PLACEMENTS), places
    assert all(fams[f] >= 5 for f in NEW), fams
    assert all(where[f, p] >= 1 for f in NEW for p in PLACEMENTS), where
    assert f32_ranks >= 1 and long_ranks >= 1 and rows >= 1 and constants >= 1
    assert set(interps) == {("linear", 0, 0.0), ("cubic", 0, 0.0), ("sinc", 16, 1.0), ("sinc", 4, 1.0), ("sinc", 64, 1.0), ("sinc", 10, 0.5)}, interps


def test_the_trees_of_the_first_seeds_have_not_moved():
    """sha256 over sample type, shape and bytes of `evaluate(tree)` for the 100 trees of `SEEDS`, recorded before the
    generator learnt the other three families: a families argument, a new draw or a new branch must leave them alone"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tree_seeds.json")) as f:
        pinned = json.load(f)
    assert sorted(pinned) == sorted(str(s) for s in SEEDS)
    for seed in SEEDS:
        got = [digest(evaluate(tree)) for _, tree in random_trees(seed)]
        assert len(got) == 20 and got == pinned[str(seed)], f"seed {seed}: trees {[i for i in range(20) if got[i] != pinned[str(seed)][i]]} moved"
        assert [digest(evaluate(tree)) for _, tree in random_trees(seed, families=SIX)] == got


# ---- the branches of the three families against direct calls of their definitions -----------------------------------------
def rows(n, c, seed=0):
    a1, a2 = coef("reson", n, c, seed)
    return a1, a2


def test_recur2_is_its_definition_over_the_evaluated_inputs():
    b = sig(T + 5, 3)
    bit_equal(evaluate(so.Recur2(1.8, -0.9, b)), recur2_ref(1.8, -0.9, b.data), "constants")
    a1, a2 = rows(T + 5, 3)
    bit_equal(evaluate(so.Recur2(so.Signal(a1, FS), so.Signal(a2, FS), b)), recur2_ref(a1, a2, b.data), "rows of 3 channels")
    # a mono coefficient `Append` longer than b, beside a row of b's channels; b itself a `Mix` of unequal lengths
    m1, _ = rows(T + 12, 1, 1)
    ca = so.Append(so.Signal(m1[:700], FS), so.Signal(m1[700:], FS))
    bb = so.Mix(b, sig(L + 1, 3, seed=1))
    want = recur2_ref(m1[:T + 5], a2, evaluate(bb))
    tree = so.Recur2(ca, so.Signal(a2, FS), bb)
    bit_equal(evaluate(tree), want, "a1 a mono Append longer than b")
    bit_equal(evaluate(tree | so.After(3 * so.frames) | so.Until(L * so.frames)), np.asfortranarray(want[3:3 + L]), "a window of it")
    assert not np.array_equal(want, recur2_ref(m1[7:T + 12], a2, evaluate(bb)))  # (the coefficient's first frames, not its last)


def test_a_moving_rank_is_its_definition_and_keeps_the_sample_type():
    for dtype in (np.float64, np.float32):
        x = sig(T + 5, 2, dtype)
        got = evaluate(so.MovingQuantile(x, 33, 0.9, ahead=7))
        assert got.dtype == dtype
        bit_equal(got, movrank_ref(x.data, 25, 7, 0.9), f"MovingQuantile {np.dtype(dtype).name}")
        bit_equal(evaluate(so.MovingMedian(so.Append(x, x), 5, center=True)), movrank_ref(np.concatenate([x.data, x.data]), 2, 2, 0.5), "over Append")
    # an infinite padded child under `Until`: frame n looks `ahead` frames into the pad, the window is clipped at the front only
    x = sig(66, 2)
    n, back, ahead = 70, 10, 6
    padded = np.concatenate([x.data, np.full((n + ahead - 66, 2), 2.5)])
    tree = so.MovingQuantile(so.Pad(x, 2.5), back + ahead + 1, 0.5, ahead=ahead) | so.Until(n * so.frames)
    bit_equal(evaluate(tree), movrank_ref(padded, back, ahead, 0.5)[:n], "an infinite padded child under Until")
    assert not np.array_equal(evaluate(tree), movrank_ref(padded[:n], back, ahead, 0.5))  # (not clipped at frame n)


def test_sampleat_cubic_and_sinc_are_their_definition():
    x, pos = sig(65, 2), so.Signal(np.asfortranarray(np.random.default_rng(5).uniform(-2.0, 67.0, (1001, 1))), FS)
    for kw in ({"interp": "cubic"}, {"interp": "sinc"}, {"interp": "sinc", "taps": 4}, {"interp": "sinc", "taps": 64}, {"interp": "sinc", "taps": 10, "cutoff": 0.5}):
        for wrap in (False, True):
            got = evaluate(so.SampleAt(x, pos, left=-1.5, right=2.0, wrap=wrap, **kw))
            want = sampleat_interp(x.data, pos.data, kw["interp"], -1.5, 2.0, False, wrap, taps=kw.get("taps", 16), cutoff=kw.get("cutoff", 1.0))
            bit_equal(got, want, f"{kw} wrap={wrap}")
    lin = evaluate(so.SampleAt(x, pos, left=-1.5, right=2.0))
    bit_equal(lin, sampleat_np(x.data, pos.data, -1.5, 2.0, False, False), "linear")
    assert not np.array_equal(lin, evaluate(so.SampleAt(x, pos, left=-1.5, right=2.0, interp="cubic")))
