"""The composite-tree evaluator (tests/tree_ref.py) without a GPU: its structural part -- `Until`, `After`, every pad kind,
`Append`, `ToChannels`, `Mix` and `Amplify` with signals of unequal length, numbers and mono broadcast -- equals the CPU
oracle bit for bit on seeded random trees, and the random trees tests/test_gpu_node_trees.py runs are finite, hold every
family of device-only node and every placement the planner treats on its own.  No rule had to leave the grammar: the
oracle agrees on all of them."""
from collections import Counter

import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import signals as S
from oracle_bridge import oracle_sink
from moving_ref import same_bits
from tree_ref import FAMILIES, FS, SEEDS, census, evaluate, random_trees, walk

PLACEMENTS = ("under_root_append", "over_append_or_pad", "pad_behind_node", "two_readers")


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
    assert set(fams) == set(FAMILIES), fams
    assert all(places[p] >= 5 for p in PLACEMENTS), places
