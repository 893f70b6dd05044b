"""Every device-only stage node (a subclass of `StageSignal`) through every place that treats them alike: the lowering,
`ToFramerate`, the demand analysis, `BlockStream`'s refusal and the three sharding refusals.  One tiny instance per class
and form, in one table; the table must cover every subclass, so a new node cannot be added without a row -- and a row
fails wherever the node was forgotten.  No GPU, no engine library: trees and node tables only."""
import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import _capi as K
from sigops_amd import engine, sharding
from sigops_amd import lowering as LW
from sigops_amd import signals as S

N, NCH, FS = 100, 2, 10_000.0


def _leaf(fs, n=N, nch=NCH):
    return S.ArraySig(np.zeros((n, nch)), fs)


# name -> (class, SO_NODE_* kind, the family refusals print, the instance over leaves of rate fs,
#          the frames of every child that the first 10 frames of the node need)
ROWS = {
    "SampleAt": (S.SampleAtSignal, K.NODE_SAMPLEAT, "SampleAt",
                 lambda fs: S.SampleAtSignal(_leaf(fs), _leaf(fs, 40, 1), -1.5, 2.5, True, False), [N, 10]),
    "SampleAt-sinc": (S.SampleAtSignal, K.NODE_SAMPLEAT, "SampleAt",
                      lambda fs: S.SampleAtSignal(_leaf(fs), _leaf(fs, 40, 1), 0.0, 0.0, False, True, "sinc", 4, 0.5), [N, 10]),
    "Comb": (S.CombSignal, K.NODE_COMB, "Comb / Allpass", lambda fs: S.CombSignal(_leaf(fs), 7, 1.0, 0.25, 0.5), [10]),
    "Cumsum": (S.CumsumSignal, K.NODE_CUMSUM, "Cumsum / Integrate", lambda fs: S.CumsumSignal(_leaf(fs)), [10]),
    "Moving": (S.MovingSignal, K.NODE_MOVING, "MovingMax / MovingMin", lambda fs: S.MovingSignal(_leaf(fs), 7, 4, True), [14]),
    "MovingSum": (S.MovingSumSignal, K.NODE_MOVSUM, "MovingSum / MovingMean / MovingRMS",
                  lambda fs: S.MovingSumSignal(_leaf(fs), 7, 4, 2), [14]),
    "MovingRank": (S.MovingRankSignal, K.NODE_MOVRANK, "MovingMedian / MovingQuantile",
                   lambda fs: S.MovingRankSignal(_leaf(fs), 7, 4, 0.3), [14]),
    "Recur": (S.RecurSignal, K.NODE_RECUR, "Recur / OnePole / Smooth / PeakDecay", lambda fs: S.RecurSignal(0.75, _leaf(fs), 1), [10]),
    "Recur-signal": (S.RecurSignal, K.NODE_RECUR, "Recur / OnePole / Smooth / PeakDecay",
                     lambda fs: S.RecurSignal(_leaf(fs, 150, 1), _leaf(fs), 0), [10, 10]),
    "Recur2": (S.Recur2Signal, K.NODE_RECUR2, "Recur2 / Resonator / Sweep", lambda fs: S.Recur2Signal(0.75, -0.5, _leaf(fs)), [10]),
    "Recur2-signal": (S.Recur2Signal, K.NODE_RECUR2, "Recur2 / Resonator / Sweep",
                      lambda fs: S.Recur2Signal(_leaf(fs, 150, 1), _leaf(fs), _leaf(fs)), [10, 10, 10]),
}
each_row = pytest.mark.parametrize("row", list(ROWS))


def _params(x):
    """what a node holds besides its children and what it takes from them"""
    return {k: v for k, v in vars(x).items() if not k.startswith("_") and k not in ("fs", "children", "coefs") and not isinstance(v, S.AbstractSignal)}


def test_the_table_covers_every_stage_node():
    assert {row[0] for row in ROWS.values()} == set(S.StageSignal.__subclasses__())
    assert all(not cls.__subclasses__() for cls in S.StageSignal.__subclasses__())
    assert len({cls.family for cls in S.StageSignal.__subclasses__()}) == 8


@each_row
def test_it_lowers_to_its_node_kind(row):
    cls, kind, family, make, _ = ROWS[row]
    x = make(FS)
    assert type(x) is cls and x.family == family
    lw = LW.lower(x)
    nd = lw.nodes[lw.root]
    assert nd.kind == kind and nd.n_children == len(x.children)
    assert nd.nch == NCH and nd.nframes == S.nframes(x) and nd.fs == FS
    assert all(lw.nodes[nd.children[j]].kind == K.NODE_ARRAY for j in range(nd.n_children))


@each_row
def test_a_missing_rate_goes_to_the_children_that_take_one(row):
    cls, _, _, make, _ = ROWS[row]
    x = make(None)
    y = so.ToFramerate(x, 8000.0)
    assert type(y) is cls and y.fs == 8000.0 and _params(y) == _params(x) and len(y.children) == len(x.children)
    for j, (c, d) in enumerate(zip(x.children, y.children)):
        if cls is S.SampleAtSignal and j == 0:
            assert d is c and d.fs is None  # the table: a table of frames, its own rate is not consulted
        else:
            assert isinstance(d, S.ArraySig) and d.data is c.data and d.fs == 8000.0


@each_row
def test_a_rate_it_has_is_resampled(row):
    x = ROWS[row][3](FS)
    y = so.ToFramerate(x, 8000.0)
    assert isinstance(y, S.FilteredSignal) and isinstance(y.fn, S.ResamplerFn) and y.signal is x and y.fs == 8000.0


@each_row
def test_the_demand_of_every_child(row):
    x = ROWS[row][3](FS)
    need = {}
    LW._demand(x | so.Until(10 * so.frames), 10, need)
    assert [need.get(id(c)) for c in x.children] == [(m, 0) for m in ROWS[row][4]]
    assert len(need) == len(x.children)


@each_row
def test_blockstream_refuses_it_by_name(row):
    family, x = ROWS[row][2], ROWS[row][3](FS)
    for tree in (x, x | so.Filt(so.Lowpass, 1 * so.kHz), so.Mix(x, 1.0)):
        with pytest.raises(so.ErrorException, match="^BlockStream: " + family + " .*; not streamable$"):
            engine._streamable(tree)


@each_row
def test_shards_refuse_it_by_name(row):
    family, x = ROWS[row][2], ROWS[row][3](FS)
    text = "sharding a tree that contains " + family + " over several GPUs is not built"
    for what, call in (("shard_append", lambda: sharding.shard_append(so.Append(x, x), 0, 2)),
                       ("shard_time", lambda: sharding.shard_time(so.Mix(x, 1.0), 0, 2)),
                       ("shard_channels", lambda: sharding.shard_channels(x, 0, 2))):
        with pytest.raises(so.ErrorException) as e:
            call()
        assert str(e.value).startswith(what + ": " + text)


def test_of_several_families_the_shards_name_the_first_in_their_order():
    order = ["SampleAt", "Recur2", "Cumsum", "Moving", "MovingSum", "MovingRank"]  # (two that start at frame 0: the first met)
    nodes = [ROWS[r][3](FS) for r in order]
    for first in range(len(nodes)):
        rest = list(reversed(nodes[first:])) if first != 1 else list(reversed(nodes[3:])) + [nodes[1], nodes[2]]
        tree = so.Append(_leaf(FS), *rest)
        with pytest.raises(so.ErrorException, match="contains " + ROWS[order[first]][2] + " over several GPUs"):
            sharding.shard_time(tree, 0, 2)
