"""What a `BlockStream` needs of the device-only nodes, above the C-ABI: the refusals of a stream with nowhere to keep state
(`engine._streamable(tree)`, word for word what they were), the same check with a state store, what every family
declares it carries, the node fields a carry lowers to, the checkpoint rule and the walk that tells the carrying nodes of
one push from those of the next.  No GPU, no engine library: trees and node tables only."""
import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import _capi as K
from sigops_amd import engine
from sigops_amd import lowering as LW
from sigops_amd import signals as S
from cumsum_ref import CH

N, NCH, FS = 100, 2, 10_000.0


def _leaf(n=N, nch=NCH):
    return S.ArraySig(np.zeros((n, nch)), FS)


# family -> (an instance, the whole text `_streamable(tree)` raises for it, the Float64 a channel a stream carries for it)
NOT_BUILT = ", and that is not built"
ROWS = {
    "SampleAt": (lambda: S.SampleAtSignal(_leaf(), _leaf(40, 1), 0.0, 0.0, True, False),
                 "BlockStream: SampleAt reads its table at any position, and a stream keeps only a tail of its input resident; not streamable", None),
    "Comb": (lambda: S.CombSignal(_leaf(), 7, 1.0, 0.25, 0.5),
             "BlockStream: Comb / Allpass would have to carry the D frames of its delay line from one push to the next" + NOT_BUILT + "; not streamable", 14),
    "Cumsum": (lambda: S.CumsumSignal(_leaf()),
               "BlockStream: Cumsum / Integrate would have to carry its running sum (and its place in the summation tree) from one push to the next" + NOT_BUILT
               + "; not streamable", 1),
    "Moving": (lambda: S.MovingSignal(_leaf(), 7, 4, True),
               "BlockStream: MovingMax / MovingMin would have to keep the `back` input frames of its window from one push to the next and hold `ahead` output frames back"
               + NOT_BUILT + "; not streamable", 0),
    "MovingSum": (lambda: S.MovingSumSignal(_leaf(), 7, 4, 2),
                  "BlockStream: MovingSum / MovingMean / MovingRMS would have to keep the `back` input frames of its window from one push to the next, hold `ahead` output "
                  "frames back and keep its place in the summation tree" + NOT_BUILT + "; not streamable", 0),
    "MovingRank": (lambda: S.MovingRankSignal(_leaf(), 7, 4, 0.3),
                   "BlockStream: MovingMedian / MovingQuantile would have to keep the `back` input frames of its window from one push to the next and hold `ahead` output "
                   "frames back" + NOT_BUILT + "; not streamable", 0),
    "Recur": (lambda: S.RecurSignal(0.75, _leaf(), 1),
              "BlockStream: Recur / OnePole / Smooth / PeakDecay would have to carry its last value (and its place in the tree of the scan) from one push to the next"
              + NOT_BUILT + "; not streamable", 1),
    "Recur2": (lambda: S.Recur2Signal(_leaf(150, 1), _leaf(), _leaf()),
               "BlockStream: Recur2 / Resonator / Sweep would have to carry its last two values (and its place in the tree of the scan) from one push to the next"
               + NOT_BUILT + "; not streamable", 2),
}
each_row = pytest.mark.parametrize("row", list(ROWS))


def test_the_table_covers_every_stage_node():
    assert {type(make()) for make, _, _ in ROWS.values()} == set(S.StageSignal.__subclasses__())


@each_row
def test_with_nowhere_to_keep_state_every_family_is_refused_as_before(row):
    make, text, _ = ROWS[row]
    for tree in (make(), make() | so.Filt(so.Lowpass, 1 * so.kHz), so.Mix(make(), 1.0)):
        with pytest.raises(so.ErrorException) as e:
            engine._streamable(tree)
        assert str(e.value) == text
        with pytest.raises(so.ErrorException) as e:
            engine._streamable(tree, None)
        assert str(e.value) == text


@each_row
def test_with_a_state_store_seven_families_pass_and_sampleat_is_refused_by_name(row):
    make, text, carried = ROWS[row]
    for store in ([], object()):
        for tree in (make(), make() | so.Filt(so.Lowpass, 1 * so.kHz), so.Mix(make(), 1.0)):
            if carried is None:
                with pytest.raises(so.ErrorException) as e:
                    engine._streamable(tree, store)
                assert str(e.value) == text and text.startswith("BlockStream: SampleAt ")
            else:
                engine._streamable(tree, store)


def test_a_state_store_lifts_no_other_refusal():
    x = _leaf()
    for tree, text in ((so.Normpower(so.Cumsum(x)), "Normpower needs the whole signal"), (so.Cumsum(x) | so.RampOff(10 * so.frames), "a ramp at the END"),
                       (so.Cumsum(so.Pad(x, so.mirror) | so.Until(200 * so.frames)), "lastframe / cycle / mirror padding")):
        with pytest.raises(so.ErrorException, match=text):
            engine._streamable(tree, [])


@each_row
def test_what_a_stream_carries_for_the_family(row):
    make, _, carried = ROWS[row]
    x = make()
    assert x.stream_doubles() == carried and (carried is None or type(carried) is int)
    assert "stream_doubles" in vars(type(x)), "declared by the class itself, beside not_streamable"
    assert S.CombSignal(_leaf(), 4800, 1.0, 0.0, 0.5).stream_doubles() == 2 * 4800  # (x, y) per frame of the delay line


@each_row
def test_the_carry_fields_are_zero_unless_a_carry_is_attached(row):
    make, _, carried = ROWS[row]
    x = make()
    assert x.carry is None and "carry" not in vars(x) and "carry" not in x.fields()
    before = dict(x.fields())
    lw = LW.lower(x)
    nd = lw.nodes[lw.root]
    if row != "SampleAt":  # (its sinc form uses p0 and s0 for the tap table: never a carrying node)
        assert (nd.s0, nd.p0, nd.p1) == (0, None, None) and lw.carry_nodes == []
    if not carried:
        return
    rec_in, rec_out = np.zeros(NCH * carried), np.zeros(NCH * carried)
    x.carry = (3 * CH, rec_in.ctypes.data, rec_out.ctypes.data)
    lw = LW.lower(x)
    nd = lw.nodes[lw.root]
    assert (nd.s0, nd.p0, nd.p1) == (3 * CH, rec_in.ctypes.data, rec_out.ctypes.data)
    assert lw.carry_nodes == [(lw.root, x)] and x.fields() == before
    x.carry = (0, 0, rec_out.ctypes.data)  # from rest, with a record to leave
    nd = LW.lower(x).nodes[lw.root]
    assert (nd.s0, nd.p0, nd.p1) == (0, None, rec_out.ctypes.data)
    for f in ("i0", "i1", "i2", "i3", "l0", "l1", "d0", "d1", "d2", "d3"):  # every other field as without a carry
        x.carry = None
        plain = getattr(LW.lower(x).nodes[lw.root], f)
        x.carry = (CH, rec_in.ctypes.data, 0)
        assert getattr(LW.lower(x).nodes[lw.root], f) == plain


def test_the_checkpoint_rule():
    """the state left is the one that enters the last chunk holding a frame read, k1 = (need - 1) // 16384: a push that ends
    exactly on a chunk boundary has not entered the next chunk"""
    from cumsum_ref import _constant

    assert S.SCAN_CHUNK == CH == 16384 == _constant("kCumsumRun") * 64 * _constant("kCumsumTiles")
    for make in (ROWS["Cumsum"][0], ROWS["Recur"][0], ROWS["Recur2"][0]):  # what BlockStream holds every plan's report to
        rule = make().stream_checkpoint
        assert [rule(0, n) for n in (16384, 16385, 32768)] == [0, 16384, 16384]
        assert [rule(0, n) for n in (0, 1, 16383, 32769, 70001)] == [0, 0, 0, 32768, 65536]
        assert [rule(16384, n) for n in (16385, 32768, 32769)] == [16384, 16384, 32768]  # resumed: unchanged until the next chunk is entered
        for need in (1, 16384, 16385, 32768, 49153):
            k1 = (need - 1) // 16384
            assert rule(0, need) == k1 * 16384 and k1 * 16384 < need <= (k1 + 1) * 16384
    comb = ROWS["Comb"][0]().stream_checkpoint
    assert [comb(r, n) for r, n in ((0, 1), (0, 16384), (500, 501), (500, 70001))] == [1, 16384, 501, 70001]  # where the push ended
    assert all(not hasattr(ROWS[r][0](), "stream_checkpoint") for r in ("SampleAt", "Moving", "MovingSum", "MovingRank"))


def _dag(x):
    """one Smooth read twice, a Comb beside it, a Cumsum over a moving window, a node without state in between"""
    y = so.Smooth(x, 1 * so.ms)
    return so.Mix(y, so.Comb(y, 7, 0.5), so.Cumsum(so.MovingMax(y, 5)), so.Recur2(0.5, 0.25, x))


def test_the_walk_lists_every_carrying_node_once_in_a_stable_order():
    trees = [_dag(_leaf()) for _ in range(3)]
    walks = [engine._carrying(t) for t in trees]
    for w in walks:
        assert [type(n).__name__ for n in w] == ["RecurSignal", "CombSignal", "CumsumSignal", "Recur2Signal"]
        assert len({id(n) for n in w}) == 4
        assert w[1].signal is w[0] and w[2].signal.signal is w[0]  # the node read twice (and a third time): one entry
    assert engine._carrying(trees[0]) == walks[0]  # the same tree: the same list
    assert engine._carrying(so.MovingMax(_leaf(), 5)) == [] and engine._carrying(_leaf()) == []
    # the lowering numbers them in the same order: node-table order is the walk's
    for n in walks[0]:
        n.carry = (0, 0, 1)
    lw = LW.lower(trees[0])
    assert [s for _, s in lw.carry_nodes] == walks[0] and [i for i, _ in lw.carry_nodes] == sorted(i for i, _ in lw.carry_nodes)


def test_a_refusal_names_its_node():
    tree = _dag(_leaf())
    nodes = engine._carrying(tree)
    for n in nodes:
        n.carry = (0, 0, 1)
    lw = LW.lower(tree)
    for k, (idx, _) in enumerate(lw.carry_nodes):
        err = so.ErrorException("whatever the planner words it as")
        assert engine._refused(err, nodes) is None  # (not a planner's error: nothing says which table it speaks of)
        err.lowered, err.resume_node = lw, idx  # what `Plan` leaves on it, from the "[resume node N]" of the refusal
        assert engine._refused(err, nodes) == k
    other = so.ErrorException("frame 5 of a streamed leaf is needed, but frames before 64 are no longer resident (raise the stream's history)")
    other.lowered, other.resume_node = lw, -1
    assert engine._refused(other, nodes) is None
