"""`SampleAt(x, pos)` / `Delay(x, d)` above the C-ABI (signals.py, lowering.py): length, rate and channel algebra, currying,
the `ToFramerate` rule, every refusal, the lowered node and the demand analysis -- and the NumPy restatement of the
device's uniform-knot formula (tests/sampleat_ref.py) held to `np.interp` bit for bit on exactly the inputs the device
tests read (tests/test_gpu_sampleat.py).  No GPU needed."""
import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import _capi as K
from sigops_amd import engine, sharding
from sigops_amd import lowering as LW
from sigops_amd import signals as S
from sampleat_ref import N_CHANNELS, N_RESULT, N_TABLE, positions, same_bits, sampleat_np, sampleat_restated, table

FS = 10 * so.kHz


def _x(n=100, c=2, dtype=np.float64, fs=FS):
    return so.Signal(np.asfortranarray(np.arange(n * c, dtype=dtype).reshape(c, n).T), fs)


# ---- 1. algebra ------------------------------------------------------------------------------------------------------
def test_length_rate_and_channels():
    x = _x(100, 3, np.float32, fs=44.1 * so.kHz)
    pos = so.Signal(np.zeros((40, 1)), FS)
    y = so.SampleAt(x, pos)
    assert isinstance(y, so.SampleAtSignal)
    assert so.nframes(y) == 40 and so.nchannels(y) == 3 and so.framerate(y) == 10_000.0  # pos's length and rate, x's channels
    assert so.sampletype(y) == np.float64  # always, as np.interp
    assert so.duration(y) == 40 / 10_000.0
    assert so.SampleAt(x, so.Signal(np.zeros((40, 3)), FS)).nch == 3
    assert so.SampleAt(x, so.Signal(np.zeros(40, dtype=np.float32), FS)).dtype == np.float64
    # an infinite pos gives an infinite result
    inf = so.SampleAt(x, so.Signal(so.elementwise(lambda t: t * 3.0), FS))
    assert so.isinf(so.nframes(inf))
    assert so.nframes(inf | so.Until(25 * so.frames)) == 25
    assert so.sampletype(y | so.ToEltype(np.float32)) == np.float32
    # a number is a constant position
    assert so.isinf(so.nframes(so.SampleAt(x, 2.5)))
    # a computed table
    assert so.nframes(so.SampleAt(x | so.Filt(so.Lowpass, 1 * so.kHz), pos)) == 40


def test_currying_and_piping():
    x = _x()
    pos = so.Signal(np.zeros((40, 1)), FS)
    y = x | so.SampleAt(pos, left=1.0, right=2.0, relative=True, wrap=True)
    assert isinstance(y, so.SampleAtSignal) and y.signal is x and y.pos is pos
    assert (y.left, y.right, y.relative, y.wrap) == (1.0, 2.0, True, True)
    z = np.zeros((100, 2)) | so.SampleAt(pos)  # a bare array on the left
    assert isinstance(z, so.SampleAtSignal) and z.nch == 2
    d = x | so.Delay(3)
    assert so.nframes(d) == 100
    assert so.nframes(so.pipe(x, so.Delay(3), so.Until(10 * so.frames))) == 10


def test_toframerate_gives_an_unknown_rate_to_pos_only():
    x = _x(fs=44.1 * so.kHz)
    pos = so.Signal(np.zeros((40, 1)))  # no rate
    y = so.SampleAt(x, pos)
    assert y.fs is None
    z = so.ToFramerate(y, 8 * so.kHz)
    assert isinstance(z, so.SampleAtSignal) and z.fs == 8000.0 and z.pos.fs == 8000.0
    assert z.signal is x and x.fs == 44100.0  # never pushed into the table
    assert so.nframes(z) == 40
    # a function pos without a rate takes it the same way
    f = so.ToFramerate(so.SampleAt(x, so.Signal(so.elementwise(lambda t: t))), 8 * so.kHz)
    assert isinstance(f, so.SampleAtSignal) and f.pos.fs == 8000.0


def test_toframerate_resamples_a_result_that_has_a_rate():
    y = so.SampleAt(_x(), so.Signal(np.zeros((40, 1)), FS))
    z = so.ToFramerate(y, 20 * so.kHz)
    assert isinstance(z, so.FilteredSignal) and isinstance(z.fn, so.ResamplerFn) and z.signal is y
    assert z.fs == 20_000.0 and so.nframes(z) == 80
    assert so.ToFramerate(y, FS) is y


def test_delay_is_a_relative_sampleat_over_the_frames_of_x():
    x = _x(100, 2)
    d = so.Delay(x, 3)
    assert isinstance(d, so.CutApply) and d.kind == "until" and so.nframes(d) == 100 and d.fs == 10_000.0
    sa = d.signal
    assert isinstance(sa, so.SampleAtSignal) and sa.signal is x and sa.relative and not sa.wrap and (sa.left, sa.right) == (0.0, 0.0)
    assert isinstance(sa.pos, so.NumberSig) and sa.pos.val == -3.0 and sa.pos.dtype == np.float64
    # a time: one multiplication with the rate of x
    assert so.Delay(x, 2 * so.ms).signal.pos.val == -(0.002 * 10_000.0)
    assert so.Delay(x, 7 * so.frames).signal.pos.val == -7.0
    # a signal: negated; a shorter one is extended with zeros, a longer one cut
    short = so.Delay(x, so.Signal(np.full((60, 1), 1.5), FS))
    assert so.nframes(short) == 100 and isinstance(short.signal, so.PaddedSignal)
    neg = short.signal.signal.pos
    assert isinstance(neg, so.MapSignal) and neg.fn == S.SUB and len(neg.signals) == 1
    assert so.nframes(so.Delay(x, so.Signal(np.full((160, 1), 1.5), FS))) == 100
    with pytest.raises(so.ErrorException, match="Delay"):
        so.Delay(_x(fs=None), 2 * so.ms)


# ---- 2. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_name_the_construct():
    x = _x()
    pos = so.Signal(np.zeros((40, 1)), FS)
    cases = [
        (lambda: so.SampleAt(so.Signal(np.sin, FS, ω=5 * so.Hz), pos), "known, finite length"),
        (lambda: so.SampleAt(so.Signal(np.zeros(10)) | so.Filt(so.Lowpass, 1 * so.kHz), pos), "known, finite length"),  # unknown: no rate
        (lambda: so.SampleAt(so.Signal(np.zeros((0, 2)), FS), pos), "at least one frame"),
        (lambda: so.SampleAt(so.Signal(np.arange(10), FS), pos), "Float32 or Float64"),
        (lambda: so.SampleAt(x, so.Signal(np.zeros((40, 3)), FS)), "3 channels; 1 or the table's 2"),
        (lambda: so.SampleAt(x, pos, left="zero"), "left must be a number"),
        (lambda: so.SampleAt(x, pos, right=None), "right must be a number"),
        (lambda: so.SampleAt(x, pos, left=1 + 2j), "left must be a number"),
        (lambda: engine._streamable(so.SampleAt(x, pos) | so.Filt(so.Lowpass, 1 * so.kHz)), "BlockStream: SampleAt"),
        (lambda: sharding.shard_time(so.SampleAt(x, pos), 0, 2), "SampleAt over several GPUs is not built"),
        (lambda: sharding.shard_channels(so.Mix(so.SampleAt(x, pos), 1.0), 0, 2), "SampleAt over several GPUs is not built"),
        (lambda: sharding.shard_append(so.Append(so.SampleAt(x, pos), so.SampleAt(x, pos)), 0, 2), "SampleAt over several GPUs is not built"),
    ]
    for make, words in cases:
        with pytest.raises(so.ErrorException) as e:
            make()
        assert "SampleAt" in str(e.value) and words in str(e.value), str(e.value)


# ---- 3. the lowered node ---------------------------------------------------------------------------------------------
def test_the_lowered_node():
    assert K.NODE_SAMPLEAT == 12
    x = _x(100, 2, np.float32)
    pos = so.Signal(np.zeros((40, 1)), FS)
    for kw, flags in (({}, 0), ({"relative": True}, 1), ({"wrap": True}, 2), ({"relative": True, "wrap": True}, 3)):
        lw = LW.lower(so.SampleAt(x, pos, left=-1.5, right=2.5, **kw))
        nd = lw.nodes[lw.root]
        assert nd.kind == K.NODE_SAMPLEAT and nd.i0 == flags and (nd.d0, nd.d1) == (-1.5, 2.5)
        assert nd.n_children == 2 and nd.nch == 2 and nd.dtype == K.SO_F64 and nd.nframes == 40 and nd.fs == 10_000.0
        cx, cp = lw.nodes[nd.children[0]], lw.nodes[nd.children[1]]
        assert cx.kind == K.NODE_ARRAY and cx.l0 == 100 and cx.dtype == K.SO_F32 and cx.nch == 2
        assert cp.kind == K.NODE_ARRAY and cp.l0 == 40 and cp.nch == 1
        assert (nd.i1, nd.i2, nd.i3, nd.l0, nd.l1, nd.s0, nd.s1) == (0,) * 7 and not nd.p0 and not nd.p1
    lw = LW.lower(so.Delay(x, 3))  # Until(SampleAt(x, CONST -3, relative))
    kinds = [lw.nodes[i].kind for i in range(lw.n)]
    assert kinds == [K.NODE_ARRAY, K.NODE_CONST, K.NODE_SAMPLEAT, K.NODE_UNTIL]
    assert lw.nodes[1].d0 == -3.0 and lw.nodes[2].i0 == 1 and lw.nodes[2].nframes == K.SO_LEN_INF and lw.nodes[3].l0 == 100


def test_demand_takes_the_table_whole_and_the_positions_in_part():
    x = _x(100, 2)
    pos = so.Signal(np.zeros((40, 1)), FS)
    tree = so.SampleAt(x, pos)
    need = {}
    LW._demand(tree | so.Until(10 * so.frames), 10, need)
    assert need[id(x)] == (100, 0) and need[id(pos)] == (10, 0)
    need = {}
    LW._demand(tree | so.After(5 * so.frames) | so.Until(10 * so.frames), 10, need)
    assert need[id(x)] == (100, 0) and need[id(pos)] == (15, 5)  # the skip is handed on to pos, never to x
    # a host-drawn noise as the positions is sized by what the sink reaches; as the table it is drawn whole
    noise = so.Signal(so.randn, FS)
    need = {}
    LW._demand(so.SampleAt(noise | so.Until(64 * so.frames), noise) | so.Until(7 * so.frames), 7, need)
    assert need[id(noise)] == (64, 0)


# ---- 4. the restatement is NumPy's np.interp ----------------------------------------------------------------------------
def _hold(x, pos, **kw):
    want = sampleat_np(x, pos, **kw)
    got = sampleat_restated(x, pos, **kw)
    assert same_bits(got, want), (x.shape, pos.shape, kw, np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))).ravel())[:5])


@pytest.mark.parametrize("N", N_TABLE)
def test_the_restatement_equals_numpy_bit_for_bit(N):
    for C in N_CHANNELS:
        for L in N_RESULT:
            x = table(N, C)
            pos = positions(N, L)
            for kw in ({}, {"left": -7.5, "right": np.inf}, {"wrap": True}, {"relative": True}, {"relative": True, "wrap": True}):
                _hold(x, pos, **kw)
            _hold(x, positions(N, L, C), left=1.0, right=-0.0)
    for C in (1, 3):
        xn = table(N, C, nonfinite=True)
        pos = positions(N, 1001, C)
        for kw in ({}, {"wrap": True}, {"left": np.nan, "right": -np.inf}):
            _hold(xn, pos, **kw)
        _hold(table(N, C, np.float32, nonfinite=True), positions(N, 1001, 1, np.float32), left=0.25)
        _hold(table(N, C, np.float32), positions(N, 1001, 1, np.float32), wrap=True)


def test_both_slope_fall_backs_are_taken_by_the_planted_tables():
    x = table(65, 1, nonfinite=True)[:, 0]
    f0, f1 = x[:-1], x[1:]
    with np.errstate(all="ignore"):
        s = f1 - f0
        mid = s * 0.5 + f0
        other = s * -0.5 + f1
    first = np.isnan(mid) & ~np.isnan(other)
    second = np.isnan(mid) & np.isnan(other) & (f0 == f1)
    assert first.any() and second.any() and (x == 0).any() and np.signbit(x[x == 0]).all()
    pos = positions(65, 1001)
    assert all((pos == k + 0.5).any() for k in np.flatnonzero(first | second))  # ... and the positions reach those segments


def test_integer_delays_and_wrapped_positions_of_the_definition():
    x = table(64, 2)
    zero = np.zeros((64, 1))
    assert same_bits(sampleat_np(x, zero, relative=True), x)
    for k in (1, 63, 64, 65):
        want = np.zeros_like(x)
        want[k:] = x[:max(64 - k, 0)]
        assert same_bits(sampleat_np(x, np.full((64, 1), -float(k)), relative=True), want)
    p = np.asarray([-1.0, -64.0, 64.0, 129.5, -0.5]).reshape(-1, 1)
    w = sampleat_np(x, p, wrap=True)
    assert same_bits(w[:3], x[[63, 0, 0]]) and w[3, 0] == 0.5 * (x[2, 0] - x[1, 0]) + x[1, 0] and w[4, 0] == (x[0, 0] - x[63, 0]) * 0.5 + x[63, 0]
