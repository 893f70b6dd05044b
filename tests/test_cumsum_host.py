"""`Cumsum(x)` / `Integrate(x)` above the C-ABI (signals.py, lowering.py): the NumPy definition the device is held to
(tests/cumsum_ref.py) checked against its scalar restatement, against itself on every prefix, against `np.cumsum` where
every order of additions gives the same bits and against `math.fsum`; length, rate and channel algebra, currying, the
`ToFramerate` rules, every refusal and the lowered node.  No GPU needed."""
import math

import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import _capi as K
from sigops_amd import engine, sharding
from sigops_amd import lowering as LW
from cumsum_ref import (BOUNDARIES, CH, G, L, LENGTHS, T, W, cumsum_1d, cumsum_loop, cumsum_ref, huge, integrate_ref, kernel_constants,
                        planted, same_bits, signal, wide)

FS = 10 * so.kHz


def _x(n=100, c=2, dtype=np.float64, fs=FS):
    return so.Signal(np.asfortranarray(np.arange(n * c, dtype=dtype).reshape(c, n).T), fs)


# ---- 1. the reference ------------------------------------------------------------------------------------------------
def test_the_constants_are_the_kernels():
    assert kernel_constants() == (L, G) and (L, W, T, G, CH) == (16, 64, 1024, 16, 16384)
    assert LENGTHS == [1, 15, 16, 17, 1023, 1024, 1025, 16383, 16384, 16385, 2 * 16384 + 1, 3 * 16384 + 77]


@pytest.mark.parametrize("make", [signal, wide, huge, planted])
def test_the_block_form_equals_the_scalar_loop_bit_for_bit(make):
    for N in (1, L, L + 1, T - 1, T + L + 3, CH + 1, 2 * CH + T + L + 5):
        x = make(N, 1)[:, 0]
        with np.errstate(all="ignore"):
            assert same_bits(cumsum_1d(np.ascontiguousarray(x)), cumsum_loop(x)), (make.__name__, N)
    x32 = signal(CH + 77, 1, np.float32)
    assert same_bits(cumsum_ref(x32)[:, 0], cumsum_loop(x32[:, 0].astype(np.float64)))


@pytest.mark.parametrize("make", [signal, wide, huge])
def test_a_prefix_does_not_depend_on_what_follows(make):
    """the tree depends on the frame index only: the sum of a shorter signal is the prefix of a longer one's"""
    N = 3 * CH + 77
    x = make(N, 1)
    whole = cumsum_ref(x)
    for m in [b for b in BOUNDARIES if 0 < b <= N] + [N - 1, N]:
        assert same_bits(cumsum_ref(x[:m]), whole[:m]), (make.__name__, m)


def test_a_single_run_and_exact_sums_equal_np_cumsum():
    for n in range(1, L + 1):  # one run: the sequential sum
        for x in (signal(n, 2), wide(n, 2), huge(n, 2)):
            with np.errstate(all="ignore"):
                assert same_bits(cumsum_ref(x), np.asfortranarray(np.cumsum(x, axis=0))), n
    rng = np.random.default_rng(3)
    for N in (T + 5, CH + T + 3, 3 * CH + 77):  # small integers: every partial sum is exact in any order
        x = np.asfortranarray(rng.integers(-1000, 1001, (N, 2)).astype(np.float64))
        assert same_bits(cumsum_ref(x), np.asfortranarray(np.cumsum(x, axis=0))), N


@pytest.mark.parametrize("N", [T, CH, 3 * CH + 77])
def test_accuracy_against_fsum(N):
    """Higham's bound for a summation tree in which no summand passes through more than h additions: 15 in the run, 6
    Kogge-Stone steps, 2 to reach the tile's values, at most 15 tile carries and one per chunk: h = 40 + chunks"""
    u = 2.0 ** -53
    h = 40 + -(-N // CH)
    x = signal(N, 1)[:, 0]
    y = cumsum_ref(x)[:, 0]
    idx = sorted({i for i in list(range(0, N, 97)) + [b - 1 for b in BOUNDARIES if 0 < b <= N] + [N - 1]})
    worst = 0.0
    for i in idx:
        exact = math.fsum(x[:i + 1])
        mass = math.fsum(np.abs(x[:i + 1]))
        err = abs(y[i] - exact)
        worst = max(worst, err / (u * mass))
        assert err <= h * u / (1 - h * u) * mass, (i, err, mass)
    print(f"N={N}: worst error {worst:.3f} u sum|x| (the bound: {h})")


def test_the_sign_of_zero_survives():
    for N in (1, L + 1, T + 1, CH + T + L + 1):
        y = cumsum_ref(np.full((N, 1), -0.0))
        assert np.signbit(y).all() and not y.any(), N
        z = cumsum_ref(np.zeros((N, 1)))
        assert not np.signbit(z).any()
    x = np.full(40, -0.0)
    x[20] = 0.0  # (-0) + (+0) = +0 from there on
    y = cumsum_ref(x)[:, 0]
    assert np.signbit(y[:20]).all() and not np.signbit(y[20:]).any()


def test_infinities_and_nans_appear_where_the_tree_says():
    for N, a, b in ((100, 17, 40), (3 * T, T - 1, T), (2 * CH + 5, CH - 1, CH + T + 3), (2 * CH + 5, 3, 2 * CH)):
        x = signal(N, 1)
        x[a] = np.inf
        x[b] = -np.inf
        y = cumsum_ref(x)[:, 0]
        assert np.isfinite(y[:a]).all() and (y[a:b] == np.inf).all() and np.isnan(y[b:]).all(), (N, a, b)
    for N, k in ((50, 0), (3 * T, T + L), (CH + 9, CH - 1), (2 * CH + 5, CH + 1)):
        x = signal(N, 1)
        x[k] = np.nan
        y = cumsum_ref(x)[:, 0]
        assert np.isfinite(y[:k]).all() and np.isnan(y[k:]).all(), (N, k)


# ---- 2. algebra ------------------------------------------------------------------------------------------------------
def test_length_rate_channels_and_type():
    x = _x(100, 3, np.float32, fs=44.1 * so.kHz)
    y = so.Cumsum(x)
    assert isinstance(y, so.CumsumSignal) and y.evaltrait == "computed" and y.signal is x and y.children == (x,)
    assert so.nframes(y) == 100 and so.nchannels(y) == 3 and so.framerate(y) == 44_100.0
    assert so.sampletype(y) == np.float64 and so.duration(y) == 100 / 44_100.0
    assert so.nframes(so.Cumsum(x | so.Filt(so.Lowpass, 1 * so.kHz))) == 100  # a computed child
    assert so.nframes(so.Signal(np.sin, FS, ω=5 * so.Hz) | so.Until(300 * so.frames) | so.Cumsum) == 300
    assert so.sampletype(y | so.ToEltype(np.float32)) == np.float32
    assert so.Cumsum(_x(fs=None)).fs is None


def test_currying_and_piping():
    x = _x()
    y = x | so.Cumsum
    assert isinstance(y, so.CumsumSignal) and y.signal is x
    z = np.zeros((100, 2)) | so.Cumsum  # a bare array on the left
    assert isinstance(z, so.CumsumSignal) and z.nch == 2
    assert so.nframes(so.pipe(x, so.Cumsum, so.Cumsum, so.Until(10 * so.frames))) == 10
    w = x | so.Integrate
    assert isinstance(w, so.MapSignal) and so.nframes(w) == 100 and so.framerate(w) == 10_000.0 and so.sampletype(w) == np.float64


def test_integrate_is_cumsum_times_the_reciprocal_rate():
    x = _x(100, 2, np.float32, fs=44.1 * so.kHz)
    y = so.Integrate(x)
    assert isinstance(y, so.MapSignal) and y.fn == so.signals.MUL and len(y.signals) == 2
    c, k = y.signals
    assert isinstance(c, so.CumsumSignal) and c.signal is x
    while isinstance(k, so.MapSignal):  # (`Uniform` spreads the number over the channels of x)
        assert len(k.signals) == 1
        k = k.signals[0]
    assert isinstance(k, so.NumberSig) and k.dtype == np.float64 and k.val == 1.0 / 44_100.0 and not k.dB
    lw = LW.lower(y)
    root = lw.nodes[lw.root]
    assert root.kind == K.NODE_MAP and root.n_children == 2 and lw.nodes[root.children[0]].kind == K.NODE_CUMSUM
    kinds = [lw.nodes[i].kind for i in range(lw.n)]
    assert kinds.count(K.NODE_CUMSUM) == 1 and kinds.count(K.NODE_CONST) == 1 and kinds.count(K.NODE_ARRAY) == 1
    const = lw.nodes[kinds.index(K.NODE_CONST)]
    assert const.d0 == 1.0 / 44_100.0 and const.dtype == K.SO_F64
    # the value the device is held to: one more rounding a sample
    data = signal(50, 2)
    assert same_bits(integrate_ref(data, 8000.0), np.asfortranarray(cumsum_ref(data) * (1.0 / 8000.0)))


def test_toframerate():
    y = so.Cumsum(_x(fs=None))  # no rate: it is handed to x
    z = so.ToFramerate(y, 8 * so.kHz)
    assert isinstance(z, so.CumsumSignal) and z.fs == 8000.0 and z.signal.fs == 8000.0 and so.nframes(z) == 100
    y = so.Cumsum(_x())  # a rate: resampled like any computed signal
    z = so.ToFramerate(y, 20 * so.kHz)
    assert isinstance(z, so.FilteredSignal) and isinstance(z.fn, so.ResamplerFn) and z.signal is y
    assert z.fs == 20_000.0 and so.nframes(z) == 200
    assert so.ToFramerate(y, FS) is y


# ---- 3. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_name_the_construct():
    x = _x()
    cases = [
        (lambda: so.Cumsum(so.Signal(np.sin, FS, ω=5 * so.Hz)), "Cumsum", "use `Until`"),
        (lambda: so.Signal(np.sin, FS, ω=5 * so.Hz) | so.Cumsum, "Cumsum", "use `Until`"),
        (lambda: so.Cumsum(so.Signal(np.zeros(10)) | so.Filt(so.Lowpass, 1 * so.kHz)), "Cumsum", "use `Until`"),  # unknown: no rate
        (lambda: so.Integrate(so.Signal(np.sin, FS, ω=5 * so.Hz)), "Integrate", "use `Until`"),
        (lambda: so.Cumsum(so.Signal(np.arange(10), FS)), "Cumsum", "Float32 or Float64"),
        (lambda: so.Integrate(so.Signal(np.arange(10), FS)), "Integrate", "Float32 or Float64"),
        (lambda: so.Integrate(_x(fs=None)), "Integrate", "needs a frame rate"),
        (lambda: np.zeros(10) | so.Integrate, "Integrate", "needs a frame rate"),
        (lambda: engine._streamable(so.Cumsum(x) | so.Filt(so.Lowpass, 1 * so.kHz)), "BlockStream: Cumsum", "not streamable"),
        (lambda: engine._streamable(so.Mix(so.Integrate(x), 1.0)), "BlockStream: Cumsum", "not streamable"),
        (lambda: sharding.shard_time(so.Cumsum(x), 0, 2), "Cumsum", "Cumsum / Integrate over several GPUs is not built"),
        (lambda: sharding.shard_channels(so.Mix(so.Integrate(x), 1.0), 0, 2), "Cumsum", "Cumsum / Integrate over several GPUs is not built"),
        (lambda: sharding.shard_append(so.Append(so.Cumsum(x), so.Cumsum(x)), 0, 2), "Cumsum", "Cumsum / Integrate over several GPUs is not built"),
    ]
    for make, name, words in cases:
        with pytest.raises(so.ErrorException) as e:
            make()
        assert name in str(e.value) and "Cumsum" in str(e.value) and words in str(e.value), str(e.value)
    with pytest.raises(so.ErrorException) as e:  # the generalised refusal still names Comb
        sharding.shard_time(so.Comb(x, 7, 0.5), 0, 2)
    assert "Comb / Allpass over several GPUs is not built" in str(e.value)


# ---- 4. the lowered node ---------------------------------------------------------------------------------------------
def test_the_lowered_node():
    assert K.NODE_CUMSUM == 14
    x = _x(100, 2, np.float32)
    lw = LW.lower(so.Cumsum(x))
    nd = lw.nodes[lw.root]
    assert nd.kind == K.NODE_CUMSUM and nd.n_children == 1 and nd.nch == 2 and nd.dtype == K.SO_F64 and nd.nframes == 100 and nd.fs == 10_000.0
    cx = lw.nodes[nd.children[0]]
    assert cx.kind == K.NODE_ARRAY and cx.l0 == 100 and cx.dtype == K.SO_F32 and cx.nch == 2
    assert (nd.i0, nd.i1, nd.i2, nd.i3, nd.l0, nd.l1, nd.s0, nd.s1, nd.d0, nd.d1, nd.d2, nd.d3) == (0,) * 12 and not nd.p0 and not nd.p1


def test_demand_starts_at_frame_0_whatever_the_window():
    x = _x(100, 2)
    tree = so.Cumsum(x)
    need = {}
    LW._demand(tree | so.Until(10 * so.frames), 10, need)
    assert need[id(x)] == (10, 0)
    need = {}
    LW._demand(tree | so.After(5 * so.frames) | so.Until(10 * so.frames), 10, need)
    assert need[id(x)] == (15, 0)  # the skipped frames are summed too: the skip is not handed on
