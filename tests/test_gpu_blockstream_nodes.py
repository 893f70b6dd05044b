"""`BlockStream` over the device-only nodes: `Cumsum`, `Recur`, `Recur2`, `Comb` and their wrappers resumed from carried
state (include/sigops.h "Carried state"; csrc/k_cumsum.hip, k_recur.hip, k_recur2.hip, k_comb.hip), the moving windows
from the resident tail.  These nodes are bit-exact by contract, so every comparison is equality of bits, `-0.0` included:
the concatenated outputs against `so.sink` of the pipeline over the whole input, and against the family's NumPy
definition wherever the family's own test file compares bit for bit (a coefficient signal enters the definition as its
own sunk sub-tree).

The input is 70 001 frames by 2 channels -- four chunks of 16384 frames and a ragged tail -- pushed in two lists of sizes,
one of which ends pushes exactly on chunk boundaries; with a history of 24 000 frames the head of the input has left
device memory before the last pushes (asserted), so a stage that still started at frame 0 would be refused: the work and
the memory of a push are bounded."""
import numpy as np
import pytest

import sigops_amd as so
from sigops_amd.engine import Plan
from oracle_bridge import relerr
from comb_ref import comb_ref
from cumsum_ref import cumsum_ref, integrate_ref, same_bits
from moving_ref import moving_ref
from movingmedian_ref import movrank_ref
from movingsum_ref import movingsum_ref
from recur2_ref import recur2_ref
from recur_ref import recur_ref

pytestmark = pytest.mark.gpu
FS = 10 * so.kHz
N, NCH, HISTORY, CHUNK = 70_001, 2, 24_000, 16_384


def _rest(sizes, n=N):
    return sizes + [n - sum(sizes)]


# pushes of one frame, across and onto chunk boundaries (4099 + 1 + 12285 = 16385, + 16383 = 32768), a block longer than a chunk
SIZES_A = _rest([4099, 1, 12285, 16383, 1, 7, 20000])
# pushes that END exactly at frames 16384 and 32768: the edge of "the last chunk that holds a frame read"
SIZES_B = _rest([1000, 15384, 16384, 20000])
BOTH = pytest.mark.parametrize("sizes", [SIZES_A, SIZES_B], ids=["ragged", "chunk-ends"])


@pytest.fixture(scope="module")
def x64():
    x = np.random.default_rng(2024).standard_normal((N, NCH))
    x[[0, 5, 16383, 16384, 40000], 0] = -0.0  # zeros of the other sign, on both sides of a chunk boundary
    return x


@pytest.fixture(scope="module")
def x32(x64):
    x = x64.astype(np.float32)
    return x


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bit_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} against {want.dtype} {want.shape}"
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} samples differ, first at {np.argwhere(bad)[0]}"
    assert same_bits(got, want), f"{what}: a zero of the other sign"


def streamed(pipe, x, sizes, history=HISTORY, head_leaves=True):
    """push `x` in `sizes`, concatenate the outputs and `finish()`: -> (frames x channels, frames per push and of finish)"""
    assert sum(sizes) == x.shape[0]
    bs = so.BlockStream(pipe, FS, nch=x.shape[1], dtype=x.dtype, history=history)
    outs, pos = [], 0
    for m in sizes:
        outs.append(bs.push(dev(x[pos:pos + m])).cpu().numpy())
        pos += m
    outs.append(bs.finish().cpu().numpy())
    if head_leaves:
        assert bs.start > 0, "the head of the input never left device memory: the run proves nothing about bounded work"
    return np.concatenate(outs, axis=0), [o.shape[0] for o in outs]


def whole(pipe, x):
    y = so.sink(pipe(so.Signal(np.asfortranarray(x), FS)), so.Array)
    return y.reshape(y.shape[0], -1)


def sunk(tree_of, x):
    """a sub-tree over the whole input, sunk on its own: what a coefficient signal is in the family's definition"""
    return np.asfortranarray(whole(tree_of, x))


def check(pipe, x, sizes, ref=None, what="", **kw):
    got, counts = streamed(pipe, x, sizes, **kw)
    bit_equal(got, whole(pipe, x), f"{what}: the stream against the whole sink")
    if ref is not None:
        bit_equal(got, ref() if callable(ref) else ref, f"{what}: the stream against the NumPy definition")
    return got, counts


# ---- Cumsum / Integrate --------------------------------------------------------------------------------------------------
@BOTH
def test_cumsum_float64(x64, sizes):
    check(lambda s: so.Cumsum(s), x64, sizes, lambda: cumsum_ref(x64), "Cumsum")


@BOTH
def test_cumsum_float32_input(x32, sizes):
    check(lambda s: so.Cumsum(s), x32, sizes, lambda: cumsum_ref(x32), "Cumsum of Float32")


@BOTH
def test_integrate(x64, sizes):
    check(lambda s: so.Integrate(s), x64, sizes, lambda: integrate_ref(x64, 10_000.0), "Integrate")


# ---- Recur and its wrappers ----------------------------------------------------------------------------------------------
@BOTH
def test_recur_constant(x64, sizes):
    check(lambda s: so.Recur(0.999, s), x64, sizes, lambda: recur_ref(0.999, x64, 0), "Recur(0.999)")


def _coef(s):  # a coefficient in (0.9, 1) computed from the stream itself
    return so.OperateOn(so.elementwise(lambda v: 0.95 + 0.04 * np.tanh(v)), s)


@BOTH
def test_recur_coefficient_signal_from_the_stream(x64, sizes):
    check(lambda s: so.Recur(_coef(s), s), x64, sizes, lambda: recur_ref(sunk(_coef, x64), x64, 0), "Recur(a(x), x)")


@BOTH
def test_recur_one_channel_of_coefficients_under_two_of_b(x64, sizes):
    a = lambda s: _coef(so.ToChannels(s, 1))  # noqa: E731
    check(lambda s: so.Recur(a(s), s), x64, sizes, lambda: recur_ref(sunk(a, x64), x64, 0), "Recur(a of one channel, x)")


@BOTH
def test_peakdecay_is_op_1(x64, sizes):
    mag = np.abs(x64)
    check(lambda s: so.PeakDecay(s, r=0.9995), mag, sizes, lambda: recur_ref(0.9995, mag, 1), "PeakDecay")


@BOTH
def test_onepole_and_smooth(x64, sizes):
    check(lambda s: so.OnePole(s, 200 * so.Hz), x64, sizes, what="OnePole")
    check(lambda s: so.Smooth(s, 5 * so.ms), x64, sizes, what="Smooth")


# ---- Recur2 and its wrappers ---------------------------------------------------------------------------------------------
@BOTH
def test_recur2_constants(x64, sizes):
    check(lambda s: so.Recur2(1.2, -0.72, s), x64, sizes, lambda: recur2_ref(1.2, -0.72, x64), "Recur2(1.2, -0.72)")


@BOTH
def test_recur2_both_coefficients_signals(x64, sizes):
    a1 = lambda s: so.OperateOn(so.elementwise(lambda v: 1.2 + 0.1 * np.tanh(v)), s)  # noqa: E731
    a2 = lambda s: so.OperateOn(so.elementwise(lambda v: -0.72 + 0.05 * np.tanh(v)), so.ToChannels(s, 1))  # noqa: E731
    check(lambda s: so.Recur2(a1(s), a2(s), s), x64, sizes, lambda: recur2_ref(sunk(a1, x64), sunk(a2, x64), x64), "Recur2(a1(x), a2(x), x)")


@BOTH
def test_recur2_poles_next_to_one_carry_the_carry_kernels_state(x64, sizes):
    """a double pole at 0.9995: the state the carry kernel applies in double-doubles and the last two outputs, which walk the
    loop, differ in their bits here -- a stream that carried the outputs would not reproduce the whole sink"""
    check(lambda s: so.Recur2(1.999, -0.999001, s), x64, sizes, lambda: recur2_ref(1.999, -0.999001, x64), "Recur2 next to z = 1")


def _fc(s):  # a centre frequency in Hz that follows the stream
    return so.OperateOn(so.elementwise(lambda v: 800.0 + 300.0 * np.tanh(v)), so.ToChannels(s, 1))


@BOTH
def test_resonator_and_sweep_with_an_fc_signal(x64, sizes):
    check(lambda s: so.Resonator(s, _fc(s), 40 * so.Hz), x64, sizes, what="Resonator(fc(x))")
    check(lambda s: so.Sweep(s, so.Lowpass, _fc(s), 2.0), x64, sizes, what="Sweep(Lowpass, fc(x))")


# ---- Comb / Allpass -------------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("D", [7, 4800, 20_000])
def test_comb(x64, sizes, D):
    """D = 20 000 is longer than most pushes: most classes have no frame in a push and copy their entry of the record"""
    check(lambda s: so.Comb(s, D, 0.6, feedforward=0.25), x64, sizes, lambda: comb_ref(x64, D, 1.0, 0.25, 0.6), f"Comb D={D}")


@BOTH
def test_allpass(x64, sizes):
    check(lambda s: so.Allpass(s, 113, 0.5), x64, sizes, lambda: comb_ref(x64, 113, -0.5, 1.0, 0.5), "Allpass")


@BOTH
def test_comb_float32_input(x32, sizes):
    check(lambda s: so.Comb(s, 4800, 0.6), x32, sizes, lambda: comb_ref(x32, 4800, 1.0, 0.0, 0.6), "Comb of Float32")


def test_comb_pushes_of_one_frame(x64):
    x = x64[:300]
    check(lambda s: so.Comb(s, 7, 0.6, feedforward=0.25), x, [1] * 300, lambda: comb_ref(x, 7, 1.0, 0.25, 0.6), "Comb, one frame a push",
          head_leaves=False)


# ---- the moving windows ---------------------------------------------------------------------------------------------------
@BOTH
def test_movingmax_trailing_and_centred(x64, sizes):
    check(lambda s: so.MovingMax(s, 481), x64, sizes, lambda: moving_ref(x64, 480, 0), "MovingMax trailing")
    check(lambda s: so.MovingMax(s, 481, center=True), x64, sizes, lambda: moving_ref(x64, 240, 240), "MovingMax centred")
    check(lambda s: so.MovingMin(s, 481, center=True), x64, sizes, lambda: moving_ref(x64, 240, 240, True), "MovingMin centred")


@BOTH
def test_movingmax_float32(x32, sizes):
    check(lambda s: so.MovingMax(s, 481, center=True), x32, sizes, lambda: moving_ref(x32, 240, 240), "MovingMax of Float32")


@BOTH
def test_movingmax_long_form(x64, sizes):
    check(lambda s: so.MovingMax(s, 5000), x64, sizes, lambda: moving_ref(x64, 4999, 0), "MovingMax w=5000")


@BOTH
def test_movingmean_centred(x64, sizes):
    check(lambda s: so.MovingMean(s, 481, center=True), x64, sizes, lambda: movingsum_ref(x64, 240, 240, 1), "MovingMean centred")


@BOTH
def test_movingrms_long_form(x64, sizes):
    check(lambda s: so.MovingRMS(s, 3001), x64, sizes, lambda: movingsum_ref(x64, 3000, 0, 2), "MovingRMS w=3001")


@BOTH
def test_movingmedian_centred(x64, sizes):
    check(lambda s: so.MovingMedian(s, 5, center=True), x64, sizes, lambda: movrank_ref(x64, 2, 2, 0.5), "MovingMedian w=5")


@BOTH
def test_movingquantile(x64, sizes):
    check(lambda s: so.MovingQuantile(s, 1025, 0.1), x64, sizes, lambda: movrank_ref(x64, 1024, 0, 0.1), "MovingQuantile(1025, 0.1)")


def test_outputs_held_back_by_ahead_arrive_with_finish(x64):
    got, counts = check(lambda s: so.MovingMax(s, 481, center=True), x64, SIZES_A, what="MovingMax centred")
    assert sum(counts) == N and counts[0] == SIZES_A[0] - 240 - 1  # (a push's last frame may still be the signal's last: one more waits)
    assert counts[-1] == 240 + 1, counts  # what the look-ahead held back


# ---- composite trees ------------------------------------------------------------------------------------------------------
def _limiter(s, w=241, tau=2 * so.ms):
    mag = so.OperateOn(so.elementwise(lambda v: np.abs(v)), s)
    env = so.Smooth(so.MovingMean(so.MovingMax(mag, w, center=True), w, center=True), tau)
    return so.OperateOn(so.elementwise(lambda v, e: v / np.maximum(1.0, e)), s, env)


@BOTH
def test_look_ahead_limiter(x64, sizes):
    got, _ = check(_limiter, 3.0 * x64, sizes, what="limiter")
    assert np.isfinite(got).all()


@BOTH
def test_nested_cumsum(x64, sizes):
    check(lambda s: so.Cumsum(so.Cumsum(s)), x64, sizes, lambda: cumsum_ref(cumsum_ref(x64)), "Cumsum(Cumsum)")


@BOTH
def test_mix_of_two_carrying_nodes(x64, sizes):
    check(lambda s: so.Mix(so.Smooth(s, 5 * so.ms), so.Comb(s, 4800, 0.6)), x64, sizes, what="Mix(Smooth, Comb)")


@BOTH
def test_cumsum_under_toframerate(x64, sizes):
    check(lambda s: so.Cumsum(s) | so.ToFramerate(15 * so.kHz), x64, sizes, what="Cumsum | ToFramerate")


@BOTH
@pytest.mark.parametrize("node", ["recur2", "recur2-near-one", "comb"])
def test_a_filt_above_a_carrying_node(x64, sizes, node):
    """An IIR `Filt` reads a warm start in front of every block, so the node under it is read from before its newest
    checkpoint: the planner refuses that plan by node and the push is planned again from the record before (asserted to
    have happened; under a `Comb`, whose checkpoint is the end of the push, at every push, and the record that serves is
    the one of two pushes ago).  A streamed `Filt` is itself not bit-exact against the whole sink -- every push starts it from rest a
    decay time before the block (tests/test_gpu_windows.py holds it to 1e-11) -- so the bits are
    asserted against a second stream that pushes the node's precomputed whole-sink output through the same `Filt` in the
    same sizes: both plan the `Filt` alike, and any difference is the resumed node's.  The 1e-11 against the whole sink is
    asserted besides."""
    under = {"recur2": lambda s: so.Recur2(1.2, -0.72, s), "recur2-near-one": lambda s: so.Recur2(1.999, -0.999001, s),
             "comb": lambda s: so.Comb(s, 113, 0.6, feedforward=0.25)}[node]
    filt = lambda s: s | so.Filt(so.Lowpass, 2 * so.kHz)  # noqa: E731
    pipe = lambda s: filt(under(s))  # noqa: E731
    assert sum(sizes) == N
    bs = so.BlockStream(pipe, FS, nch=NCH, history=HISTORY)
    outs, pos = [], 0
    for m in sizes:
        outs.append(bs.push(dev(x64[pos:pos + m])).cpu().numpy())
        pos += m
    got = np.concatenate(outs + [bs.finish().cpu().numpy()], axis=0)
    assert bs.start > 0
    if node == "comb" or sizes is SIZES_A:  # (a scan falls back only where the warm start crosses its last chunk boundary: the one-frame pushes)
        assert bs.replanned > 0
    mid = sunk(under, x64)  # the node over the whole input: bit for bit what the cases above hold the stream to
    ref, _ = streamed(filt, mid, sizes)
    bit_equal(got, ref, f"{node} | Filt: the stream against Filt streamed over the node's whole-sink output")
    want = whole(pipe, x64)
    assert got.shape == want.shape and got.dtype == want.dtype and np.isfinite(got).all()
    e = relerr(got, want)
    print(f"{node} | Filt, stream against the whole sink: {e:.3e}")
    assert e <= 1e-11


@BOTH
def test_cumsum_over_and_under_after(x64, sizes):
    check(lambda s: s | so.After(100 * so.frames) | so.Cumsum, x64, sizes, lambda: cumsum_ref(x64[100:]), "After | Cumsum")
    check(lambda s: so.Cumsum(s) | so.After(100 * so.frames), x64, sizes, lambda: cumsum_ref(x64)[100:], "Cumsum | After")


# ---- the resumed plan itself ------------------------------------------------------------------------------------------------
def test_a_resumed_plan_executed_twice_gives_the_same_bytes(x64):
    """one plan with a hand-made carry: Cumsum resumed at chunk 2 from the running total that enters it, read from frame
    40 000 on; two executes give the same result and the same carry-out, and the carry-in record is not written"""
    import torch

    ref = cumsum_ref(x64)
    r, first = 2 * CHUNK, 40_000
    cin = dev(ref[r - 1].copy())  # the running total behind chunk 1, one Float64 a channel
    cin0 = cin.clone()
    cout = torch.full((NCH,), np.nan, dtype=torch.float64, device="cuda")
    node = so.Cumsum(so.Signal(dev(x64).t().contiguous().t(), FS))
    node.carry = (r, cin.data_ptr(), cout.data_ptr())
    tree = node | so.After(first * so.frames)
    outs, couts = [], []
    plan = Plan(tree, (N - first, NCH), np.float64, (1, N - first), True)
    try:
        (stands,) = plan.carried()
        assert stands[0] is node and stands[1:] == ((N - 1) // CHUNK * CHUNK, N)
        for _ in range(2):
            res = torch.empty((NCH, N - first), dtype=torch.float64, device="cuda")
            cout.fill_(np.nan)
            plan.execute(res.data_ptr())
            plan.check()
            outs.append(res.t().cpu().numpy())
            couts.append(cout.cpu().numpy())
    finally:
        plan.close()
    bit_equal(outs[0], ref[first:], "the resumed plan against the definition")
    assert outs[0].tobytes() == outs[1].tobytes() and couts[0].tobytes() == couts[1].tobytes()
    bit_equal(couts[0], ref[(N - 1) // CHUNK * CHUNK - 1], "the carry-out: the total that enters the last chunk")
    assert torch.equal(cin, cin0)


def test_the_planner_refuses_a_bad_resume(x64):
    import torch

    rec = torch.zeros((NCH,), dtype=torch.float64, device="cuda")
    x = so.Signal(dev(x64).t().contiguous().t(), FS)

    def create(carry, after=40_000, make=so.Cumsum):
        node = make(x)
        node.carry = carry
        Plan(node | so.After(after * so.frames), (N - after, NCH), np.float64, (1, N - after), True).close()

    with pytest.raises(so.ErrorException, match="not a multiple of its chunk of 16384"):
        create((1000, rec.data_ptr(), 0))
    with pytest.raises(so.ErrorException, match="without a carry-in record"):
        create((CHUNK, 0, 0))
    with pytest.raises(so.ErrorException, match="beyond the 70001 frames"):
        create((5 * CHUNK, rec.data_ptr(), 0))
    with pytest.raises(so.ErrorException, match="before its resume frame 32768") as e:
        create((2 * CHUNK, rec.data_ptr(), 0), after=20_000)
    assert e.value.resume_node >= 0 and dict(e.value.lowered.carry_nodes)[e.value.resume_node].carry[0] == 2 * CHUNK
    with pytest.raises(so.ErrorException, match="beyond the 70001 frames") as e:  # any other refusal names no node
        create((5 * CHUNK, rec.data_ptr(), 0))
    assert e.value.resume_node == -1
    with pytest.raises(so.ErrorException, match="not its carry-in record"):
        create((CHUNK, rec.data_ptr(), rec.data_ptr()))
    create((0, 0, 0))  # all three zero: the node as ever


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_a_history_too_short_for_the_resume_point_is_refused(x64):
    """pushes of 16000 frames under a history of 8000: the fourth push resumes at frame 32768, and the tail kept starts at
    40000 -- the planner's own refusal, and no output for that push"""
    bs = so.BlockStream(lambda s: so.Cumsum(s), FS, nch=NCH, history=8000)
    for k in range(3):
        assert bs.push(dev(x64[16000 * k:16000 * (k + 1)])).shape[0] == 16000 - (k == 0)
    with pytest.raises(so.ErrorException, match="no longer resident .*raise the stream's history"):
        bs.push(dev(x64[48000:64000]))
    assert bs.emitted == 48000 - 1


def test_a_pipeline_whose_carrying_nodes_change_is_refused(x64):
    delays = iter([7, 7, 9])
    bs = so.BlockStream(lambda s: so.Comb(s, next(delays), 0.5), FS, nch=NCH)
    bs.push(dev(x64[:1000]))
    bs.push(dev(x64[1000:2000]))
    with pytest.raises(so.ErrorException, match="BlockStream: the pipeline's nodes that carry state changed between pushes"):
        bs.push(dev(x64[2000:3000]))
    kinds = iter([so.Cumsum, lambda s: so.Recur(0.5, s)])
    bs = so.BlockStream(lambda s: next(kinds)(s), FS, nch=NCH)
    bs.push(dev(x64[:1000]))
    with pytest.raises(so.ErrorException, match="changed between pushes"):
        bs.push(dev(x64[1000:2000]))
    kinds = iter([lambda s: s | so.Amplify(0.5), so.Cumsum])  # none at the first push, one later: refused as well
    bs = so.BlockStream(lambda s: next(kinds)(s), FS, nch=NCH)
    bs.push(dev(x64[:1000]))
    with pytest.raises(so.ErrorException, match="changed between pushes"):
        bs.push(dev(x64[1000:2000]))


def test_sampleat_and_delay_are_refused_by_name_at_the_first_push(x64):
    ramp = lambda s: so.OperateOn(so.elementwise(lambda v: 0.5 * np.abs(v)), so.ToChannels(s, 1))  # noqa: E731
    for pipe in (lambda s: so.SampleAt(s, ramp(s), relative=True), lambda s: so.Delay(s, ramp(s)), lambda s: so.Delay(s, 3)):
        bs = so.BlockStream(pipe, FS, nch=NCH)
        with pytest.raises(so.ErrorException, match="^BlockStream: SampleAt .*; not streamable$"):
            bs.push(dev(x64[:1000]))
