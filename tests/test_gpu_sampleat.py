"""`SampleAt(x, pos)` and `Delay(x, d)` on the device (include/sigops.h SO_NODE_SAMPLEAT; csrc/k_sample_at.hip), through the
C-ABI: bit for bit against the two NumPy expressions that define the node (tests/sampleat_ref.py sampleat_np) and against
the restatement of the device's formula -- no tolerance, the arithmetic is specified operation by operation.  The
reference functions and their inputs are held to each other without a GPU in tests/test_sampleat_host.py."""
import ctypes as C
from itertools import islice

import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import _capi as K
from sigops_amd import lowering as LW
from sigops_amd import signals as S
from sigops_amd.engine import Plan
from oracle_bridge import relerr
from sampleat_ref import N_CHANNELS, N_RESULT, N_TABLE, positions, same_bits, sampleat_np, sampleat_restated, table

pytestmark = pytest.mark.gpu
FS = 10 * so.kHz
MODES = ({}, {"left": -7.5, "right": np.inf}, {"wrap": True}, {"relative": True}, {"relative": True, "wrap": True})


def bit_equal(got, want, what=""):
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} samples differ, first at {np.argwhere(bad)[0]}"
    assert same_bits(got, want), f"{what}: a zero of the other sign"


def check(x, pos, what="", **kw):
    """the sink of SampleAt(x, pos) against the definition and the restatement"""
    got = so.sink(so.SampleAt(so.Signal(x, FS), so.Signal(pos, FS), **kw), so.Array)
    bit_equal(got, sampleat_np(x, pos, **kw), f"{what} {kw}")
    assert same_bits(got, sampleat_restated(x, pos, **kw))
    return got


def dev(a):
    """a planar device tensor [frames x channels]"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t()


# ---- 1. planted positions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", N_CHANNELS)
@pytest.mark.parametrize("N", N_TABLE)
def test_planted_positions_equal_numpy_bit_for_bit(N, Cn):
    x = table(N, Cn)
    for L in N_RESULT:
        pos = positions(N, L)
        for kw in MODES:
            check(x, pos, f"N={N} L={L} C={Cn}", **kw)


@pytest.mark.parametrize("N", N_TABLE)
def test_non_finite_tables_take_numpys_fall_backs(N):
    for Cn in (1, 3):
        x = table(N, Cn, nonfinite=True)
        pos = positions(N, 1001, Cn)
        for kw in ({}, {"wrap": True}, {"left": np.nan, "right": -np.inf}):
            check(x, pos, f"non-finite N={N} C={Cn}", **kw)


@pytest.mark.parametrize("N", [1, 3, 65, 4097])
def test_float32_tables_and_float32_positions(N):
    x = table(N, 3, np.float32, nonfinite=True)
    pos = positions(N, 1001, 1, np.float32)
    got = check(x, pos, "Float32", left=0.25)
    assert got.dtype == np.float64
    check(table(N, 2, np.float32), pos, "Float32 wrap", wrap=True)
    check(table(N, 2, np.float32), positions(N, 1001, 2), "Float32 table, Float64 positions", relative=True)
    check(table(N, 2), positions(N, 1001, 2, np.float32), "Float64 table, Float32 positions")


# ---- 2. broadcast and modes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [2, 3, 8])
def test_a_mono_pos_is_broadcast_and_a_pos_per_channel_is_not(Cn):
    x = table(65, Cn)
    mono = positions(65, 1001)
    a = check(x, mono, "mono")
    b = check(x, np.asfortranarray(np.repeat(mono, Cn, axis=1)), "repeated")
    bit_equal(a, b, "mono against repeated")
    per = positions(65, 1001, Cn)
    c = check(x, per, "per channel", left=3.0, right=-4.0)
    assert not np.array_equal(c[:, 0], sampleat_np(x, per[:, 1:2], left=3.0, right=-4.0)[:, 0])  # (each channel reads its own column)


def test_wrap_reads_a_wavetable_at_negative_positions_and_beyond_the_table():
    for N in (1, 2, 64, 65):
        x = table(N, 2)
        p = np.concatenate([np.linspace(-3.0 * N - 0.75, 4.0 * N + 0.25, 997), [-float(N), float(N), -1.0, N - 0.5, -1e-20, 1e17]]).reshape(-1, 1)
        got = check(x, np.asfortranarray(p), f"wrap N={N}", wrap=True, left=5.0, right=6.0)  # (left / right ignored, as NumPy does)
        bit_equal(got[-6:-4], x[[0, 0]], "whole periods")
        bit_equal(got[-4:-3], x[[N - 1]], "one frame back")


def test_delays():
    x = table(65, 3)
    xs = so.Signal(x, FS)
    bit_equal(so.sink(so.Delay(xs, 0), so.Array), x, "Delay(x, 0) is x")
    bit_equal(so.sink(so.SampleAt(xs, so.Signal(np.zeros((65, 1)), FS), relative=True), so.Array), x, "a zero relative position")
    for k in (1, 63, 64, 65):
        want = np.zeros_like(x)
        want[k:] = x[:max(65 - k, 0)]
        bit_equal(so.sink(so.Delay(xs, k), so.Array), want, f"Delay(x, {k})")
        bit_equal(so.sink(xs | so.Delay(k * so.frames), so.Array), want, f"Delay(x, {k} frames)")
    # a Float32 signal delayed is its values, widened
    x32 = table(64, 2, np.float32)
    want = np.zeros((64, 2), order="F")
    want[1:] = x32[:-1]
    bit_equal(so.sink(so.Delay(so.Signal(x32, FS), 1), so.Array), want, "Float32")
    # a fractional constant delay, as a number, a time and a signal
    d = 2.375
    want = sampleat_np(x, np.full((65, 1), -d), relative=True)
    bit_equal(so.sink(so.Delay(xs, d), so.Array), want, "fractional")
    bit_equal(so.sink(so.Delay(xs, 0.2375 * so.ms), so.Array), sampleat_np(x, np.full((65, 1), -(0.2375 / 1000 * 10_000.0)), relative=True), "a time")
    bit_equal(so.sink(so.Delay(xs, so.Signal(np.full((65, 1), d), FS)), so.Array), want, "a signal")
    # a delay signal shorter than x: the result is extended with zeros to the frames of x
    short = so.sink(so.Delay(xs, so.Signal(np.full((40, 1), d), FS)), so.Array)
    bit_equal(short, np.asfortranarray(np.vstack([want[:40], np.zeros((25, 3))])), "extended")
    # a vibrato: a slowly moving delay
    lfo = np.asfortranarray((3.0 + 2.5 * np.sin(np.arange(65) / 9.0)).reshape(-1, 1))
    bit_equal(so.sink(so.Delay(xs, so.Signal(lfo, FS)), so.Array), sampleat_np(x, -lfo, relative=True), "vibrato")


def test_an_odd_window_base_and_odd_stream_blocks():
    x = table(65, 3)
    pos = positions(65, 1001, 3)
    for kw in ({}, {"relative": True}, {"wrap": True}):
        tree = so.SampleAt(so.Signal(x, FS), so.Signal(pos, FS), **kw)
        whole = sampleat_np(x, pos, **kw)
        bit_equal(so.sink(tree | so.After(1 * so.frames), so.Array), whole[1:], f"After(1 frame) {kw}")
        bit_equal(np.vstack([b for b in so.stream(tree, 333, so.Array)]), whole, f"blocks of 333 {kw}")
        bit_equal(np.vstack(list(islice(so.stream(tree | so.After(1 * so.frames), 7, so.Array), 30))), whole[1:211], f"blocks of 7 {kw}")


# ---- 3. computed operands ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [False, True])
def test_a_filtered_table(batch, monkeypatch):
    if batch:
        monkeypatch.setenv("SIGOPS_RSOS_BATCH", "1")
    raw = table(4097, 2)
    pos = positions(4097, 1001, 2)
    filtered = so.Signal(raw, FS) | so.Filt(so.Lowpass, 1 * so.kHz)
    xf = so.sink(filtered, so.Array)  # the table, sunk separately
    assert np.isfinite(xf).all() and np.ptp(xf) > 0.5
    for kw in ({}, {"relative": True, "wrap": True}):
        got = so.sink(so.SampleAt(filtered, so.Signal(pos, FS), **kw), so.Array)
        bit_equal(got, sampleat_np(xf, pos, **kw), f"Filt(Lowpass) as the table {kw} batch={batch}")
    # two filtered tables in one tree (members of ONE launch where the batched launch is forced), each read by its own
    # SampleAt: the stage must run behind the launch that writes its table.  The tables are sunk separately as a pair too
    # -- two filters of one plan share their launches, and the batched one-pass form rounds differently from a filter
    # that has the plan to itself; the filter's own accuracy is tests/test_gpu_rsos_batch.py's subject, not this test's
    other = so.Signal(table(4097, 2, seed=1), FS) | so.Filt(so.Lowpass, 2 * so.kHz)
    pair = so.sink(so.AddChannel(filtered, other), so.Array)
    xf2, xo2 = np.asfortranarray(pair[:, :2]), np.asfortranarray(pair[:, 2:])
    assert np.isfinite(pair).all() and np.ptp(xf2) > 0.5 and np.ptp(xo2) > 0.5
    got = so.sink(so.Mix(so.SampleAt(filtered, so.Signal(pos, FS)), so.SampleAt(other, so.Signal(pos, FS), wrap=True)), so.Array)
    bit_equal(got, np.asfortranarray(sampleat_np(xf2, pos) + sampleat_np(xo2, pos, wrap=True)), f"two filtered tables batch={batch}")


def test_a_traced_position_formula():
    x = table(65, 2)
    fn = so.elementwise(lambda t: 32.0 + 40.0 * np.sin(t * 700.0))
    psig = so.Signal(fn, FS) | so.Until(1001 * so.frames)
    pos = so.sink(psig, so.Array)  # the positions, sunk separately
    assert pos.min() < -2 and pos.max() > 66
    for kw in ({}, {"wrap": True}, {"relative": True}):
        bit_equal(so.sink(so.SampleAt(so.Signal(x, FS), psig, **kw), so.Array), sampleat_np(x, pos, **kw), f"Signal(elementwise) as pos {kw}")
    # an infinite pos: sunk through Until
    got = so.sink(so.SampleAt(so.Signal(x, FS), so.Signal(fn, FS)) | so.Until(1001 * so.frames), so.Array)
    bit_equal(got, sampleat_np(x, pos), "an infinite pos under Until")
    # a map of an array as pos
    base = positions(65, 1001)
    got = so.sink(so.SampleAt(so.Signal(x, FS), so.Amplify(so.Signal(base, FS), 0.5)), so.Array)
    bit_equal(got, sampleat_np(x, base * 0.5), "Amplify(pos, 0.5)")


# ---- 4. windows and streams ----------------------------------------------------------------------------------------------
def test_windows_and_streams_equal_the_whole_sink():
    x = table(4097, 2)
    pos = positions(4097, 1001, 2)
    for kw in ({}, {"relative": True}):
        tree = so.SampleAt(so.Signal(x, FS), so.Signal(pos, FS), **kw)
        whole = so.sink(tree, so.Array)
        bit_equal(whole, sampleat_np(x, pos, **kw))
        bit_equal(so.sink(tree | so.After(130 * so.frames) | so.Until(64 * so.frames), so.Array), whole[130:194], "After | Until")
        bit_equal(so.sink(tree | so.Until(65 * so.frames), so.Array), whole[:65], "Until")
        bit_equal(so.sink(tree | so.After(1000 * so.frames), so.Array), whole[1000:], "After")
        bit_equal(np.vstack([b for b in so.stream(tree, 64, so.Array)]), whole, "blocks of 64")
        # a formula as pos: the window computes only its own frames, with absolute frame numbers
        f = so.SampleAt(so.Signal(x, FS), so.Signal(so.elementwise(lambda t: t * 3000.0), FS), **kw) | so.Until(1001 * so.frames)
        fw = so.sink(f, so.Array)
        bit_equal(so.sink(f | so.After(333 * so.frames) | so.Until(65 * so.frames), so.Array), fw[333:398], "a formula, windowed")
        bit_equal(np.vstack([b for b in so.stream(f, 65, so.Array)]), fw, "a formula, streamed")


# ---- 5. leaves and plan reuse --------------------------------------------------------------------------------------------
def test_device_leaves_host_leaves_and_a_device_result():
    for N, L, Cn in ((65, 1001, 3), (4097, 65, 8), (3, 63, 2)):
        x, pos = table(N, Cn), positions(N, L, Cn)
        for kw in ({}, {"relative": True, "wrap": True}):
            want = sampleat_np(x, pos, **kw)
            got, fs = so.sink(so.SampleAt(so.Signal(dev(x), FS), so.Signal(dev(pos), FS), **kw), "torch")
            assert fs == 10_000.0 and got.is_cuda
            bit_equal(got.cpu().numpy(), np.ascontiguousarray(want), "device leaves, device result")
            bit_equal(so.sink(so.SampleAt(so.Signal(dev(x), FS), so.Signal(pos, FS), **kw), so.Array), want, "device table, host pos")
            got, _ = so.sink(so.SampleAt(so.Signal(x, FS), so.Signal(dev(pos), FS), **kw), "torch")
            bit_equal(got.cpu().numpy(), np.ascontiguousarray(want), "host table, device pos")
    # an interleaved host table (frames x channels, C order) is read where it lies too
    xi = np.ascontiguousarray(table(65, 3))
    bit_equal(so.sink(so.SampleAt(so.Signal(xi, FS), so.Signal(positions(65, 1001), FS)), so.Array), sampleat_np(xi, positions(65, 1001)), "interleaved")


def test_a_plan_is_reused_after_set_array_on_x_and_on_pos():
    import torch

    xs = [table(65, 2, seed=k) for k in range(3)]
    ps = [positions(65, 1001, 2, seed=k) for k in range(3)]
    res = np.zeros((1001, 2), order="F")
    p = Plan(so.SampleAt(so.Signal(xs[0], FS), so.Signal(ps[0], FS), relative=True), res.shape, res.dtype, (1, res.shape[0]), False)
    scratch = p.stats()["scratch_bytes"]
    for kx, kp in ((0, 0), (1, 0), (1, 1), (2, 2), (0, 2)):
        p.set_array(0, xs[kx])
        p.set_array(1, ps[kp])
        p.execute(res.ctypes.data)
        bit_equal(res, sampleat_np(xs[kx], ps[kp], relative=True), f"host leaves x{kx} pos{kp}")
        assert p.stats()["scratch_bytes"] == scratch
    p.close()
    # device leaves, a device result: nothing is copied, and no buffer but the result is written
    dx, dp = [dev(a) for a in xs], [dev(a) for a in ps]
    out = torch.empty((2, 1001), dtype=torch.float64, device="cuda").t()
    p = Plan(so.SampleAt(so.Signal(dx[0], FS), so.Signal(dp[0], FS), wrap=True), (1001, 2), np.float64, (1, 1001), True)
    for kx, kp in ((0, 0), (0, 0), (0, 0), (1, 0), (1, 1), (2, 2), (2, 2), (2, 2)):
        p.set_array(0, dx[kx])
        p.set_array(1, dp[kp])
        p.execute(out.data_ptr())
        p.check()
        bit_equal(out.cpu().numpy(), np.ascontiguousarray(sampleat_np(xs[kx], ps[kp], wrap=True)), f"device leaves x{kx} pos{kp}")
        s = p.stats()
        assert s["h2d_bytes"] == 0 and s["d2h_bytes"] == 0 and s["scratch_bytes"] <= 4096  # the table is read in place: no copy of it
    p.close()


# ---- 6. consumers ------------------------------------------------------------------------------------------------------
def close(got, want, what):
    """the bound tests/test_gpu_elementwise_interp.py holds a filter behind a materialised buffer to"""
    assert got.shape == want.shape
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    e = relerr(got, want)
    print(f"worst {what}: {e:.3e}")
    assert e <= 1e-12, f"{what}: {e:.3e}"


def test_a_filter_and_a_resampler_behind_it():
    x = table(4097, 2)
    pos = np.asfortranarray(np.linspace(0.0, 4096.0, 30_000).reshape(-1, 1) + 3.0 * np.sin(np.arange(30_000) / 50.0).reshape(-1, 1))
    tree = so.SampleAt(so.Signal(x, FS), so.Signal(pos, FS))
    mid = so.sink(tree, so.Array)  # the SampleAt result, sunk separately
    bit_equal(mid, sampleat_np(x, pos))
    for name, tail in (("Filt(Highpass)", lambda t: t | so.Filt(so.Highpass, 1 * so.kHz)),
                       ("ToFramerate", lambda t: t | so.ToFramerate(12 * so.kHz)),
                       ("Normpower", lambda t: t | so.Normpower),
                       ("a map", lambda t: so.Amplify(t, 0.25) | so.ToEltype(np.float32))):
        got = so.sink(tail(tree), so.Array)
        want = so.sink(tail(so.Signal(mid, FS)), so.Array)
        assert got.dtype == want.dtype and np.ptp(want) > 0.1
        close(got, want, f"SampleAt | {name}")


# ---- 7. refusals that need the engine --------------------------------------------------------------------------------
def _create(lw, nframes, nch):
    out = K.so_out_desc_t(dtype=K.SO_F64, nch=nch, nframes=nframes, frame_stride=1, chan_stride=nframes, is_device=0)
    plan = C.c_void_p()
    st = K.lib().so_plan_create(lw.nodes, lw.n, lw.root, C.byref(out), 0, C.byref(plan))
    if plan.value:
        K.lib().so_plan_destroy(plan)
    return st, K.last_error() if st else ""


def test_malformed_nodes_are_refused():
    x, pos = so.Signal(table(65, 3), FS), so.Signal(positions(65, 64), FS)
    lw = LW.lower(so.SampleAt(x, pos))
    assert _create(lw, 64, 3)[0] == 0  # the well-formed node
    node = lw.root
    assert lw.nodes[node].kind == K.NODE_SAMPLEAT
    lw.nodes[node].n_children = 1
    st, err = _create(lw, 64, 3)
    assert st == -1 and f"node {node}" in err and "SampleAt" in err and "two children" in err, err
    three = (C.c_int32 * 3)(0, 1, 0)
    lw.nodes[node].children = C.cast(three, C.POINTER(C.c_int32))
    lw.nodes[node].n_children = 3
    st, err = _create(lw, 64, 3)
    assert st == -1 and "SampleAt" in err and "two children" in err, err
    lw.nodes[node].n_children = 2
    lw.nodes[node].i0 = 4
    st, err = _create(lw, 64, 3)
    assert st == -1 and "unknown flags" in err, err
    # a pos of two channels against a table of three (the host refuses to build it: the node is made by hand)
    bad = S.SampleAtSignal(x, so.Signal(positions(65, 64, 2), FS))
    st, err = _create(LW.lower(bad), 64, 3)
    assert st == -1 and "SampleAt" in err and "2 channels" in err, err
    # an infinite table and an empty one never reach a kernel either
    st, err = _create(LW.lower(S.SampleAtSignal(so.Signal(np.sin, FS, ω=5 * so.Hz), pos)), 64, 1)
    assert st == -2 and "finite length" in err, err
    st, err = _create(LW.lower(S.SampleAtSignal(so.Signal(np.zeros((0, 3)), FS), pos)), 64, 3)
    assert st == -2 and "at least one frame" in err, err
