"""Counter-based device noise on the GPU (`Signal(randn, rng=so.DeviceRNG(seed, stream))`, include/sigops.h
SO_FN_RANDN, csrc/krand.h): values against the NumPy restatement (philox_ref.py), the bit-equalities that follow from
"frame i is a function of (seed, stream, i)" -- blocks, windows, shards, repeated executes, the fill kernel against the
expression form, hipRTC against the interpreter -- pipelines against the CPU oracle (which is handed the samples as an
array leaf: it does not know the generator), and the distribution of the samples.

Measured on MI355X (this file's own run): see DESIGN.md, "Device noise"."""
import os

import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import sharding
from oracle_bridge import oracle_sink, relerr

import philox_ref as R

pytestmark = pytest.mark.gpu

FS = 44.1 * so.kHz
SEEDS = [0, 2024, 0xDEADBEEFCAFEF00D]
STREAMS = [0, 1, (1 << 32) + 7]


def F(a):
    return np.asfortranarray(a)


class env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def noise(seed=2024, stream=0, fs=FS):
    return so.Signal(so.randn, fs, rng=so.DeviceRNG(seed, stream))


def steps_of(x, dtype=np.float64):
    n, nch = so.nframes(x), so.nchannels(x)
    p = so.Plan(so.ToChannels(x, nch), (n, nch), dtype, (1, n), False)
    names = [s["name"] for s in p.steps()]
    p.close()
    return names


def within_ulps(d, ref, k=8):
    err = np.abs(d - ref) / np.spacing(np.abs(ref))
    print("worst error: %.3f ulp" % err.max())
    return np.isfinite(d).all() and err.max() <= k


# ---- values ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("stream", STREAMS)
def test_values_match_the_restatement(seed, stream):
    n = 1 << 20
    x = noise(seed, stream) | so.Until(n * so.frames)
    assert steps_of(x) == ["k_randn_fill"]
    got = so.sink(x, so.Array)
    assert got.shape == (n, 1) and got.dtype == np.float64
    assert within_ulps(got[:, 0], R.randn(seed, stream, 0, n))


@pytest.mark.parametrize("offset", [(1 << 31) - 7, (1 << 32) + 1, (1 << 33) + 12345])
@pytest.mark.parametrize("seed, stream", [(0, 0), (2024, 1), (0xDEADBEEFCAFEF00D, (1 << 32) + 7)])
def test_windows_far_into_the_signal(offset, seed, stream):
    """the pair index's high counter word"""
    x = noise(seed, stream) | so.After(offset * so.frames) | so.Until(4096 * so.frames)
    got = so.sink(x, so.Array)[:, 0]
    assert within_ulps(got, R.randn(seed, stream, offset, 4096))
    # ... and through the expression form
    y = so.Mix(x, so.Signal(F(np.zeros((4096, 1))), FS))
    assert "k_randn_fill" not in steps_of(y)
    assert np.all(so.sink(y, so.Array)[:, 0] == got)


# ---- bit-equalities -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocksize, n", [(1, 301), (333, 10_000), (65_537, 300_000)])
def test_stream_blocks_are_the_whole_sink(blocksize, n):
    x = noise(7, 3) | so.Until(n * so.frames)
    whole = so.sink(x, so.Array)
    blocks = list(so.stream(x, blocksize, so.Array))
    assert all(b.shape[0] == blocksize for b in blocks[:-1])
    assert np.array_equal(np.concatenate(blocks, axis=0), whole)


@pytest.mark.parametrize("k", [1, 2, 255, 256, 511, 100_001, 100_002])
def test_after_windows_are_slices(k):
    n = 200_000
    whole = so.sink(noise(11, 5) | so.Until(n * so.frames), so.Array)
    for m in (1, 2, 513, n - k):
        part = so.sink(noise(11, 5) | so.After(k * so.frames) | so.Until(m * so.frames), so.Array)
        assert np.array_equal(part, whole[k:k + m]), (k, m)


def _expr_tree(n, seed=2024, stream=0, nch=1):
    """the leaf through the interpreter / hipRTC: a Mix with an array of zeros is no fill step"""
    return so.Mix(noise(seed, stream) | so.Until(n * so.frames), so.Signal(F(np.zeros((n, nch))), FS))


def test_fill_form_equals_expression_form_and_hiprtc_equals_interpreter():
    n = 300_001
    fill = so.sink(noise() | so.Until(n * so.frames), so.Array)
    with env(SIGOPS_RTC="0"):
        assert steps_of(_expr_tree(n)) == ["k_pointwise"]
        interp = so.sink(_expr_tree(n), so.Array)
    with env(SIGOPS_RTC="1"):
        assert steps_of(_expr_tree(n)) == ["k_pointwise_rtc"]
        rtc = so.sink(_expr_tree(n), so.Array)
    with env(SIGOPS_RTC=None):
        default = so.sink(_expr_tree(n), so.Array)
    with env(SIGOPS_RANDN_NOFILL="1", SIGOPS_RTC="0"):
        assert steps_of(noise() | so.Until(n * so.frames)) == ["k_pointwise"]
        nofill = so.sink(noise() | so.Until(n * so.frames), so.Array)
    # (== and not array_equal on bit patterns: z + 0.0 turns a -0.0 into +0.0)
    assert np.all(interp == fill) and np.all(rtc == fill) and np.all(default == fill)
    assert np.array_equal(nofill.view(np.uint64), fill.view(np.uint64))
    # several channels through the expression form: the value of a frame is the same in all of them
    e8 = so.sink(_expr_tree(50_000, nch=8), so.Array)
    assert e8.shape == (50_000, 8) and np.all(e8 == fill[:50_000])


def test_two_executes_of_one_plan():
    import torch

    n = 100_003
    x = so.ToChannels(noise(3, 1) | so.Until(n * so.frames), 2)
    outs = [torch.empty((2, n), dtype=torch.float64, device="cuda").t() for _ in range(2)]
    p = so.Plan(x, (n, 2), np.float64, (1, n), True)
    try:
        for o in outs:
            p.execute(o.data_ptr())
            p.check()
    finally:
        p.close()
    torch.cuda.synchronize()
    a, b = (o.cpu().numpy() for o in outs)
    assert np.array_equal(a, b) and np.array_equal(a[:, 0], so.sink(noise(3, 1) | so.Until(n * so.frames), so.Array)[:, 0])


def test_tochannels_replicates_the_noise():
    n = 123_457
    one = so.sink(noise(5, 2) | so.Until(n * so.frames), so.Array)
    x = so.ToChannels(noise(5, 2) | so.Until(n * so.frames), 8)
    assert steps_of(x) == ["k_randn_fill"]
    got = so.sink(x, so.Array)
    assert got.shape == (n, 8)
    for c in range(8):
        assert np.array_equal(got[:, c], one[:, 0]), c
    # times a constant: still the fill kernel, one product per sample
    y = so.Amplify(x, 0.3)
    assert steps_of(y) == ["k_randn_fill"]
    assert np.array_equal(so.sink(y, so.Array), got * 0.3)


def test_time_range_shards_are_the_unsharded_sink():
    n = 400_003
    x = so.ToChannels(noise(17, 4) | so.Until(n * so.frames), 2)
    whole = so.sink(x, so.Array)
    parts = []
    for rank in range(4):
        sub, a, cnt = sharding.shard_time(x, rank, 4)
        assert a == sum(p.shape[0] for p in parts)
        parts.append(so.sink(sub, so.Array))
        assert parts[-1].shape[0] == cnt
    assert np.array_equal(np.concatenate(parts, axis=0), whole)


def test_float32_rounds_at_the_store():
    n = 100_001
    x64 = noise(23, 0) | so.Until(n * so.frames)
    x32 = so.ToEltype(x64, np.float32)
    assert steps_of(x32, np.float32) == ["k_randn_fill"]
    a = so.sink(x32, so.Array)
    assert a.dtype == np.float32 and np.array_equal(a, so.sink(x64, so.Array).astype(np.float32))
    # ... also from an odd frame (8-byte stores are not aligned there)
    b = so.sink(so.ToEltype(noise(23, 0) | so.After(3 * so.frames) | so.Until(1001 * so.frames), np.float32), so.Array)
    assert np.array_equal(b, a[3:1004])


# ---- pipelines against the oracle -------------------------------------------------------------------------------------
def _as_array(seed, stream, n, fs=FS):
    """(the device noise leaf cut to n frames, the same samples as an array leaf for the oracle)"""
    dev = noise(seed, stream, fs) | so.Until(n * so.frames)
    return dev, so.Signal(F(so.sink(dev, so.Array)), fs)


def test_noise_rerated_by_toframerate_under_a_filter():
    """`ToFramerate` over a function signal changes the rate the function is evaluated at (reference
    src/reformatting.jl: a SignalFunction is rebuilt, not resampled), through `Filt` and `Until` as well: the noise leaf
    is generated at 48 kHz -- the generator object survives the rebuild -- and the array the oracle gets holds those
    samples."""
    pipe = lambda x: x | so.Until(2 * so.s) | so.Filt(so.Bandstop, 0.5 * so.kHz, 2 * so.kHz) | so.ToFramerate(48 * so.kHz)  # noqa: E731
    dev = pipe(noise(2024, 0))
    assert so.nframes(dev) == 96_000
    arr = so.Signal(F(so.sink(noise(2024, 0, 48 * so.kHz) | so.Until(2 * so.s), so.Array)), 48 * so.kHz)
    names = steps_of(dev)
    assert names[0] == "k_randn_fill" and len(names) >= 2 and not any(nm.startswith("k_pointwise") for nm in names)
    assert all(nm.startswith(("k_sos", "k_rsos")) for nm in names[1:])
    got = so.sink(dev, so.Array)
    want = oracle_sink(pipe(arr))
    print("relerr", relerr(got, want))
    assert got.shape == want.shape and relerr(got, want) < 1e-9


def test_mix_sine_noise_lowpass():
    n = 100_000
    dev, arr = _as_array(2024, 1, n)
    pipe = lambda x: so.Mix(so.Signal(so.sin, ω=1 * so.kHz) | so.Until(n * so.frames), x) | so.Filt(so.Lowpass, 3 * so.kHz)  # noqa: E731
    names = steps_of(pipe(dev))
    assert names[0] in ("k_randn_fill", "k_pointwise", "k_pointwise_rtc") and any(nm.startswith(("k_sos", "k_rsos")) for nm in names)
    got = so.sink(pipe(dev), so.Array)
    want = oracle_sink(pipe(arr))
    print("relerr", relerr(got, want))
    assert relerr(got, want) < 1e-10


def test_amplify_ramp_normpower_append():
    n = 60_000
    dev, arr = _as_array(9, 0, n)
    dev_b, arr_b = _as_array(9, 1, 40_000)
    # tolerances, relative to the largest sample: the ramp's gain is sinpi_c against the oracle's libm sinpi (an ulp or
    # two per sample: 1e-15 leaves a factor of four); Normpower as test_gpu_normpower_array.close64; Append copies
    for name, pipe, tol in [
        ("ramp", lambda x, y: so.Amplify(x, 0.5) | so.RampOn(50 * so.ms), 1e-15),
        ("normpower", lambda x, y: x | so.Normpower, 1e-15),
        ("append", lambda x, y: so.Append(x, y), 0.0),
    ]:
        got = so.sink(pipe(dev, dev_b), so.Array)
        want = oracle_sink(pipe(arr, arr_b))
        err = np.max(np.abs(got - want)) / np.max(np.abs(want))
        print(name, "error", err)
        assert got.shape == want.shape and err <= tol, name


def test_streaming_a_filter_over_noise():
    """block k's warm start re-reads the noise block k-1 emitted: the blocks are the whole sink (false for a host `randn`)"""
    n = 5 * 48_000
    x = noise(31, 0, 48 * so.kHz) | so.Until(n * so.frames) | so.Filt(so.Highpass, 100 * so.Hz)
    whole = so.sink(x, so.Array)
    blocks = list(so.stream(x, 48_000, so.Array))
    assert len(blocks) == 5
    got = np.concatenate(blocks, axis=0)
    print("relerr", relerr(got, whole))
    assert got.shape == whole.shape and relerr(got, whole) <= 1e-12


# ---- distribution -----------------------------------------------------------------------------------------------------
def test_distribution():
    N = 1 << 22
    a = so.sink(noise(2024, 0) | so.Until(N * so.frames), so.Array)[:, 0]
    b = so.sink(noise(2024, 1) | so.Until(N * so.frames), so.Array)[:, 0]
    for z in (a, b):
        assert np.isfinite(z).all() and np.abs(z).max() < 8.58
        m, v = z.mean(), z.var()
        kurt = np.mean((z - m) ** 4) / v ** 2
        stats = {
            "mean": abs(m) * np.sqrt(N),
            "var": abs(v - 1) * np.sqrt(N / 2),
            "kurtosis": abs(kurt - 3) * np.sqrt(N / 24),
            "lag1": abs(np.mean(z[1:] * z[:-1])) * np.sqrt(N),
            "lag2": abs(np.mean(z[2:] * z[:-2])) * np.sqrt(N),
        }
        print(stats)
        assert all(s < 4 for s in stats.values()), stats
    cross = abs(np.mean(a * b)) * np.sqrt(N)
    print("cross", cross)
    assert cross < 4


# ---- further coverage -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("stream", STREAMS)
def test_high_counter_word_for_every_seed_and_stream(seed, stream):
    for offset in ((1 << 31) - 7, (1 << 32) + 1, (1 << 33) + 12345):
        x = noise(seed, stream) | so.After(offset * so.frames) | so.Until(4096 * so.frames)
        assert within_ulps(so.sink(x, so.Array)[:, 0], R.randn(seed, stream, offset, 4096)), offset


@pytest.mark.parametrize("rate", [48 * so.kHz, 44.1 * np.pi / 3 * so.kHz])
def test_noise_under_a_real_resampler(rate):
    """an upsampled `Mix(noise, array)` is resampled as a whole (the map is wrapped, not its children re-rated): the
    resampler's loaders must refuse the noise as a per-frame value and read a materialised buffer"""
    n = 60_000
    ones = so.Signal(F(np.full((n, 2), 0.25)), FS)
    dev, arr = _as_array(9, 0, n)
    pipe = lambda x: so.Mix(x, ones) | so.ToFramerate(rate)  # noqa: E731
    names = steps_of(pipe(dev))
    print(names)
    assert len(names) >= 2 and names[0] in ("k_pointwise_rtc", "k_pointwise") and any("resample" in nm for nm in names[1:])
    got = so.sink(pipe(dev), so.Array)
    want = oracle_sink(pipe(arr))
    print("relerr", relerr(got, want))
    assert got.shape == want.shape and relerr(got, want) < 1e-9


def test_unknown_function_id_is_invalid_and_noise_needs_no_rate():
    import ctypes as C

    from sigops_amd import _capi as K

    lw = so.lower(noise(1, 2) | so.Until(16 * so.frames))
    node = next(i for i in range(lw.n) if lw.nodes[i].kind == K.NODE_FUNC)
    out = K.so_out_desc_t(dtype=K.SO_F64, nch=1, nframes=16, frame_stride=1, chan_stride=16, is_device=0)
    for bad in (4, -1, 99):
        lw.nodes[node].i0 = bad
        plan = C.c_void_p()
        assert K.lib().so_plan_create(lw.nodes, lw.n, lw.root, C.byref(out), 0, C.byref(plan)) == -1, bad  # SO_ERR_INVALID
        assert "unknown function" in K.last_error()
    lw.nodes[node].i0 = K.FN["randn"]
    for i in range(lw.n):
        lw.nodes[i].fs = 0.0  # the values do not depend on a frame rate
    plan = C.c_void_p()
    assert K.lib().so_plan_create(lw.nodes, lw.n, lw.root, C.byref(out), 0, C.byref(plan)) == 0, K.last_error()
    res = np.empty((16, 1), order="F")
    assert K.lib().so_plan_execute(plan, C.c_void_p(res.ctypes.data), None) == 0, K.last_error()
    K.lib().so_plan_destroy(plan)
    assert np.array_equal(res, so.sink(noise(1, 2) | so.Until(16 * so.frames), so.Array))


def test_opaque_closure_over_a_noise_operand():
    """`OperateOn` with a closure the engine cannot trace sinks its operands through the engine: the noise comes from the device"""
    z = so.sink(noise(4, 4) | so.Until(1000 * so.frames), so.Array)
    y = so.OperateOn(lambda a: a * 2.0 + 1.0, noise(4, 4) | so.Until(1000 * so.frames))
    assert np.array_equal(so.sink(y, so.Array), z * 2.0 + 1.0)


def test_float32_product_in_the_fill_kernel_equals_the_expression_form():
    """the fill kernel's rounding flags: Float32 noise times a Float32 constant, and a Float64 product stored as Float32"""
    n = 70_001
    trees = {
        "f32 noise * f32 const": (so.Amplify(so.ToEltype(noise(6, 0) | so.Until(n * so.frames), np.float32), np.float32(0.3)), np.float32),
        "f64 product, f32 result": (so.ToEltype(so.Amplify(noise(6, 0) | so.Until(n * so.frames), 0.3), np.float32), np.float32),
        "f32 noise * f64 const": (so.Amplify(so.ToEltype(noise(6, 0) | so.Until(n * so.frames), np.float32), 0.3), None),
    }
    for name, (tree, dt) in trees.items():
        assert steps_of(tree, dt or np.float64) == ["k_randn_fill"], name
        a = so.sink(tree, so.Array)
        with env(SIGOPS_RANDN_NOFILL="1"):
            assert steps_of(tree, dt or np.float64) != ["k_randn_fill"], name
            b = so.sink(tree, so.Array)
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    z = so.sink(noise(6, 0) | so.Until(n * so.frames), so.Array).astype(np.float32)
    assert np.array_equal(so.sink(trees["f32 noise * f32 const"][0], so.Array), z * np.float32(0.3))
