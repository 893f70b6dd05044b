"""`SampleAt(x, pos, interp="cubic" | "sinc")` and `Delay(..., interp=)` on the device (include/sigops.h SO_NODE_SAMPLEAT,
i1 = 1 | 2; csrc/k_sample_at_fir.hip), through `sink` and through the C-ABI: bit for bit against the definition
(tests/sampleat_interp_ref.py) -- no tolerance, the arithmetic is specified operation by operation.  The definition's two
forms and its inputs are held to each other without a GPU in tests/test_sampleat_interp_host.py."""
import ctypes as C
from itertools import islice

import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import _capi as K
from sigops_amd import lowering as LW
from sigops_amd.engine import Plan
from oracle_bridge import relerr
from sampleat_interp_ref import KINDS, N_CHANNELS, N_RESULT, N_TABLE, P, positions, same_bits, sampleat_interp, table
from sampleat_ref import sampleat_np

pytestmark = pytest.mark.gpu
FS = 10 * so.kHz
MODES = ({}, {"left": -7.5, "right": np.inf}, {"wrap": True}, {"relative": True}, {"relative": True, "wrap": True})
KIND_IDS = [k + "".join(f"-{a}{v}" for a, v in kw.items()) for k, kw in KINDS]


def bit_equal(got, want, what=""):
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} samples differ, first at {np.argwhere(bad)[0]}"
    assert same_bits(got, want), f"{what}: a zero of the other sign"


def check(x, pos, interp, what="", **kw):
    """the sink of SampleAt(x, pos, interp=...) against the definition"""
    got = so.sink(so.SampleAt(so.Signal(x, FS), so.Signal(pos, FS), interp=interp, **kw), so.Array)
    bit_equal(got, sampleat_interp(x, pos, interp, **kw), f"{what} {interp} {kw}")
    return got


def dev(a):
    """a planar device tensor [frames x channels]"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t()


# ---- 1. planted positions, every table length ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("N", N_TABLE)
def test_planted_positions_equal_the_definition_bit_for_bit(N, kind):
    interp, kw = kind
    for Cn, L in zip(N_CHANNELS + [2, 3], N_RESULT):  # (1, 1) (2, 2) (3, 63) (8, 64) (2, 65) (3, 1001)
        x = table(N, Cn)
        for mode in MODES:
            check(x, positions(N, L), interp, f"N={N} L={L} C={Cn}", **kw, **mode)
    check(table(N, 8), positions(N, 1001, 8), interp, f"N={N}, a pos per channel", **kw, left=1.0, right=-0.0)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_non_finite_and_negative_zero_table_values(kind):
    interp, kw = kind
    for N in (3, 17, 65, 4097):
        for Cn in (1, 3):
            x = table(N, Cn, nonfinite=True)
            pos = positions(N, 1001, Cn)
            for mode in ({}, {"wrap": True}, {"left": np.nan, "right": -np.inf}):
                got = check(x, pos, interp, f"non-finite N={N} C={Cn}", **kw, **mode)
                assert np.isnan(got).any() and (N < 4097 or np.isfinite(got).any())  # (a table shorter than the kernel is poisoned whole)


@pytest.mark.parametrize("kind", KINDS[:4], ids=KIND_IDS[:4])
def test_float32_tables_and_float32_positions(kind):
    interp, kw = kind
    for N in (1, 3, 65, 4097):
        pos = positions(N, 1001, 1, np.float32)
        got = check(table(N, 3, np.float32, nonfinite=True), pos, interp, "Float32", **kw, left=0.25)
        assert got.dtype == np.float64
        check(table(N, 2, np.float32), pos, interp, "Float32 wrap", **kw, wrap=True)
        check(table(N, 2, np.float32), positions(N, 1001, 2), interp, "Float32 table, Float64 positions", **kw, relative=True)
        check(table(N, 2), positions(N, 1001, 2, np.float32), interp, "Float64 table, Float32 positions", **kw)


def test_integer_positions_return_the_table_by_value():
    x = table(65, 3)
    n = np.asfortranarray(np.arange(65, dtype=np.float64).reshape(-1, 1))
    for interp, kw in KINDS[:4]:
        for mode in ({}, {"wrap": True}):
            bit_equal(check(x, n, interp, "integers", **kw, **mode), x, f"x[j] by value {interp} {kw}")
        z = x.copy()
        z[30, 0] = -0.0
        got = check(z, n, interp, "a negative zero", **kw)
        assert got[30, 0] == 0.0 and not np.signbit(got[30, 0])  # the one exception: the sum makes it +0.0
        z[30, 0] = np.inf
        got = check(z, n, interp, "an Inf", **kw)
        assert not np.isfinite(got[29:32, 0]).any() and np.isnan(got[29, 0])  # 0 * Inf poisons the neighbours' integer positions too


def test_the_sinc_kernel_with_its_taps_in_lds():
    """K <= 16 and 2^17 frames x channels or more: the persistent form that stages the tap table in LDS.  Both sides of the
    threshold, both parities of the rows, Float32 and wrap."""
    N = 4097
    for L, Cn, taps in ((131_072, 1, 16), (131_071, 1, 16), (16_385, 8, 16), (43_691, 3, 10), (65_537, 2, 4)):
        x = table(N, Cn)
        pos = np.asfortranarray(np.linspace(-3.0, N + 2.0, L).reshape(-1, 1) + 2.5 * np.sin(np.arange(L) / 50.0).reshape(-1, 1))
        pos[:1001] = positions(N, 1001)
        check(x, pos, "sinc", f"L={L} C={Cn}", taps=taps)
        check(x, pos, "sinc", f"L={L} C={Cn}", taps=taps, cutoff=0.5, wrap=True)
    x32 = table(N, 2, np.float32)
    rng = np.random.default_rng(5)
    pos = np.asfortranarray(rng.uniform(-2.0, N + 2.0, size=(70_001, 2)))
    check(x32, pos, "sinc", "random positions, Float32")
    tree = so.SampleAt(so.Signal(x32, FS), so.Signal(pos, FS), interp="sinc", relative=True, wrap=True)
    whole = so.sink(tree, so.Array)
    bit_equal(whole, sampleat_interp(x32, pos, "sinc", relative=True, wrap=True), "relative, wrap")
    bit_equal(so.sink(tree | so.After(1 * so.frames), so.Array), whole[1:], "an odd window base")


# ---- 2. broadcast, windows, streams ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS[:4], ids=KIND_IDS[:4])
def test_a_mono_pos_is_broadcast_and_windows_and_streams_equal_the_whole_sink(kind):
    interp, kw = kind
    x = table(65, 3)
    mono = positions(65, 1001)
    a = check(x, mono, interp, "mono", **kw)
    b = check(x, np.asfortranarray(np.repeat(mono, 3, axis=1)), interp, "repeated", **kw)
    bit_equal(a, b, "mono against repeated")
    pos = positions(65, 1001, 3)
    for mode in ({}, {"relative": True}, {"wrap": True}):
        tree = so.SampleAt(so.Signal(x, FS), so.Signal(pos, FS), interp=interp, **kw, **mode)
        whole = sampleat_interp(x, pos, interp, **kw, **mode)
        bit_equal(so.sink(tree, so.Array), whole, f"whole {mode}")
        bit_equal(so.sink(tree | so.After(1 * so.frames), so.Array), whole[1:], f"After(1 frame) {mode}")  # (an odd window base)
        bit_equal(so.sink(tree | so.After(130 * so.frames) | so.Until(65 * so.frames), so.Array), whole[130:195], f"After | Until {mode}")
        bit_equal(so.sink(tree | so.Until(63 * so.frames), so.Array), whole[:63], f"Until {mode}")  # (an odd result pitch)
        bit_equal(np.vstack([b for b in so.stream(tree, 333, so.Array)]), whole, f"blocks of 333 {mode}")
        bit_equal(np.vstack(list(islice(so.stream(tree | so.After(1 * so.frames), 7, so.Array), 30))), whole[1:211], f"blocks of 7 {mode}")
    # a formula as pos: the window computes only its own frames, with absolute frame numbers
    f = so.SampleAt(so.Signal(x, FS), so.Signal(so.elementwise(lambda t: t * 3000.0), FS), interp=interp, relative=True, **kw) | so.Until(1001 * so.frames)
    fw = so.sink(f, so.Array)
    bit_equal(so.sink(f | so.After(333 * so.frames) | so.Until(65 * so.frames), so.Array), fw[333:398], "a formula, windowed")
    bit_equal(np.vstack([b for b in so.stream(f, 65, so.Array)]), fw, "a formula, streamed")


# ---- 3. leaves, strides, plan reuse ------------------------------------------------------------------------------------------
def test_device_leaves_host_leaves_interleaved_and_strided_tables():
    import torch

    for interp, kw in KINDS[:4]:
        for N, L, Cn in ((65, 1001, 3), (4097, 65, 8), (3, 63, 2)):
            x, pos = table(N, Cn), positions(N, L, Cn)
            for mode in ({}, {"relative": True, "wrap": True}):
                want = sampleat_interp(x, pos, interp, **kw, **mode)
                got, fs = so.sink(so.SampleAt(so.Signal(dev(x), FS), so.Signal(dev(pos), FS), interp=interp, **kw, **mode), "torch")
                assert fs == 10_000.0 and got.is_cuda
                bit_equal(got.cpu().numpy(), np.ascontiguousarray(want), "device leaves, device result")
                bit_equal(so.sink(so.SampleAt(so.Signal(dev(x), FS), so.Signal(pos, FS), interp=interp, **kw, **mode), so.Array), want, "device table, host pos")
        # an interleaved host table (frames x channels, C order) and an interleaved device table are read where they lie
        xi = np.ascontiguousarray(table(65, 3))
        want = sampleat_interp(xi, positions(65, 1001), interp, **kw)
        bit_equal(so.sink(so.SampleAt(so.Signal(xi, FS), so.Signal(positions(65, 1001), FS), interp=interp, **kw), so.Array), want, "interleaved")
        bit_equal(so.sink(so.SampleAt(so.Signal(torch.from_numpy(xi).cuda(), FS), so.Signal(positions(65, 1001), FS), interp=interp, **kw), so.Array), want, "interleaved, device")
        # a strided view: every second frame of a longer table, two of four channels
        big = table(130, 4)
        view = big[::2, 1:3]
        bit_equal(so.sink(so.SampleAt(so.Signal(view, FS), so.Signal(positions(65, 1001), FS), interp=interp, **kw), so.Array),
                  sampleat_interp(np.asfortranarray(view), positions(65, 1001), interp, **kw), "a strided view")


@pytest.mark.parametrize("kind", [KINDS[0], KINDS[1], KINDS[3]], ids=[KIND_IDS[0], KIND_IDS[1], KIND_IDS[3]])
def test_a_plan_is_reused_after_set_array_on_x_and_on_pos(kind):
    import torch

    interp, kw = kind
    xs = [table(65, 2, seed=k) for k in range(3)]
    ps = [positions(65, 1001, 2, seed=k) for k in range(3)]
    res = np.zeros((1001, 2), order="F")
    p = Plan(so.SampleAt(so.Signal(xs[0], FS), so.Signal(ps[0], FS), relative=True, interp=interp, **kw), res.shape, res.dtype, (1, res.shape[0]), False)
    scratch = p.stats()["scratch_bytes"]
    for kx, kp in ((0, 0), (1, 0), (1, 1), (2, 2), (0, 2)):
        p.set_array(0, xs[kx])
        p.set_array(1, ps[kp])
        p.execute(res.ctypes.data)
        bit_equal(res, sampleat_interp(xs[kx], ps[kp], interp, relative=True, **kw), f"host leaves x{kx} pos{kp}")
        assert p.stats()["scratch_bytes"] == scratch
    p.close()
    # device leaves, a device result: nothing is copied per execute; the plan owns the tap table and nothing else
    dx, dp = [dev(a) for a in xs], [dev(a) for a in ps]
    out = torch.empty((2, 1001), dtype=torch.float64, device="cuda").t()
    p = Plan(so.SampleAt(so.Signal(dx[0], FS), so.Signal(dp[0], FS), wrap=True, interp=interp, **kw), (1001, 2), np.float64, (1, 1001), True)
    p.set_profiling(True)
    tab_bytes = (2 * P + 1) * kw.get("taps", 16) * 8 if interp == "sinc" else 0
    for kx, kp in ((0, 0), (0, 0), (1, 0), (1, 1), (2, 2), (2, 2)):
        p.set_array(0, dx[kx])
        p.set_array(1, dp[kp])
        p.execute(out.data_ptr())
        p.check()
        bit_equal(out.cpu().numpy(), np.ascontiguousarray(sampleat_interp(xs[kx], ps[kp], interp, wrap=True, **kw)), f"device leaves x{kx} pos{kp}")
        s = p.stats()
        assert s["h2d_bytes"] == 0 and s["d2h_bytes"] == 0 and tab_bytes <= s["scratch_bytes"] <= tab_bytes + 4096
    steps = p.steps()
    p.close()
    assert [s["name"] for s in steps] == ["k_sample_at_" + interp] and steps[0]["launches"] == 1, steps
    taps = kw.get("taps", 16) if interp == "sinc" else 4
    assert steps[0]["algorithmic_bytes"] == 1001 * (2 * 8 + 2 * (taps * 8 + 8)), steps


def test_linear_spelled_out_is_the_node_it_was_and_runs_k_sample_at():
    import torch

    x, pos = table(65, 2), positions(65, 1001, 2)
    for mode in MODES:
        a = so.sink(so.SampleAt(so.Signal(x, FS), so.Signal(pos, FS), **mode), so.Array)
        b = so.sink(so.SampleAt(so.Signal(x, FS), so.Signal(pos, FS), interp="linear", **mode), so.Array)
        bit_equal(b, a, f"interp='linear' {mode}")
        bit_equal(b, sampleat_np(x, pos, **mode), f"np.interp {mode}")
    bit_equal(so.sink(so.Delay(so.Signal(x, FS), 2.375, interp="linear"), so.Array), so.sink(so.Delay(so.Signal(x, FS), 2.375), so.Array), "Delay")
    out = torch.empty((2, 1001), dtype=torch.float64, device="cuda").t()
    p = Plan(so.SampleAt(so.Signal(dev(x), FS), so.Signal(dev(pos), FS), interp="linear"), (1001, 2), np.float64, (1, 1001), True)
    p.set_profiling(True)
    p.execute(out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    steps = p.steps()
    p.close()
    assert [s["name"] for s in steps] == ["k_sample_at"] and steps[0]["algorithmic_bytes"] == 1001 * (2 * 8 + 2 * (2 * 8 + 8)), steps


# ---- 4. computed operands and consumers ------------------------------------------------------------------------------------
def test_a_filtered_table_and_a_traced_position():
    raw = table(4097, 2)
    pos = positions(4097, 1001, 2)
    filtered = so.Signal(raw, FS) | so.Filt(so.Lowpass, 1 * so.kHz)
    xf = so.sink(filtered, so.Array)  # the table, sunk separately
    assert np.isfinite(xf).all() and np.ptp(xf) > 0.5
    x = table(65, 2)
    fn = so.elementwise(lambda t: 32.0 + 40.0 * np.sin(t * 700.0))
    psig = so.Signal(fn, FS) | so.Until(1001 * so.frames)
    traced = so.sink(psig, so.Array)  # the positions, sunk separately
    assert traced.min() < -2 and traced.max() > 66
    for interp, kw in KINDS[:4]:
        for mode in ({}, {"relative": True, "wrap": True}):
            got = so.sink(so.SampleAt(filtered, so.Signal(pos, FS), interp=interp, **kw, **mode), so.Array)
            bit_equal(got, sampleat_interp(xf, pos, interp, **kw, **mode), f"Filt(Lowpass) as the table {interp} {mode}")
        for mode in ({}, {"wrap": True}, {"relative": True}):
            got = so.sink(so.SampleAt(so.Signal(x, FS), psig, interp=interp, **kw, **mode), so.Array)
            bit_equal(got, sampleat_interp(x, traced, interp, **kw, **mode), f"Signal(elementwise) as pos {interp} {mode}")


def close(got, want, what):
    """the bound tests/test_gpu_sampleat.py holds a consumer behind a materialised buffer to"""
    assert got.shape == want.shape
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    e = relerr(got, want)
    print(f"worst {what}: {e:.3e}")
    assert e <= 1e-12, f"{what}: {e:.3e}"


@pytest.mark.parametrize("kind", [KINDS[0], KINDS[1]], ids=KIND_IDS[:2])
def test_consumers_behind_it(kind):
    interp, kw = kind
    x = table(4097, 2)
    pos = np.asfortranarray(np.linspace(0.0, 4096.0, 30_000).reshape(-1, 1) + 3.0 * np.sin(np.arange(30_000) / 50.0).reshape(-1, 1))
    tree = so.SampleAt(so.Signal(x, FS), so.Signal(pos, FS), interp=interp, **kw)
    mid = so.sink(tree, so.Array)  # the SampleAt result, sunk separately
    bit_equal(mid, sampleat_interp(x, pos, interp, **kw))
    for name, tail in (("Filt(Highpass)", lambda t: t | so.Filt(so.Highpass, 1 * so.kHz)),
                       ("ToFramerate", lambda t: t | so.ToFramerate(12 * so.kHz)),
                       ("Normpower", lambda t: t | so.Normpower),
                       ("a map", lambda t: so.Amplify(t, 0.25) | so.ToEltype(np.float32))):
        got = so.sink(tail(tree), so.Array)
        want = so.sink(tail(so.Signal(mid, FS)), so.Array)
        assert got.dtype == want.dtype and np.ptp(want) > 0.1
        close(got, want, f"SampleAt({interp}) | {name}")


def test_delays_a_vibrato_and_a_wavetable_oscillator():
    x = table(65, 3)
    xs = so.Signal(x, FS)
    for interp, kw in KINDS[:4]:
        for k in (0, 1, 63, 64, 65):  # an integer delay: x behind k zeros, by value
            want = np.zeros_like(x)
            want[k:] = x[:max(65 - k, 0)]
            got = so.sink(so.Delay(xs, k, interp=interp, **kw), so.Array)
            assert np.array_equal(got, want), f"Delay(x, {k}) {interp} {kw}"
            bit_equal(got, sampleat_interp(x, np.full((65, 1), -float(k)), interp, relative=True, **kw), f"Delay(x, {k}) {interp} {kw}")
        d = 2.375
        want = sampleat_interp(x, np.full((65, 1), -d), interp, relative=True, **kw)
        bit_equal(so.sink(so.Delay(xs, d, interp=interp, **kw), so.Array), want, "a fractional delay")
        bit_equal(so.sink(xs | so.Delay(so.Signal(np.full((65, 1), d), FS), interp=interp, **kw), so.Array), want, "a signal, curried")
    # a vibrato: SampleAt(x, n + depth * sin), the positions traced on the device and sunk separately for the reference
    tone = np.asfortranarray(np.sin(2 * np.pi * 0.11 * np.arange(4097)).reshape(-1, 1))
    lfo = so.Signal(so.elementwise(lambda t: t * 10_000.0 + 5.0 + 4.5 * np.sin(t * 40.0)), FS) | so.Until(4000 * so.frames)
    p = so.sink(lfo, so.Array)
    got = so.sink(so.SampleAt(so.Signal(tone, FS), lfo, interp="sinc"), so.Array).reshape(-1, 1)
    bit_equal(got, sampleat_interp(tone, p.reshape(-1, 1), "sinc"), "vibrato")
    assert np.ptp(got) > 1.9
    # a wavetable oscillator: a 2048-entry sine read at the running sum of a frequency trajectory
    n, size = 40_000, 2048
    wt = np.sin(2 * np.pi * np.arange(size) / size).reshape(-1, 1)
    hz = 220.0 * np.exp2(np.linspace(0.0, 2.0, n))
    f = np.asfortranarray((hz * size / 10_000.0).reshape(-1, 1))
    phase = so.sink(so.Cumsum(so.Signal(f, FS)), so.Array).reshape(n, 1)
    assert phase[-1, 0] > 1000 * size  # many wraps
    got = so.sink(so.SampleAt(so.Signal(wt, FS), so.Cumsum(so.Signal(f, FS)), wrap=True, interp="cubic"), so.Array)
    bit_equal(got.reshape(n, 1), sampleat_interp(wt, phase, "cubic", wrap=True), "the oscillator")
    assert np.ptp(got) > 1.9


# ---- 5. refusals that need the engine ------------------------------------------------------------------------------------
def _create(lw, nframes, nch):
    out = K.so_out_desc_t(dtype=K.SO_F64, nch=nch, nframes=nframes, frame_stride=1, chan_stride=nframes, is_device=0)
    plan = C.c_void_p()
    st = K.lib().so_plan_create(lw.nodes, lw.n, lw.root, C.byref(out), 0, C.byref(plan))
    if plan.value:
        K.lib().so_plan_destroy(plan)
    return st, K.last_error() if st else ""


def test_malformed_nodes_are_refused():
    x, pos = so.Signal(table(65, 3), FS), so.Signal(positions(65, 64), FS)
    lw = LW.lower(so.SampleAt(x, pos, interp="sinc", taps=8))
    assert _create(lw, 64, 3)[0] == 0  # the well-formed node
    nd = lw.nodes[lw.root]
    assert nd.kind == K.NODE_SAMPLEAT and (nd.i1, nd.i2, nd.s0) == (2, 8, (2 * P + 1) * 8)

    def refused(words, **fields):
        old = {k: getattr(nd, k) for k in fields}
        for k, v in fields.items():
            setattr(nd, k, v)
        st, err = _create(lw, 64, 3)
        for k, v in old.items():
            setattr(nd, k, v)
        assert st == -1 and f"node {lw.root}" in err and "SampleAt" in err and words in err, (fields, st, err)

    refused("unknown interpolation 3", i1=3)
    refused("unknown interpolation -1", i1=-1)
    refused("unknown flags", i0=4)
    refused("even number of taps from 4 to 64 (7 given)", i2=7)
    refused("even number of taps from 4 to 64 (2 given)", i2=2)
    refused("even number of taps from 4 to 64 (66 given)", i2=66)
    refused("tap table of (2 * 512 + 1) * 10 = 10250 doubles (8200 given)", i2=10)
    refused("tap table of (2 * 512 + 1) * 8 = 8200 doubles (8199 given)", s0=8199)
    refused("tap table of (2 * 512 + 1) * 8 = 8200 doubles (none given)", p0=None)
    refused("sinc interpolation only", i1=1)  # (a cubic node that carries taps and a table)
    refused("sinc interpolation only", i1=0)
    tab = np.ctypeslib.as_array(C.cast(nd.p0, C.POINTER(C.c_double)), shape=(nd.s0,))
    for bad in (np.nan, np.inf):
        keep, tab[4321] = tab[4321], bad
        refused("tap table entry 4321 is not finite")
        tab[4321] = keep
    assert _create(lw, 64, 3)[0] == 0  # (everything was put back)
