"""The folded block of the fused resampler + IIR kernel (k_rsos.hip rsos_ywave<..., FOLD>; csrc/stages.cpp rsos_fold_tables).

A folded plan (`plan.counters()["fold"] == 1`) resamples with M_g = T . Tap_g^T, so that a block's product is its zero-state
output Z; the chain wave gets E . Z (E = D . T^-1) and the result is Z + C . S, stored without a transposition.
`SIGOPS_RSOS_NOFOLD=1` keeps the unfolded block.  Checked here on signals of ~12 s and shorter that `SIGOPS_RSOS_MINGROUPS=1`
puts on the fused kernel: the oracle (1e-9), the engine's two kernels (1e-11) and the unfolded block (rounding only:
FOLD_VS_PLAIN below, never equal) on every store path -- aligned 16-byte stores, rows that are only 8-byte aligned, windows,
partial last blocks, ranges beyond the signal, a strided device result --; a filter the planner's gate declines, bit for bit
the unfolded kernel; non-finite input, the reference's set."""
import os

import numpy as np
import pytest

import sigops_amd as so
from oracle_bridge import oracle_sink, relerr
from test_gpu_rsos import F, env

pytestmark = pytest.mark.gpu

N = 529_200  # 12 s at 44.1 kHz
# folded against unfolded, relerr: the maximum over the cases of this file as measured (profiles/r10/fold_vs_plain.txt);
# asserted at ten times that, and never above 1e-12
FOLD_VS_PLAIN = 1.8e-14
CEILING = 1e-12
_seen = {}


def record(name, d):
    """every case's figure printed; SIGOPS_RECORD_FOLD=<file>: the figures so far and their maximum rewritten there (how
    profiles/r10/fold_vs_plain.txt was made)"""
    print(f"fold_vs_plain {name} {d:.3e}")
    _seen[name] = d
    if os.environ.get("SIGOPS_RECORD_FOLD"):
        with open(os.environ["SIGOPS_RECORD_FOLD"], "w") as f:
            f.write("k_rsos folded block against SIGOPS_RSOS_NOFOLD=1, norm-wise relerr per case of tests/test_gpu_rsos_fold.py\n")
            for k, v in _seen.items():
                f.write(f"{k} {v:.3e}\n")
            f.write(f"max {max(_seen.values()):.3e}\n")


def run(x, **kv):
    """(result, counters) of a fresh plan with a host result"""
    n, nch = so.nframes(x), so.nchannels(x)
    out = np.empty((n, nch), order="F")
    kv.setdefault("SIGOPS_RSOS_MINGROUPS", 1)
    with env(**kv):
        p = so.Plan(so.ToChannels(x, nch), (n, nch), np.float64, (1, n), False)
    try:
        assert "k_rsos" in [s["name"] for s in p.steps()]
        c = p.counters()
        assert p.rsos_geometry()["fold"] == c["fold"]
        p.execute(out.ctypes.data)
    finally:
        p.close()
    return out, c


def two_kernels(x):
    with env(SIGOPS_NO_RSOS=1):
        return so.sink(x)[0]


_noise = {}


def noise(nch, n=N, seed=11):
    if (nch, n, seed) not in _noise:
        _noise[(nch, n, seed)] = F(np.random.default_rng(seed + nch).standard_normal((n, nch)))
    return _noise[(nch, n, seed)]


def bandstop(src, fs_out=48.0):
    return src | so.Filt(so.Bandstop, 0.5 * so.kHz, 2 * so.kHz) | so.ToFramerate(fs_out * so.kHz)


# (kind: tree, environment of the plan)
def make(kind, d=None):
    if kind in ("plain", "nwaves8", "grid26"):
        return bandstop(so.Signal(noise(8) if d is None else d, 44.1 * so.kHz))
    if kind == "ldstaps":  # twelve waves that read their taps from the LDS table (at 44.1 kHz table and ring do not fit together)
        return bandstop(so.Signal(noise(8, 288_000), 24 * so.kHz))
    if kind == "mix":
        return bandstop(so.Mix(so.Signal(so.sin, ω=1 * so.kHz), so.Signal(noise(8) if d is None else d, 44.1 * so.kHz)) | so.Until(N * so.frames))
    if kind == "ch16_highpass":  # 16 channels: one range per group; 4 sections
        return so.Signal(noise(16, N // 2), 44.1 * so.kHz) | so.Filt(so.Highpass, 200 * so.Hz, order=7) | so.ToFramerate(48 * so.kHz)
    if kind == "32to48":  # another rate pair: a tap table of the kernel's own, another window length
        return bandstop(so.Signal(noise(8, 384_000), 32 * so.kHz))
    if kind == "cyc2":  # twelve waves whose blocks cycle through two phase groups each
        return bandstop(so.Signal(noise(8, 264_600), 22.05 * so.kHz))
    if kind == "window":  # store_lo, and the first ranges' blocks in front of the signal
        return bandstop(so.Signal(noise(8), 44.1 * so.kHz)) | so.After(300 * so.frames) | so.Until(500_000 * so.frames)
    if kind == "short_odd":  # n_out odd and no multiple of 16: a partial last block, odd channels' rows 8-byte aligned only
        return bandstop(so.Signal(noise(8, 60_001), 44.1 * so.kHz)) | so.Until(65_307 * so.frames)
    raise KeyError(kind)


ENV = {"nwaves8": dict(SIGOPS_RSOS_NWAVES=8), "grid26": dict(SIGOPS_RSOS_GRID=26, SIGOPS_RSOS_RANGES=156), "ldstaps": dict(SIGOPS_RSOS_LDSTAPS=1),
       "short_odd": dict(SIGOPS_RSOS_RANGES=4)}
CYC = {"ldstaps": 0, "plain": 1, "cyc2": 2}

_oracle = {}


def oracle(kind):
    if kind not in _oracle:
        _oracle[kind] = oracle_sink(make(kind))
    return _oracle[kind]


@pytest.mark.parametrize("kind", ["plain", "mix", "ch16_highpass", "32to48", "ldstaps", "cyc2", "nwaves8", "grid26", "window", "short_odd"])
def test_folded_against_oracle_two_kernels_and_unfolded(kind, capfd):
    x = make(kind)
    kv = ENV.get(kind, {})
    if kind in CYC:
        got, c = run(x, SIGOPS_DEBUG_PLAN=1, **kv)
        assert f"cyc={CYC[kind]} " in capfd.readouterr().err  # (the dispatch's tap form this case is here for)
    else:
        got, c = run(x, **kv)
    assert c["fold"] == 1 and c["fused_mfmas_per_block"] in (22, 23, 24, 26, 30)  # (window k-steps + 10)
    if kind == "short_odd":
        assert got.shape[0] % 2 == 1 and got.shape[0] % 16 != 0
    plain, cp = run(x, SIGOPS_RSOS_NOFOLD=1, **kv)
    assert cp["fold"] == 0 and cp["fused_mfmas_per_block"] == c["fused_mfmas_per_block"] + 4
    d = relerr(got, plain)
    record(kind, d)
    assert relerr(got, oracle(kind)) < 1e-9
    assert relerr(got, two_kernels(x)) < 1e-11
    assert not np.array_equal(got, plain)  # (the folded block ran: another association of the same sums)
    assert d < min(CEILING, 10 * FOLD_VS_PLAIN)


def test_device_result_with_the_benchmark_strides():
    """a device-resident leaf and a [nch][n_out] device result read as frames x channels, as bench.py makes them"""
    torch = pytest.importorskip("torch")
    a = noise(8)
    leaf = torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t()
    x = bandstop(so.Mix(so.Signal(so.sin, ω=1 * so.kHz), so.Signal(leaf, 44.1 * so.kHz)) | so.Until(N * so.frames))
    nout = so.nframes(x)
    res = {}
    for nofold in (None, 1):
        out_t = torch.zeros((8, nout), dtype=torch.float64, device="cuda")
        out = out_t.t()
        with env(SIGOPS_RSOS_MINGROUPS=1, SIGOPS_RSOS_NOFOLD=nofold):
            plan = so.Plan(so.ToChannels(x, 8), (nout, 8), np.float64, (out.stride(0), out.stride(1)), True)
        try:
            assert plan.counters()["fold"] == (0 if nofold else 1)
            plan.execute(out.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            res[nofold] = out.cpu().numpy()
        finally:
            plan.close()
    d = relerr(res[None], res[1])
    record("device_result", d)
    assert relerr(res[None], oracle("mix")) < 1e-9
    assert not np.array_equal(res[None], res[1])
    assert d < min(CEILING, 10 * FOLD_VS_PLAIN)


def test_a_declined_filter_is_the_unfolded_kernel_bit_for_bit():
    """Lowpass 5 kHz of order 7: E = D . T^-1 amplifies what T removed (amp ~ 1e5) -- the planner keeps the unfolded block"""
    x = so.Signal(noise(8), 44.1 * so.kHz) | so.Filt(so.Lowpass, 5 * so.kHz, order=7) | so.ToFramerate(48 * so.kHz)
    got, c = run(x)
    assert c["fold"] == 0
    plain, cp = run(x, SIGOPS_RSOS_NOFOLD=1)
    assert cp["fold"] == 0
    assert np.array_equal(got, plain)
    assert relerr(got, oracle_sink(x)) < 1e-9


def test_non_finite_input():
    """one NaN in one channel and one Inf in another, in the middle of the signal: the reference's set of non-finite outputs"""
    d = noise(8).copy(order="F")
    d[N // 2 + 3, 1] = np.nan
    d[N // 2 + 40_001, 6] = np.inf
    for kind in ("plain", "mix"):
        x = make(kind, d)
        got, c = run(x)
        assert c["fold"] == 1
        want = oracle_sink(x)
        bad = ~np.isfinite(want)
        assert bad[:, 1].any() and bad[:, 6].any() and not bad[:, [0, 2, 3, 4, 5, 7]].any()
        assert np.array_equal(~np.isfinite(got), bad)
        assert relerr(got[~bad], want[~bad]) < 1e-9
