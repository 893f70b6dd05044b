"""The chain wave's recurrence on the 4 x 4 x 4 matrix shape (k_rsos.hip rsos_chain4; csrc/stages.cpp rsos_chain4_operands).

A^16 of a cascade is block lower triangular in 4 x 4 blocks, so the chain wave of the fused resampler + IIR kernel issues one
v_mfma_f64_4x4x4_4b_f64 per block (r, c), c <= r -- six, three or one per step -- instead of three 16 x 16 x 4
(`plan.counters()["chain4"] == 1`).  `SIGOPS_RSOS_CHAIN16=1` keeps the large shape.  The form follows the filter alone, so it
is checked here on every form the kernel has -- cascades of 1 .. 6 sections (NK = 1, 2, 3, half-filled and full last block),
folded and unfolded, eight, twelve and sixteen waves, Float32, the one-pass plain filter, the batched launch, a state that
enters block 0 through slot 0 (projected warm-up) and one that does not, a window, non-finite input -- on 60 001 frames x 8
channels in four ranges (`SIGOPS_RSOS_MINGROUPS=1`, `SIGOPS_RSOS_RANGES=4`) unless the case says otherwise (the batch: the planner's own
choice of ranges under `SIGOPS_RSOS_BATCH=1`; two and four channels: with a fused sine, which is what takes sixteen waves).

Every case: the oracle (1e-9; a Float32 result: 1e-6, the suite's Float32 bound -- its own rounding is 6e-8 a value) and
the large shape.  The sums keep their order per row block and the blocks left out added exact zeros: the two shapes gave the
same bytes in every case when this was written (profiles/r17/chain4_vs_chain16.txt), so equality is what is asserted."""
import os

import numpy as np
import pytest

import sigops_amd as so
from oracle_bridge import oracle_semantics, oracle_sink, relerr
from test_gpu_rsos import F, env

pytestmark = pytest.mark.gpu

N = 60_001
BASE = dict(SIGOPS_RSOS_MINGROUPS=1, SIGOPS_RSOS_RANGES=4)
_seen = {}


def record(name, d):
    """every case's figure printed; SIGOPS_RECORD_CHAIN4=<file>: the figures so far and their maximum rewritten there (how
    profiles/r17/chain4_vs_chain16.txt was made)"""
    print(f"chain4_vs_chain16 {name} {d:.3e}")
    _seen[name] = d
    if os.environ.get("SIGOPS_RECORD_CHAIN4"):
        with open(os.environ["SIGOPS_RECORD_CHAIN4"], "w") as f:
            f.write("k_rsos chain wave on the 4x4x4 shape against SIGOPS_RSOS_CHAIN16=1, norm-wise relerr per case of tests/test_gpu_rsos_chain4.py\n")
            for k, v in _seen.items():
                f.write(f"{k} {v:.3e}\n")
            f.write(f"max {max(_seen.values()):.3e}\n")


_noise = {}


def noise(nch, n=N, dt=np.float64, seed=17):
    key = (nch, n, np.dtype(dt).name, seed)
    if key not in _noise:
        _noise[key] = F(np.random.default_rng(seed + nch).standard_normal((n, nch)).astype(dt))
    return _noise[key]


def bandstop(src, order=5):
    return src | so.Filt(so.Bandstop, 0.5 * so.kHz, 2 * so.kHz, order=order) | so.ToFramerate(48 * so.kHz)


def mixed(d):
    return so.Mix(so.Signal(so.sin, ω=1 * so.kHz), so.Signal(d, 44.1 * so.kHz)) | so.Until(d.shape[0] * so.frames)


def run(x, step="k_rsos", dtype=np.float64, **kv):
    """(result, counters) of a fresh plan with a host result"""
    n, nch = so.nframes(x), so.nchannels(x)
    out = np.empty((n, nch), dtype=dtype, order="F")
    with env(**{**BASE, **kv}):
        p = so.Plan(so.ToChannels(x, nch), (n, nch), dtype, (1, n), False)
        try:
            c = p.counters()
            if step == "k_rsos_batch":  # (the planner forms the batch; its step is listed under that name once it has run under profiling)
                p.set_profiling(True)
            p.execute(out.ctypes.data)
            assert step in [s["name"] for s in p.steps()], p.steps()
        finally:
            p.close()
    return out, c


def make(kind, d=None):
    if kind.startswith("sections"):  # a band-stop of order k: k sections
        return bandstop(so.Signal(noise(8), 44.1 * so.kHz), order=int(kind[-1]))
    if kind in ("folded", "nofold", "nwaves8"):
        return bandstop(so.Signal(noise(8) if d is None else d, 44.1 * so.kHz))
    if kind in ("ch2", "ch4"):  # groups of two / four channels with a fused step: sixteen waves
        return bandstop(mixed(noise(int(kind[-1]))))
    if kind == "float32":
        return bandstop(so.Signal(noise(8, dt=np.float32), 44.1 * so.kHz))
    if kind == "onepass":  # the plain filter: k_rsos with the identity resampler
        return so.Signal(noise(8), 48 * so.kHz) | so.Filt(so.Bandstop, 0.5 * so.kHz, 2 * so.kHz)
    if kind == "batch":  # three filtered scenes under an Append: one k_rsos_batch launch
        return so.Append(*[so.Signal(noise(2, n, seed=40 + k), 44.1 * so.kHz) | so.Filt(so.Bandstop, 0.5 * so.kHz, 2 * so.kHz)
                           for k, n in enumerate((50_001, 7_777, 30_000))])
    if kind in ("mix", "mix_nowproj"):
        return bandstop(mixed(noise(8) if d is None else d))
    if kind == "window":
        return bandstop(so.Signal(noise(8), 44.1 * so.kHz)) | so.After(300 * so.frames) | so.Until(50_000 * so.frames)
    raise KeyError(kind)


ENV = {"nofold": dict(SIGOPS_RSOS_NOFOLD=1), "nwaves8": dict(SIGOPS_RSOS_NWAVES=8), # (scenes are batched only without MINGROUPS)
       "batch": dict(SIGOPS_RSOS_BATCH=1, SIGOPS_RSOS_MINGROUPS=None, SIGOPS_RSOS_RANGES=None),
       "mix_nowproj": dict(SIGOPS_RSOS_NOWPROJ=1)}
WANT = {"folded": dict(fold=1), "nofold": dict(fold=0), "mix": dict(wproj=1), "mix_nowproj": dict(wproj=0)}
KINDS = ["sections1", "sections2", "sections3", "sections4", "sections5", "sections6", "folded", "nofold", "nwaves8", "ch2", "ch4", "float32",
         "onepass", "batch", "mix", "mix_nowproj", "window"]


@pytest.mark.parametrize("kind", KINDS)
def test_chain4_against_oracle_and_the_large_shape(kind, capfd):
    x = make(kind)
    kv = ENV.get(kind, {})
    step = "k_rsos_batch" if kind == "batch" else "k_rsos"
    dt = np.float32 if kind == "float32" else np.float64
    got, c = run(x, step, dt, SIGOPS_DEBUG_PLAN=1, **kv)
    plan_log = capfd.readouterr().err
    ref, cr = run(x, step, dt, SIGOPS_RSOS_CHAIN16=1, **kv)
    assert c["chain4"] == 1 and cr["chain4"] == 0  # (the batch: its members are the plan's k_rsos stages, the first one's form)
    for k, v in WANT.get(kind, {}).items():
        assert c[k] == v and cr[k] == v, (k, c, cr)
    if kind == "nwaves8":
        assert "waves=8 " in plan_log
    if kind in ("ch2", "ch4"):
        assert "waves=16 " in plan_log
    if kind == "onepass":
        assert "IIR in one pass" in plan_log
    assert got.dtype == dt
    d = relerr(got, ref)
    record(kind, d)
    with oracle_semantics("intended"):
        want = oracle_sink(x)
    assert got.shape == want.shape
    assert relerr(got, want) < (1e-6 if dt == np.float32 else 1e-9)
    assert np.array_equal(got, ref)


def test_non_finite_input_and_the_plan_executed_again():
    """a NaN and an Inf in one channel: the oracle's set of non-finite outputs, the clean channels finite; the same plan
    executed again over finite data gives a fresh plan's bytes"""
    fin = noise(8)
    bad = fin.copy(order="F")
    bad[N // 3 + 3, 5] = np.nan
    bad[N // 2 + 1001, 5] = np.inf
    x = make("folded", fin)
    n = so.nframes(x)
    fresh, c = run(x)
    assert c["chain4"] == 1 and np.isfinite(fresh).all()
    want = oracle_sink(make("folded", bad))
    w = ~np.isfinite(want)
    assert w[:, 5].any() and not w[:, [0, 1, 2, 3, 4, 6, 7]].any()
    with env(**BASE):
        p = so.Plan(so.ToChannels(x, 8), (n, 8), np.float64, (1, n), False)
    try:
        assert p.counters()["chain4"] == 1
        outs = []
        for d in (bad, fin, bad, fin):
            out = np.full((n, 8), -1.0, order="F")
            p.set_array(0, d)
            p.execute(out.ctypes.data)
            outs.append(out)
    finally:
        p.close()
    for got in (outs[0], outs[2]):
        assert np.array_equal(~np.isfinite(got), w)
        assert relerr(got[~w], want[~w]) < 1e-9
    ref, cr = run(make("folded", bad), SIGOPS_RSOS_CHAIN16=1)
    assert cr["chain4"] == 0
    record("nonfinite", relerr(outs[0][~w], ref[~w]))
    assert np.array_equal(outs[0], ref, equal_nan=True)
    for got in (outs[1], outs[3]):
        assert np.array_equal(got, fresh)
