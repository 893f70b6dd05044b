"""The fused resampler + IIR kernel's warm-up as one product (k_rsos.hip rsos_wproj_*, csrc/stages.cpp rsos_wproj_matrix).

A range of the kernel starts wp periods early from rest; where those periods lie wholly inside the array the state at their
end comes from s_0 = V . in instead of a walk through them (`plan.counters()["wproj"]`; `SIGOPS_RSOS_NOWPROJ=1` keeps the
walk).  Checked here, on signals of ~12 s that `SIGOPS_RSOS_MINGROUPS=1` puts on the fused kernel: the oracle (1e-9) and the
engine's two kernels (1e-11) as in test_gpu_rsos.py; projection against walk (rounding only: WPROJ_VS_WALK below); groups
that must walk (the signal's first ranges, windows) next to groups that project, several groups per workgroup; non-finite
samples inside, just outside and in the k-step padding of a projected span (the reference's set of non-finite outputs, as
in test_gpu_rsos_nonfinite.py); graph replay and replaced array leaves."""
import numpy as np
import pytest

import sigops_amd as so
from oracle_bridge import oracle_sink, relerr
from test_gpu_rsos import F, env

pytestmark = pytest.mark.gpu

N = 529_200  # 12 s at 44.1 kHz
# projection against walk, relerr: the maximum over the cases of this file as measured (profiles/r07/wproj_vs_walk.txt: 6.6e-13
# with the fused sine, whose phase at the span's first frame is rounded differently from the loader's chunk bases; 5e-15
# without); asserted at ten times that, and never above the kernel-against-two-kernels bound
WPROJ_VS_WALK = 6.7e-13
CEILING = 1e-11


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
        p.execute(out.ctypes.data)
    finally:
        p.close()
    return out, c


def two_kernels(x):
    with env(SIGOPS_NO_RSOS=1):
        return so.sink(x)[0]


_noise = {}


def noise(nch, n=N, seed=7):
    if (nch, n, seed) not in _noise:
        _noise[(nch, n, seed)] = F(np.random.default_rng(seed + nch).standard_normal((n, nch)))
    return _noise[(nch, n, seed)]


def bandstop(src, fs_out=48.0):
    return src | so.Filt(so.Bandstop, 0.5 * so.kHz, 2 * so.kHz) | so.ToFramerate(fs_out * so.kHz)


def make(kind, d=None):
    if kind == "plain":
        return bandstop(so.Signal(noise(8) if d is None else d, 44.1 * so.kHz))
    if kind == "mix":
        return bandstop(so.Mix(so.Signal(so.sin, ω=1 * so.kHz), so.Signal(noise(8) if d is None else d, 44.1 * so.kHz)) | so.Until(N * so.frames))
    if kind == "minus":  # v - sine
        return bandstop(so.OperateOn(np.subtract, so.Signal(noise(8), 44.1 * so.kHz), so.Signal(so.sin, ω=1 * so.kHz)) | so.Until(N * so.frames))
    if kind == "ch16_lowpass4":  # 16 channels: one range per group; 4 sections: two k-steps of state
        return so.Signal(noise(16, N // 2), 44.1 * so.kHz) | so.Filt(so.Lowpass, 5 * so.kHz, order=7) | so.ToFramerate(48 * so.kHz)
    if kind == "32to48":  # another rate pair: a tap table of the kernel's own, another window length
        return bandstop(so.Signal(noise(8, 384_000), 32 * so.kHz))
    if kind == "window":  # the first range's warm-up lies in front of the array: that group walks, the others project
        return bandstop(so.Signal(noise(8), 44.1 * so.kHz)) | so.After(300 * so.frames) | so.Until(500_000 * so.frames)
    raise KeyError(kind)


_oracle = {}


def oracle(kind):
    if kind not in _oracle:
        _oracle[kind] = oracle_sink(make(kind))
    return _oracle[kind]


@pytest.mark.parametrize("kind", ["plain", "mix", "minus", "ch16_lowpass4", "32to48", "window"])
def test_projection_against_oracle_two_kernels_and_walk(kind):
    x = make(kind)
    got, c = run(x)
    assert c["wproj"] == 1
    walk, cw = run(x, SIGOPS_RSOS_NOWPROJ=1)
    assert cw["wproj"] == 0
    d = relerr(got, walk)
    print(f"wproj_vs_walk {kind} {d:.3e}")
    assert relerr(got, oracle(kind)) < 1e-9
    assert relerr(got, two_kernels(x)) < 1e-11
    assert not np.array_equal(got, walk)  # (the projection ran: another association of the same sums)
    assert d < min(CEILING, 10 * WPROJ_VS_WALK)


@pytest.mark.parametrize("kind", ["plain", "mix"])
@pytest.mark.parametrize("grid, ranges", [(256, None), (26, 156)])
def test_groups_per_workgroup(kind, grid, ranges):
    """one sequence group per workgroup, and three (156 ranges = 78 groups of two on 26 workgroups): the prologue runs at
    every group's start"""
    x = make(kind)
    got, c = run(x, SIGOPS_RSOS_GRID=grid, SIGOPS_RSOS_RANGES=ranges)
    assert c["wproj"] == 1
    walk, _ = run(x, SIGOPS_RSOS_GRID=grid, SIGOPS_RSOS_RANGES=ranges, SIGOPS_RSOS_NOWPROJ=1)
    d = relerr(got, walk)
    print(f"wproj_vs_walk {kind}/grid{grid} {d:.3e}")
    assert relerr(got, oracle(kind)) < 1e-9
    assert relerr(got, two_kernels(x)) < 1e-11
    assert not np.array_equal(got, walk)
    assert d < min(CEILING, 10 * WPROJ_VS_WALK)


def test_a_plan_whose_groups_all_walk_is_the_walk_bit_for_bit():
    """two ranges = one group, and it holds range 0, whose warm-up lies in front of the signal"""
    x = make("mix")
    got, c = run(x, SIGOPS_RSOS_RANGES=2)
    assert c["wproj"] == 1
    walk, cw = run(x, SIGOPS_RSOS_RANGES=2, SIGOPS_RSOS_NOWPROJ=1)
    assert cw["wproj"] == 0
    assert np.array_equal(got, walk)
    assert relerr(got, oracle("mix")) < 1e-9


def plan_geometry(x):
    """(periods per range, warm-up periods, input frames per period, frames of the projected span, its first frame relative
    to the warm-up's first input) of the plan `sink(x)` runs"""
    n, nch = so.nframes(x), so.nchannels(x)
    with env(SIGOPS_RSOS_MINGROUPS=1):
        p = so.Plan(so.ToChannels(x, nch), (n, nch), np.float64, (1, n), False)
    try:
        g = p.rsos_geometry()
    finally:
        p.close()
    assert g["wproj_frames"] > 0, g
    return g["pr"], g["wp"], g["M"], g["wproj_frames"], g["wproj_first"]


@pytest.mark.parametrize("where", ["inside", "one frame in front", "padding behind"])
def test_non_finite_samples_around_a_projected_span(where):
    """NaN in channel 1 around the span of range 5, Inf in channel 6 around that of range 9 (groups of two ranges: both
    project).  The padding behind a span of K frames are the frames up to the next multiple of 8: never loaded."""
    pr, wp, M, K, j0 = plan_geometry(make("plain"))
    d = noise(8).copy(order="F")
    for r, ch, val in ((5, 1, np.nan), (9, 6, np.inf)):
        lo = (r * pr - wp) * M + j0
        i = {"inside": lo + K // 2 + r, "one frame in front": lo - 1, "padding behind": lo + K}[where]
        assert 0 < i < N
        d[i, ch] = val
    for kind in ("plain", "mix"):
        x = make(kind, d)
        got, c = run(x)
        assert c["wproj"] == 1
        want = oracle_sink(x)
        bad = ~np.isfinite(want)
        assert bad[:, 1].any() and bad[:, 6].any() and not bad[:, [0, 2, 3, 4, 5, 7]].any()
        assert np.array_equal(~np.isfinite(got), bad)
        assert relerr(got[~bad], want[~bad]) < 1e-9


def test_graph_replay_and_a_replaced_array():
    """four pieces of an `Append`, each an array through its own filter and the resampler: four fused launches, a plan the
    executor replays from a captured graph once it has run twice into the same device result.  Replayed executes, and
    executes after every array leaf was replaced (so_plan_set_array: a new capture), are a fresh plan's results bit for bit."""
    torch = pytest.importorskip("torch")
    n = N // 2
    filts = [lambda: so.Filt(so.Bandstop, 0.5 * so.kHz, 2 * so.kHz), lambda: so.Filt(so.Lowpass, 5 * so.kHz, order=7),
             lambda: so.Filt(so.Highpass, 200 * so.Hz, order=7), lambda: so.Filt(so.Lowpass, 3 * so.kHz, order=5)]

    def tree(arrs):
        return so.Append(*[so.Signal(a, 44.1 * so.kHz) | f() | so.ToFramerate(48 * so.kHz) for a, f in zip(arrs, filts)])

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t()

    A = [noise(8, n, seed=20 + k) for k in range(4)]
    B = [noise(8, n, seed=30 + k) for k in range(4)]
    fresh = [run(tree(v))[0] for v in (A, B)]
    dA, dB = [dev(a) for a in A], [dev(b) for b in B]
    x = tree(dA)
    nout = so.nframes(x)
    out_t = torch.empty((8, nout), dtype=torch.float64, device="cuda")
    out = out_t.t()
    with env(SIGOPS_RSOS_MINGROUPS=1):
        plan = so.Plan(so.ToChannels(x, 8), (nout, 8), np.float64, (out.stride(0), out.stride(1)), True)
    stream = torch.cuda.current_stream().cuda_stream
    try:
        assert [s["name"] for s in plan.steps()].count("k_rsos") == 4, plan.steps()
        assert plan.counters()["wproj"] == 1
        for _ in range(4):  # direct, capture + launch, replay, replay
            out_t.zero_()
            plan.execute(out.data_ptr(), stream)
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), fresh[0])
        c = plan.counters()
        assert c["graph_replays"] >= 1 and c["graph_captures"] >= 1, c
        for k in range(4):
            plan.set_array(k, dB[k])
        for _ in range(3):
            out_t.zero_()
            plan.execute(out.data_ptr(), stream)
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), fresh[1])
        c2 = plan.counters()
        assert c2["graph_replays"] > c["graph_replays"] and c2["graph_captures"] > c["graph_captures"], c2
    finally:
        plan.close()
