"""The words a fused launch notes non-finite ranges in (RsSos::bad) are armed by the fix-up launch of the execute before,
not by a fill launch of every execute (csrc/executor.cpp run_rsos_fused, csrc/k_exact.hip): two sets per stage, used in
turn; the host arms both at the plan's first execute and wherever nobody else has -- graph replays, `SIGOPS_RSOS_NO_FIXUP`,
`SIGOPS_SOS_NOPOISON`.

Checked here on 8 channels x 300 000 frames, 44.1 -> 48 kHz, one k_rsos launch (`SIGOPS_RSOS_MINGROUPS=1`): a plan executed
again and again -- finite data, then an array with a NaN and an Inf, then finite data again -- gives what the oracle gives
every time: a word left at a range number would put NaN over a finite execute, a set never armed would hide a spoiled one.
The sets alternate strictly, so the sequences that tell are those in which a finite execute uses the set a spoiled one
used last ("sff", "fssf", "ssff"): without the fix-up launch's store they fail.  Both parities of the set index end a plan's life; another stream; a plan replayed from a captured graph (its fill node);
the two switches, against a fresh plan's first execute, whose words the host armed."""
import numpy as np
import pytest

import sigops_amd as so
from oracle_bridge import oracle_sink, relerr
from test_gpu_rsos import F, env, steps_of

pytestmark = pytest.mark.gpu

N, NCH = 300_000, 8
_memo = {}


def tree(d):
    return so.Signal(d, 44.1 * so.kHz) | so.ToFramerate(48 * so.kHz) | so.Filt(so.Bandstop, 0.5 * so.kHz, 2 * so.kHz)


def arrays(n=N, seed=41):
    """(finite, spoiled): the same noise, the second with one NaN in channel 2 and one Inf in channel 7"""
    if ("a", n, seed) not in _memo:
        fin = F(np.random.default_rng(seed).standard_normal((n, NCH)))
        bad = fin.copy(order="F")
        bad[n // 3, 2] = np.nan
        bad[n // 2, 7] = np.inf
        _memo[("a", n, seed)] = (fin, bad)
    return _memo[("a", n, seed)]


def oracles(n=N, seed=41):
    if ("o", n, seed) not in _memo:
        fin, bad = arrays(n, seed)
        _memo[("o", n, seed)] = (oracle_sink(tree(fin)), oracle_sink(tree(bad)))
        w = ~np.isfinite(_memo[("o", n, seed)][1])
        assert w[:, 2].any() and w[:, 7].any() and not w[:, [0, 1, 3, 4, 5, 6]].any()
    return _memo[("o", n, seed)]


def host_plan(**kv):
    """a plan over the finite array with a host result, its one step the fused kernel"""
    fin, _ = arrays()
    x = tree(fin)
    n = so.nframes(x)
    with env(SIGOPS_RSOS_MINGROUPS=1, **kv):
        assert steps_of(x) == ["k_rsos"]
        return so.Plan(so.ToChannels(x, NCH), (n, NCH), np.float64, (1, n), False), n


def execute(p, n, d, stream=None, **kv):
    """the plan's result over array d (replaced through the plan's own setter)"""
    out = np.full((n, NCH), -1.0, order="F")
    p.set_array(0, d)
    with env(**kv):
        p.execute(out.ctypes.data, stream)
    return out


def check_spoiled(got, want):
    bad_g, bad_w = ~np.isfinite(got), ~np.isfinite(want)
    for c in range(NCH):
        assert np.array_equal(bad_g[:, c], bad_w[:, c]), (c, np.nonzero(bad_g[:, c])[0][:3], np.nonzero(bad_w[:, c])[0][:3])
    assert relerr(got[~bad_w], want[~bad_w]) < 1e-9


def test_repeated_executes():
    fin, _ = arrays()
    want, _ = oracles()
    p, n = host_plan()
    try:
        out = np.empty((n, NCH), order="F")
        seen = []
        for _ in range(4):
            out[:] = -1.0
            p.execute(out.ctypes.data)
            seen.append(out.copy(order="F"))
    finally:
        p.close()
    for k in range(1, 4):
        assert np.array_equal(seen[k], seen[0]), k
    assert relerr(seen[0], want) < 1e-9


def fresh_finite():
    """a fresh plan's first execute over the finite array: its words the host armed"""
    if "fresh" not in _memo:
        p, n = host_plan()
        try:
            _memo["fresh"] = execute(p, n, arrays()[0])
        finally:
            p.close()
        assert np.isfinite(_memo["fresh"]).all() and relerr(_memo["fresh"], oracles()[0]) < 1e-9
    return _memo["fresh"]


def check_sequence(seq, outs):
    """f: finite everywhere and a fresh plan's result bit for bit; s: the oracle's set of non-finite outputs"""
    want_s = oracles()[1]
    for i, (k, got) in enumerate(zip(seq, outs)):
        if k == "f":
            assert np.isfinite(got).all(), (seq, i)
            assert np.array_equal(got, fresh_finite()), (seq, i)
        else:
            check_spoiled(got, want_s)


# Execute i of a plan uses set i & 1.  "fsfs" and its prefixes (both parities of the set index end a plan's life) keep finite
# data on one set and spoiled data on the other: they would pass on the host's fill of the first execute alone.  In the
# others a finite execute uses the set a spoiled one used LAST -- a word left at a range number puts NaN over it -- and a
# spoiled execute the set a finite one used last, behind a spoiled one on the other set.
@pytest.mark.parametrize("seq", ["fsfs", "f", "fs", "fsf", "sff", "fssf", "ssff", "sfsffs"])
def test_words_are_armed_again_after_use(seq):
    fin, bad = arrays()
    p, n = host_plan()
    try:
        outs = [execute(p, n, fin if k == "f" else bad) for k in seq]
    finally:
        p.close()
    check_sequence(seq, outs)


def test_another_stream():
    """two executes on the default stream, a device synchronize, then a second stream: its finite executes use the sets the
    spoiled ones of the default stream used last"""
    torch = pytest.importorskip("torch")
    fin, bad = arrays()
    side = torch.cuda.Stream()
    p, n = host_plan()
    try:
        outs = [execute(p, n, bad), execute(p, n, bad)]
        torch.cuda.synchronize()
        outs += [execute(p, n, fin if k == "f" else bad, side.cuda_stream) for k in "ffs"]
        torch.cuda.synchronize()
    finally:
        p.close()
    check_sequence("ssffs", outs)
    assert np.array_equal(outs[4], outs[0], equal_nan=True)


def test_graph_replay_keeps_its_fill_node():
    """four pieces of an `Append`, each an array through the resampler and the filter: four fused launches in a plan that
    is replayed from a captured graph.  Finite, spoiled (piece 1), finite: each three times into the same device result --
    direct, capture, replay."""
    torch = pytest.importorskip("torch")
    n = 150_000

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t()

    fins = [arrays(n, 50 + k)[0] for k in range(4)]
    spoiled = arrays(n, 51)[1]
    kids = [tree(a) for a in fins]
    want_f = np.concatenate([oracles(n, 50 + k)[0] for k in range(4)])
    want_s = np.concatenate([oracles(n, 50 + k)[k == 1] for k in range(4)])
    dfin, dbad = [dev(a) for a in fins], dev(spoiled)
    x = so.Append(*[tree(a) for a in dfin])
    nout = so.nframes(x)
    assert nout == sum(so.nframes(k) for k in kids)
    out_t = torch.empty((NCH, nout), dtype=torch.float64, device="cuda")
    out = out_t.t()
    with env(SIGOPS_RSOS_MINGROUPS=1):
        plan = so.Plan(so.ToChannels(x, NCH), (nout, NCH), np.float64, (out.stride(0), out.stride(1)), True)
    stream = torch.cuda.current_stream().cuda_stream
    try:
        assert [s["name"] for s in plan.steps()].count("k_rsos") == 4, plan.steps()
        first = None
        for leaf, want in ((dfin[1], want_f), (dbad, want_s), (dfin[1], want_f)):
            plan.set_array(1, leaf)
            before = plan.counters()
            for _ in range(3):
                out_t.fill_(-1.0)
                plan.execute(out.data_ptr(), stream)
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                if want is want_f:
                    first = got if first is None else first
                    assert np.isfinite(got).all() and np.array_equal(got, first)
                    assert relerr(got, want) < 1e-9
                else:
                    check_spoiled(got, want)
            after = plan.counters()
            assert after["graph_captures"] > before["graph_captures"] and after["graph_replays"] > before["graph_replays"], after
        plan.check()
    finally:
        plan.close()


@pytest.mark.parametrize("switch", ["SIGOPS_RSOS_NO_FIXUP", "SIGOPS_SOS_NOPOISON"])
def test_opt_outs_arm_their_words_themselves(switch):
    """the switches are read by every execute.  Without the fix-up launch k_sos_poison reads the words and arms nothing;
    without the words nobody reads any.  Expected, from the tests of the switches (test_gpu_rsos_nonfinite.py: finite data
    is untouched by them; test_gpu_iir_fused.py: the kernel's own set begins at a block of 16 outputs, at or in front of
    the reference's first non-finite output, and it is a superset while the words are kept): that, and a fresh plan's
    first execute -- whose words the host armed -- bit for bit."""
    fin, bad = arrays()
    want_f, want_s = oracles()
    fresh = {}
    for k, d in (("f", fin), ("s", bad)):
        p, n = host_plan()
        try:
            fresh[k] = execute(p, n, d, **{switch: 1})
        finally:
            p.close()
    p, n = host_plan()
    try:
        outs = [execute(p, n, fin if k == "f" else bad, **{switch: 1}) for k in "fsf"]
        # ... and back on the default path, which arms both sets again
        outs += [execute(p, n, fin if k == "f" else bad) for k in "sff"]
    finally:
        p.close()
    for k, got in zip("fsf", outs):
        assert np.array_equal(got, fresh[k], equal_nan=True), k
    assert np.isfinite(outs[0]).all() and relerr(outs[0], want_f) < 1e-9
    bad_g, bad_w = ~np.isfinite(outs[1]), ~np.isfinite(want_s)
    assert not bad_g[:, [0, 1, 3, 4, 5, 6]].any()
    for c in (2, 7):
        s, w = int(np.nonzero(bad_g[:, c])[0][0]), int(np.nonzero(bad_w[:, c])[0][0])
        assert s % 16 == 0 and w - 32 < s <= w, (c, s, w)
        if switch == "SIGOPS_RSOS_NO_FIXUP":
            assert bad_g[s:, c].all()
    ok = ~(bad_g | bad_w)
    assert relerr(outs[1][ok], want_s[ok]) < 1e-9
    check_sequence("sff", outs[3:])  # (the second finite execute uses the set the spoiled one used)
    assert np.array_equal(outs[4], outs[0])
