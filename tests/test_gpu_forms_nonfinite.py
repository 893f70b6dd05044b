"""Non-finite samples on every rung of the ladders of tests/test_gpu_forms.py, in windows, and on re-execution.

The promise ("The reference's set of non-finite outputs"): a resampler's output is non-finite exactly
where its own taps reach a non-finite sample, a filter's channel from its first such output to its end, no other channel is
touched, and everything else is the oracle's value.  The tests that held it run at sizes that select the default form of each
ladder; here the small spoiled inputs of tests/forms_corpus.py (what the oracle makes of them: tests/test_forms_nonfinite_host.py)
go down every rung:

1. every rung of the four ladders: the step test_gpu_forms.py saw for the rung (profiles/r11/forms_rungs.txt), the engine's set
   against the oracle's, clean channels finite, the values outside both sets within test_gpu_forms.py's bounds;
2. six filters behind `After(30000) | Until(5001)` and one `so.stream`: with `SIGOPS_NO_WARM_START` the oracle's set; by default
   a filter that starts from rest a decay time before the window does not see the frames before that start;
3. one plan per form executed on finite, spoiled, finite, otherwise spoiled, finite data: the bookkeeping is armed again;
4. more (tile, group) entries than the periodic resampler's list holds, and the execute behind it.

Found with this file: the one-pass k_sos (`SIGOPS_SOS_ONEPASS`, rung I3) had no poison pass: its look-back reaches `kt` tiles
of 2 048 frames, and a channel was finite again that far behind a NaN (1 569 to 41 571 of the oracle's non-finite outputs
missing per case of test_iir_ladder_spoiled; test_rearm_after_a_spoiled_execute[I3] and the window cases saw the same).
k_sos_poison_onepass (csrc/k_small.hip) now writes NaN behind the first tile whose published end state is non-finite.
Measured where no document stated the relation: k_resample_tiled, k_resample and the one-pass k_sos are equal to the oracle;
k_resample_tiled2 and k_resample_arb return a few samples more, within the bound of tests/test_gpu_resampler_nonfinite.py.
Behind a warm start the engine does NOT return the reference's set: see `window_rule`.

`SIGOPS_RECORD_NONFINITE=<file>`: the table of (ladder, case, rung, step, sizes of the two sets, relation) goes to that file
(profiles/r16/forms_nonfinite.txt)."""
import atexit
import functools
import os

import numpy as np
import pytest

import sigops_amd as so
from oracle_bridge import oracle_semantics, oracle_sink
from forms_corpus import (A_CASES, A_LADDER, BS, F64, FILTERS, FW_CASES, I_CASES, I_LADDER, LP, N_LADDER, NAN, INF, OVERFLOW_CASE, R_CASES,
                          RS_SWITCHES, SOS_SWITCHES, ResultView, arbitrary_tree_spoiled, filter_data_spoiled, filter_rungs,
                          filter_tree_spoiled, filter_window_tree, forgotten, ladder_noise, overflow_tree, resampler_rungs,
                          resampler_tree, resampler_tree_spoiled, rs_nf_cap, rung_env, spoiled)
from forms_corpus import filter_id as _iid, resampler_id as _rid
from test_gpu_forms import I_NAMES, RUNGS_TWO, STAGE_STEPS, block_err, bounds, norm_err, run_host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = []  # the record's lines


def _dump():
    path = os.environ.get("SIGOPS_RECORD_NONFINITE")
    if path and TABLE:
        with open(path, "w") as f:
            f.write("%-13s %-36s %-9s %-20s %8s %8s  %s\n" % ("ladder", "case", "rung", "step", "oracle", "engine", "relation") + "\n".join(TABLE) + "\n")


atexit.register(_dump)


def note(ladder, cid, rung, step, n_want, n_got, relation):
    TABLE.append("%-13s %-36s %-9s %-20s %8d %8d  %s" % (ladder, cid, rung, step, n_want, n_got, relation))


@functools.lru_cache(maxsize=None)
def expected_steps():
    """(ladder, case, rung) -> the step test_gpu_forms.py observed on the clean input: the planner does not look at the data"""
    table = {}
    for line in open(os.path.join(ROOT, "profiles", "r11", "forms_rungs.txt")):
        p = line.split()
        if len(p) >= 5 and p[0] in ("resample", "arbitrary", "filter", "filter|norm") and p[1] != "view" and p[4].isdigit():
            table[(p[0], p[1], p[2])] = p[3]
    return table


# ---- the relation of two sets ---------------------------------------------------------------------------------------------
def groups_of(mask_col):
    return set((np.nonzero(mask_col)[0] // 16).tolist())


def relation(bad_g, bad_w, plants):
    """"equal"; "superset +k": contains the oracle's set, stays within the aligned groups of 16 outputs that set touches plus one
    on either side, and holds at most 32 samples more per plant (the bound tests/test_gpu_resampler_nonfinite.py states for the
    periodic kernel alone); anything else is named for what is wrong with it"""
    if np.array_equal(bad_g, bad_w):
        return "equal"
    if (bad_w & ~bad_g).any():
        c = int(np.nonzero((bad_w & ~bad_g).any(axis=0))[0][0])
        return "MISSES %d of the oracle's (channel %d from %d)" % ((bad_w & ~bad_g).sum(), c, np.nonzero(bad_w[:, c] & ~bad_g[:, c])[0][0])
    for c in range(bad_g.shape[1]):
        if not bad_w[:, c].any() and bad_g[:, c].any():
            return "TOUCHES channel %d (%d samples from %d)" % (c, bad_g[:, c].sum(), np.nonzero(bad_g[:, c])[0][0])
        allowed = set()
        for g in groups_of(bad_w[:, c]):
            allowed |= {g - 1, g, g + 1}
        extra = int(bad_g[:, c].sum() - bad_w[:, c].sum())
        if not groups_of(bad_g[:, c]) <= allowed or extra > 32 * sum(1 for p in plants if p[0] == c):
            return "WIDER by %d in channel %d (groups %s)" % (extra, c, sorted(groups_of(bad_g[:, c]) - allowed)[:4])
    return "superset +%d" % int(bad_g.sum() - bad_w.sum())


def masked(got, want):
    """both results with every sample that either holds non-finite set to 0"""
    both = np.isfinite(got) & np.isfinite(want)
    return np.where(both, got, 0), np.where(both, want, 0)


# the relation each step owes.  Equality is documented for the periodic kernel with its fix-up, the row kernel's own redo,
# k_rsos_fixup, the three-pass k_sos ("K2 reproduced it before") and the sequential k_sos_exact.  For the rest no document
# stated it, and what is asserted is what was measured (profiles/r16/forms_nonfinite.txt): k_resample_tiled and k_resample
# (R5, R6, A2, A3: each output from its own taps) and the one-pass k_sos (I3, with its poison pass) are equal;
# k_resample_tiled2 (R4, A1: a lane's two outputs share one window) returns 1 to 9 samples more and k_resample_arb (A0) 6 to
# 21, both within the bound tests/test_gpu_resampler_nonfinite.py states for the periodic kernel alone (`relation`).
OWES = {"k_resample_periodic": "equal", "k_resample_rows": "equal", "k_rsos": "equal", "k_sos": "equal", "k_sos_exact": "equal",
        "k_resample_tiled2": "superset", "k_resample_tiled": "equal", "k_resample": "equal", "k_resample_arb": "superset"}


def walk_spoiled(ladder, kind, cid, tree, want, plants, rungs, switches, dt):
    """one spoiled input down a ladder: everything that is wrong, as a list of sentences (empty: nothing)"""
    wrong, outs = [], []
    bad_w = ~np.isfinite(want)
    planted = {p[0] for p in plants}
    nb, bb = bounds(kind, dt)
    for rung, kv in rungs:
        with rung_env(switches, kv):
            got, step, _, _, steps = run_host(tree)
        if step is None:
            wrong.append("%s: no stage step in %s" % (rung, steps))
            continue
        name = step[0]
        say = lambda s: wrong.append("%s %s: %s" % (rung, name, s))  # noqa: E731
        if got.shape != want.shape or got.dtype != want.dtype:
            say("shape or type %s %s" % (got.shape, got.dtype))
            continue
        bad_g = ~np.isfinite(got)
        rel = relation(bad_g, bad_w, plants)
        note(ladder, cid, rung, name, bad_w.sum(), bad_g.sum(), rel)
        g0, w0 = masked(got, want)
        en, eb = norm_err(g0, w0), block_err(g0, w0)
        two = 0.0
        for o in outs:
            a, b = masked(got, o)
            two = max(two, norm_err(a, b))
        outs.append(got)
        print("%-11s %-5s %-20s oracle %6d engine %6d %-14s norm %.2e block %.2e two %.2e" % (ladder, rung, name, bad_w.sum(), bad_g.sum(), rel, en, eb, two))
        if expected_steps().get((ladder, cid, rung)) != name:
            say("the clean input's step is %s" % expected_steps().get((ladder, cid, rung)))
        if ladder == "filter" and name != I_NAMES[rung]:
            say("not %s" % I_NAMES[rung])
        if rel != "equal" and not (OWES[name] == "superset" and rel.startswith("superset")):
            say("the set: %s (owed: %s)" % (rel, OWES[name]))
        if bad_g[:, [c for c in range(got.shape[1]) if c not in planted]].any() and bad_w.sum() < bad_w.size:
            say("a clean channel is not finite")
        if en > nb or eb > bb:
            say("outside the sets: norm %.3e (%g) block %.3e (%g)" % (en, nb, eb, bb))
        if np.dtype(dt) == F64 and two > RUNGS_TWO:
            say("%.3e from a rung above" % two)
    return wrong


# ---- 1. every rung of the four ladders on the spoiled inputs --------------------------------------------------------------
@pytest.mark.parametrize("case", R_CASES, ids=_rid)
def test_resampler_ladder_spoiled(case):
    x, plants = resampler_tree_spoiled(case)
    want = oracle_sink(x)
    assert (~np.isfinite(want)).any()
    wrong = walk_spoiled("resample", "resample", _rid(case), x, want, plants, resampler_rungs(case), RS_SWITCHES, case[4])
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("case", A_CASES, ids=_rid)
def test_arbitrary_rate_ladder_spoiled(case):
    x, plants = arbitrary_tree_spoiled(case)
    want = oracle_sink(x)
    assert (~np.isfinite(want)).any()
    wrong = walk_spoiled("arbitrary", "resample", _rid(case), x, want, plants, A_LADDER, RS_SWITCHES, case[4])
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("case", I_CASES, ids=_iid)
def test_iir_ladder_spoiled(case):
    """the last frame (channel 4 or 3) and frame 0 are part of the set; below a Normpower everything is NaN"""
    f, nch, dt = case
    x, plants = filter_tree_spoiled(case)
    want = oracle_sink(x)
    assert (~np.isfinite(want)).any()
    wrong = walk_spoiled("filter", "filter", _iid(case), x, want, plants, filter_rungs(case), SOS_SWITCHES, dt)
    wantn = oracle_sink(x | so.Normpower)
    assert np.isnan(wantn).all()
    wrong += walk_spoiled("filter|norm", "filter", _iid(case), x | so.Normpower, wantn, plants, N_LADDER, SOS_SWITCHES, dt)
    assert not wrong, "\n".join(wrong)


# ---- 2. windows behind a non-finite sample ----------------------------------------------------------------------------------
def run_profiled(tree):
    """(values, stage step's name, the bytes the plan's steps read and write) of a fresh plan with a planar host result"""
    v = ResultView(tree, where="host")
    v.clear()
    plan = v.plan()
    try:
        plan.set_profiling(True)
        plan.execute(v.ptr)
        steps = plan.steps()
        stage = [s["name"] for s in steps if s["name"] in STAGE_STEPS]
        return v.array(), (stage[0] if stage else None), sum(s["algorithmic_bytes"] for s in steps)
    finally:
        plan.close()


def window_rule(tree, cold_want, warm_want, kv, say, label):
    """the tree under `SIGOPS_NO_WARM_START` (the oracle's set and values) and by default.  By default a filter that starts from
    rest a decay time before the first frame anybody reads (fewer bytes than under the switch) owes the oracle's result on the
    input whose plant at frame 100 is 0.0; one that starts at frame 0 owes the oracle's.  Returns whether it warm-started."""
    nb, bb = bounds("filter", F64)

    def hold(got, want, what):
        bad_g, bad_w = ~np.isfinite(got), ~np.isfinite(want)
        if not np.array_equal(bad_g, bad_w):
            say("%s: the set is not the oracle's: %s against %s per channel" % (what, bad_g.sum(axis=0).tolist(), bad_w.sum(axis=0).tolist()))
        g0, w0 = masked(got, want)
        if norm_err(g0, w0) > nb or block_err(g0, w0) > bb:
            say("%s: norm %.3e block %.3e" % (what, norm_err(g0, w0), block_err(g0, w0)))
        return bad_g

    with rung_env(SOS_SWITCHES, {**kv, "SIGOPS_NO_WARM_START": 1}):
        cold, step, cold_bytes = run_profiled(tree)
    with rung_env(SOS_SWITCHES, {**kv, "SIGOPS_NO_WARM_START": None}):
        got, step2, warm_bytes = run_profiled(tree)
    warm = warm_bytes < cold_bytes  # (a warm-started filter may take another form: k_rsos from frame 0, k_sos from its later start)
    hold(cold, cold_want, "from frame 0")
    bad = hold(got, warm_want if warm else cold_want, "warm-started" if warm else "by default (no warm start)")
    note("filter window", label[0], label[1], step2 or "-", (~np.isfinite(cold_want)).sum(), bad.sum(),
         "warm start (%d of %d bytes): the set of the input without its plant at frame 100" % (warm_bytes, cold_bytes) if warm else "no warm start: equal")
    return warm


@functools.lru_cache(maxsize=None)
def window_case(case):
    x, plants = filter_window_tree(case)
    want = oracle_sink(x)
    less = oracle_sink(filter_window_tree(case, forgotten(plants))[0])
    bad, badl = ~np.isfinite(want), ~np.isfinite(less)
    assert bad[:, 0].all() and bad[:, 1].all() and bad[2000:, 3].all() and bad.sum() == 2 * 5001 + 3001
    assert not badl[:, 0].any() and badl[:, 1].all() and badl[2000:, 3].all() and badl.sum() == 5001 + 3001
    wrong, warm = [], {}
    for rung, kv in filter_rungs(case):
        warm[rung] = window_rule(x, want, less, kv, lambda s: wrong.append("%s: %s" % (rung, s)), (_iid(case) + "-window", rung))
    print(case[0], "warm-started:", [r for r, w in warm.items() if w])
    return wrong, warm


@pytest.mark.parametrize("case", FW_CASES, ids=_iid)
def test_filter_window_behind_a_non_finite_sample(case):
    wrong, warm = window_case(case)
    assert not wrong, "\n".join(wrong)
    if case[0] == "highpass_slow":  # (its decay length is longer than the signal)
        assert not any(warm.values()), warm


def test_most_filters_warm_start_on_the_three_pass_rung():
    """the rule for warm-started plans is not asserted on nothing"""
    warm = [c[0] for c in FW_CASES if window_case(c)[1]["I1"]]
    assert len(warm) >= 4, warm


def test_stream_blocks_behind_a_non_finite_sample():
    """`so.stream` over bandstop5 on the 40 000 frames in blocks of 10 000, the three-pass form: under `SIGOPS_NO_WARM_START` the
    blocks are the whole sink's frames, whose set is the oracle's; by default each block follows the rule of the windows"""
    case = ("bandstop5", 5, F64)
    x, plants = filter_window_tree(case, window=False)
    want = oracle_sink(x)
    less = oracle_sink(filter_window_tree(case, forgotten(plants), window=False)[0])
    kv = dict(I_LADDER)["I1"]
    nb, bb = bounds("filter", F64)
    with rung_env(SOS_SWITCHES, {**kv, "SIGOPS_NO_WARM_START": 1}):
        whole = so.sink(x, so.Array)
        blocks = list(so.stream(x, 10000, so.Array))
    got = np.concatenate(blocks, axis=0)
    assert [b.shape[0] for b in blocks] == [10000] * 4
    assert np.array_equal(~np.isfinite(whole), ~np.isfinite(want)) and np.array_equal(~np.isfinite(got), ~np.isfinite(want))
    g0, w0 = masked(got, want)
    assert norm_err(g0, w0) <= nb and block_err(g0, w0) <= bb
    with rung_env(SOS_SWITCHES, {**kv, "SIGOPS_NO_WARM_START": None}):
        blocks = list(so.stream(x, 10000, so.Array))
    wrong, nwarm = [], 0
    for k, b in enumerate(blocks):
        blk = x | so.After(10000 * k * so.frames) | so.Until(10000 * so.frames) if k else x | so.Until(10000 * so.frames)
        lo = 10000 * k
        say = lambda s: wrong.append("block %d: %s" % (k, s))  # noqa: E731
        warm = window_rule(blk, want[lo:lo + 10000], less[lo:lo + 10000], kv, say, ("bandstop5-5xfloat64-stream-block%d" % k, "I1"))
        nwarm += warm
        owed = less if warm else want
        if not np.array_equal(~np.isfinite(b), ~np.isfinite(owed[lo:lo + 10000])):
            say("the streamed block's set: %s per channel" % (~np.isfinite(b)).sum(axis=0).tolist())
        g0, w0 = masked(b, owed[lo:lo + 10000])
        if norm_err(g0, w0) > nb or block_err(g0, w0) > bb:
            say("values %.3e %.3e" % (norm_err(g0, w0), block_err(g0, w0)))
    assert not wrong, "\n".join(wrong)
    assert nwarm >= 2, nwarm  # (the blocks at 20 000 and 30 000 start a decay length of 4 096 behind frame 8 192)


# ---- 3. re-arming: finite, spoiled, finite, otherwise spoiled, finite on one plan -------------------------------------------
def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t()


def rearm(build, A, B, B2, kv, switches, kind, step=None, intended=False, pad=0, nexec=1):
    """`build(leaves)` is the tree; A, B, B2: lists of host arrays, one per leaf.  A plan with device leaves and a device result
    is executed (`nexec` times each) on A, B, A, B2, A: on A the bytes of a fresh plan's result and finite, on B and B2 the
    oracle's set and the oracle's values outside it.  Returns the plan's counters."""
    import torch

    stream = torch.cuda.current_stream().cuda_stream
    nb, bb = bounds(kind, F64)
    with oracle_semantics("intended" if intended else "reference"):
        want = [oracle_sink(build(d)) for d in (A, B, B2)]
    assert np.isfinite(want[0]).all()
    bad_b, bad_b2 = ~np.isfinite(want[1]), ~np.isfinite(want[2])
    assert bad_b.any() and bad_b2.any() and (bad_b2.any(axis=0) & ~bad_b.any(axis=0)).any()  # (B2 spoils what B left clean)
    leaves = {k: [dev(a) for a in d] for k, d in (("A", A), ("B", B), ("B2", B2))}
    with rung_env(switches, kv):
        v = ResultView(build(leaves["A"]), where="dev", pad=pad)
        plan = v.plan()
        try:
            for _ in range(nexec):
                v.clear()
                plan.execute(v.ptr, stream)
                plan.check(stream)
            fresh = v.bytes()
            names = [s["name"] for s in plan.steps()]
        finally:
            plan.close()
        assert step is None or step in names, names
        assert np.isfinite(v.array()).all() and norm_err(v.array(), want[0]) <= nb
        plan = v.plan()
        try:
            for i, k in enumerate(("A", "B", "A", "B2", "A")):
                for j, leaf in enumerate(leaves[k]):
                    plan.set_array(j, leaf)
                for e in range(nexec):
                    v.clear()
                    plan.execute(v.ptr, stream)
                    plan.check(stream)
                    if k == "A":
                        assert v.bytes() == fresh, "execute %d.%d on finite data differs from a fresh plan's" % (i + 1, e)
                        continue
                    got, w = v.array(), want[1 if k == "B" else 2]
                    bad_g, bad_w = ~np.isfinite(got), ~np.isfinite(w)
                    assert np.array_equal(bad_g, bad_w), "execute %d.%d: %s against the oracle's %s per channel" % (
                        i + 1, e, bad_g.sum(axis=0).tolist(), bad_w.sum(axis=0).tolist())
                    g0, w0 = masked(got, w)
                    assert norm_err(g0, w0) <= nb and block_err(g0, w0) <= bb, (i + 1, e, norm_err(g0, w0), block_err(g0, w0))
            return plan.counters(), names
        finally:
            plan.close()


R_REARM = (44100, 48000, 21770, 8, F64, False)
I_REARM = ("bandstop5", 5, F64)
REARM = {"R0": ("k_resample_periodic", dict(resampler_rungs(R_REARM))["R0"]), "R2": ("k_resample_rows", dict(resampler_rungs(R_REARM))["R2"]),
         **{r: (I_NAMES[r], dict(I_LADDER)[r]) for r in ("I0", "I1", "I2_64", "I2_4096", "I3")}}


@pytest.mark.parametrize("form", list(REARM))
def test_rearm_after_a_spoiled_execute(form):
    step, kv = REARM[form]
    if form[0] == "R":
        fi, fo, nout, nch, dt, _ = R_REARM
        a = ladder_noise(1000 + nch, 20001, nch, dt)
        b = spoiled(a, resampler_tree_spoiled(R_REARM)[1])                      # channels 0, 3 and 7
        b2 = spoiled(a, [(1, 3000, INF), (5, 12000, NAN), (5, 20000, NAN)])     # channels 1 and 5
        build = lambda d: so.Signal(d[0], fi * so.Hz) | so.ToFramerate(fo * so.Hz)  # noqa: E731
        rearm(build, [a], [b], [b2], kv, RS_SWITCHES, "resample", step)
    else:
        a = ladder_noise(3000 + 5, 20001, 5, F64)
        b = filter_data_spoiled(I_REARM)                                        # channels 0, 1, 3 and 4
        b2 = spoiled(a, [(2, 4095, NAN), (4, 0, INF)])                          # channel 2, and channel 4 from its first frame on
        build = lambda d: so.Signal(d[0], 44.1 * so.kHz) | FILTERS["bandstop5"][0]()  # noqa: E731
        rearm(build, [a], [b], [b2], kv, SOS_SWITCHES, "filter", step)


@pytest.mark.parametrize("batch", [0, 1], ids=["append3_three_pass", "append3_one_pass"])
def test_rearm_the_batched_forms(batch):
    """the corpus entries append3_three_pass and append3_one_pass: three filtered children of an `Append`, their own copies of
    the bookkeeping"""
    sizes = (5001, 7777, 12345)
    A = [ladder_noise(5000 + k, n, 2, F64) for k, n in enumerate(sizes)]
    B = [A[0], spoiled(A[1], [(0, 3000, NAN)]), A[2]]
    B2 = [spoiled(A[0], [(1, 5000, INF)]), A[1], spoiled(A[2], [(1, 0, NAN)])]
    build = lambda d: so.Append(*[so.Signal(a, 44.1 * so.kHz) | BS() for a in d])  # noqa: E731
    rearm(build, A, B, B2, {"SIGOPS_RSOS_BATCH": batch}, SOS_SWITCHES + ("SIGOPS_RSOS_BATCH",), "filter", intended=True)


def test_rearm_a_plan_replayed_as_a_graph():
    """built as the corpus entry three_windows: three filters of different orders under an `Append`, four steps, device leaves
    and a device result -- executed directly, captured, replayed"""
    spec = ((9999, 2), (12001, 4), (8000, 6))
    A = [ladder_noise(6000 + k, n, 2, F64) for k, (n, _) in enumerate(spec)]
    B = [A[0], spoiled(A[1], [(0, 6000, NAN)]), A[2]]
    B2 = [spoiled(A[0], [(1, 0, INF)]), A[1], spoiled(A[2], [(1, 7999, NAN)])]
    build = lambda d: so.Append(*[so.Signal(a, 44.1 * so.kHz) | LP(order=o) | so.Ramp(5 * so.ms) for a, (_, o) in zip(d, spec)])  # noqa: E731
    counters, names = rearm(build, A, B, B2, {}, SOS_SWITCHES, "filter", intended=True, pad=5, nexec=3)
    print(counters, names)
    assert len(names) == 4, names
    assert counters["graph_captures"] >= 1 and counters["graph_replays"] >= 3, counters


# ---- 4. more entries than the periodic resampler's list holds ----------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["every-fourth-frame", "first-half"])
def test_overflow_of_the_fixup_list(half):
    fi, fo, nout, nch, dt, _ = OVERFLOW_CASE
    x, plants = overflow_tree(half)
    clean = ladder_noise(1000 + nch, 20001, nch, dt)
    want, want_clean = oracle_sink(x), oracle_sink(resampler_tree(OVERFLOW_CASE))
    bad_w = ~np.isfinite(want)
    # the list takes one entry per (tile of 32 rows = 4 periods of 2 outputs x 8 channels, group of 16 outputs of the period)
    tiles = len(set((np.nonzero(bad_w[:, 5])[0] // 8).tolist()))
    assert tiles > rs_nf_cap(), (tiles, rs_nf_cap())
    nb, bb = bounds("resample", dt)
    with rung_env(RS_SWITCHES, {}):
        v = ResultView(resampler_tree(OVERFLOW_CASE), where="host")
        plan = v.plan()
        try:
            v.clear()
            plan.execute(v.ptr)
            fresh = v.bytes()
        finally:
            plan.close()
        v = ResultView(x, where="host")
        plan = v.plan()
        try:
            v.clear()
            plan.execute(v.ptr)
            got = v.array()
            assert [s["name"] for s in plan.steps() if s["name"] in STAGE_STEPS] == ["k_resample_periodic"], plan.steps()
            plan.set_array(0, clean)
            v.clear()
            plan.execute(v.ptr)
            after, after_bytes = v.array(), v.bytes()
        finally:
            plan.close()
    bad_g = ~np.isfinite(got)
    note("resample", _rid(OVERFLOW_CASE) + ("-overflow-half" if half else "-overflow"), "R0", "k_resample_periodic", bad_w.sum(), bad_g.sum(),
         "%d tiles against a list of %d: %s" % (tiles, rs_nf_cap(), relation(bad_g, bad_w, plants[:1] * len(plants))))
    assert not (bad_w & ~bad_g).any(), "misses %d of the oracle's" % (bad_w & ~bad_g).sum()
    others = [c for c in range(nch) if c != 5]
    assert not bad_g[:, others].any()
    assert norm_err(got[:, others], want[:, others]) <= nb and block_err(got[:, others], want[:, others]) <= bb
    if half:  # beyond the reach of the last plant (and the kernel's own group of 16 outputs and one more) the oracle's values
        last = int(np.nonzero(bad_w[:, 5])[0][-1])
        first_ok = (last // 16 + 2) * 16
        assert not bad_g[first_ok:, 5].any(), np.nonzero(bad_g[first_ok:, 5])[0][:4] + first_ok
        assert norm_err(got[first_ok:], want[first_ok:]) <= nb and block_err(got[first_ok:], want[first_ok:]) <= bb
    # the execute behind it: the list is empty again
    assert np.isfinite(after).all() and after_bytes == fresh
    assert norm_err(after, want_clean) <= nb
