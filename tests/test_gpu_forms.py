"""Every form of the resampler and of the IIR, and every way of executing a plan, on small inputs against the CPU oracle.

csrc/stages.cpp picks a stage's kernel by falling down a ladder ("Forms and how to force them"); the rest of the
suite reaches each rung only at the shape whose size selects it.  Here ONE small input per case goes down a whole ladder:
every rung is forced with the switch that skips the rungs above it, named by its step (`Plan.steps()`), and held to the
oracle and to the other rungs of the case.  Then the executor's corpus of small trees (tests/forms_corpus.py) is executed
three times per plan (direct launches, graph capture, replay) and under the switches that change scheduling only.

Bounds (the project's own, none derived from the code under test), norm-wise over the whole result and BLOCKWISE -- the
largest relative error over blocks of 1024 frames across all channels, the metric of
test_gpu_iir_fused.py::test_loud_then_quiet_with_a_local_tolerance: noise keeps every block at full level, so a lone bad
sample at a tile, chunk or period edge counts sqrt(N / 1024) times more than in the whole-result norm:

    resamplers, Float64     1e-9  (test_gpu_rsos.py header)        1e-8 blockwise
    filters, Float64        1e-10 (test_gpu_iir_fused.py header)   1e-9 blockwise (the ratio that test uses)
    anything Float32        1e-6                                   2e-6 blockwise (test_gpu_rsos_f32m.py)
    two rungs of one Float64 case   1e-11
    k_sos_exact in Float64  bit-equal (test_gpu_fences.py)

Found with this file: the chunked forms of a third-order high-pass at 20 Hz (poles clustered at z = 1) were 3e-11 ... 6e-11
from the oracle and 7e-11 from k_rsos and the one-chunk form (two rungs: 1e-11), because M = A^L was squared in Float64 on the
host; formed in long double and rounded once (csrc/stages.cpp matpow) every rung of that case is within 1e-12 of the others.

`SIGOPS_RECORD_RELERR=<file>`: the observed maxima per (ladder, rung, dtype) go to that file and the table of observed
(step name, launches) to forms_rungs.txt beside it (profiles/r11/)."""
import atexit
import functools
import hashlib
import os

import numpy as np
import pytest

import sigops_amd as so
import oracle_bridge as ob
from oracle_bridge import oracle_semantics, oracle_sink
from comb_ref import comb
from cumsum_ref import cumsum_ref
from sampleat_ref import sampleat_np
from forms_corpus import POS, ResultView, at_seed, corpus, env, seed_starts
# the ladders' tables and trees (tools/plan_fingerprint.py --ladders walks the same ones)
from forms_corpus import (A_CASES, A_LADDER, CHUNKS, F32, F64, FILTERS, I_CASES, I_LADDER, N_LADDER, NFRAMES, R_CASES, RS_SWITCHES, SOS_SWITCHES,
                          _I1, arbitrary_tree, filter_rungs, filter_tree, resampler_rungs, resampler_tree, rung_env)
from forms_corpus import filter_id as _iid, resampler_id as _rid

pytestmark = pytest.mark.gpu

BLOCK = 1024


# ---- metrics and the record -------------------------------------------------------------------------------------------
def norm_err(got, want):
    a, b = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (nb if nb > 0 else 1.0))


def block_err(got, want):
    """the largest relative error over whole blocks of 1024 frames (all channels), and over the last 1024 frames"""
    a, b = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    n = a.shape[0]
    if n < BLOCK:
        return norm_err(a, b)
    nb = n // BLOCK
    cut = lambda v: np.concatenate([v[:nb * BLOCK].reshape(nb, BLOCK, -1), v[n - BLOCK:].reshape(1, BLOCK, -1)])  # noqa: E731
    d, w = np.linalg.norm(cut(a) - cut(b), axis=(1, 2)), np.linalg.norm(cut(b), axis=(1, 2))
    return float((d / np.where(w > 0, w, 1.0)).max())


def record(ladder, rung, dt, metric, value):
    """the largest value seen per (ladder, rung, dtype, metric), written with oracle_bridge's record at exit"""
    if not os.environ.get("SIGOPS_RECORD_RELERR"):
        return
    if not ob._RELERR_LOG:
        atexit.register(ob._relerr_dump)
    key = "forms %s %s %s [%s]" % (ladder, rung, metric, np.dtype(dt).name)
    old = ob._RELERR_LOG.get(key, (0.0, 0))
    ob._RELERR_LOG[key] = (max(old[0], float(value)), old[1] + 1)


def bounds(kind, dt):
    """(norm-wise, blockwise) against the oracle"""
    if np.dtype(dt) == F32:
        return 1e-6, 2e-6
    return {"resample": (1e-9, 1e-8), "filter": (1e-10, 1e-9)}[kind]


RUNGS_TWO = 1e-11  # two rungs of one Float64 case

STAGE_STEPS = ("k_resample_periodic", "k_resample_rows", "k_resample_arb", "k_resample_tiled2", "k_resample_tiled", "k_resample",
               "k_rsos", "k_sos", "k_sos_exact")


def run_host(tree, dt=None, nexec=1):
    """the tree sunk into a NaN-filled planar host result by a fresh plan: (values, (stage step's name, launches), the
    bytes after each execute, counters)"""
    v = ResultView(tree, dt=dt, where="host")
    v.clear()
    plan = v.plan()
    try:
        shots = []
        for _ in range(nexec):
            plan.execute(v.ptr)
            shots.append(v.bytes())
        steps = [(s["name"], s["launches"]) for s in plan.steps()]
        stage = [s for s in steps if s[0] in STAGE_STEPS]
        return v.array(), (stage[0] if stage else None), shots, plan.counters(), steps
    finally:
        plan.close()


def walk(ladder, kind, tree, want, rungs, switches, dt):
    """one input down a ladder: per rung the step, the figures against the oracle, whether the rung is LIVE for this case
    (its step or its bytes differ from every rung before it), and the largest difference between two rungs"""
    rows, outs = [], []
    for rung, kv in rungs:
        with rung_env(switches, kv):
            got, step, shots, _, steps = run_host(tree)
        row = {"rung": rung, "step": step, "steps": steps, "shape": got.shape, "dtype": got.dtype, "nan": bool(np.isnan(got).any()),
               "norm": norm_err(got, want), "block": block_err(got, want), "equal": bool(np.array_equal(got, want)),
               "live": not any(o["step"] == step and b == shots[0] for o, b in zip(rows, outs)), "sha": hashlib.sha256(shots[0]).hexdigest()}
        row["two"] = max([norm_err(got, np.frombuffer(b, dtype=got.dtype).reshape(got.shape)) for b in outs] + [0.0])
        print("%-9s %-5s %-22s x%-2d norm %.2e block %.2e two %.2e %s" % (ladder, rung, step[0] if step else None, step[1] if step else 0,
                                                                          row["norm"], row["block"], row["two"], "" if row["live"] else "(as a rung above)"))
        record(ladder, rung, dt, "normwise", row["norm"])
        record(ladder, rung, dt, "blockwise", row["block"])
        record(ladder, rung, dt, "between rungs", row["two"])
        rows.append(row)
        outs.append(shots[0])  # (planar: frames x channels in C order)
    return rows


def hold(rows, kind, want, dt, exact=()):
    """what every rung of a case owes: the oracle's shape and type, no NaN, the bounds; `exact`: rungs that owe its bits"""
    nb, bb = bounds(kind, dt)
    for r in rows:
        assert r["step"] is not None, (r["rung"], r["steps"])
        assert r["shape"] == want.shape and r["dtype"] == want.dtype, r["rung"]
        assert not r["nan"], r["rung"]
        assert r["norm"] <= nb, (r["rung"], r["step"], r["norm"])
        assert r["block"] <= bb, (r["rung"], r["step"], r["block"])
        if np.dtype(dt) == F64:
            assert r["two"] <= RUNGS_TWO, (r["rung"], r["step"], r["two"])
            if r["rung"] in exact:
                assert r["equal"], (r["rung"], r["norm"])


def skip_cap(rows):
    """at most half of a ladder's rungs may change nothing for a case"""
    assert 2 * sum(not r["live"] for r in rows) <= len(rows), [(r["rung"], r["step"], r["live"]) for r in rows]


# ---- 1. the resampler ladder (tables and trees: forms_corpus.py) ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def resampler_case(case):
    fi, fo, nout, nch, dt, window = case
    x = resampler_tree(case)
    want = oracle_sink(x)
    assert want.shape == (nout, nch) and want.dtype == dt and np.isfinite(want).all()
    rows = walk("resample", "resample", x, want, resampler_rungs(case), RS_SWITCHES, dt)
    return rows, want.shape, want.dtype


@functools.lru_cache(maxsize=None)
def arbitrary_case(case):
    fi, fo, nout, nch, dt = case
    x = arbitrary_tree(case)
    want = oracle_sink(x)
    assert want.shape == (nout, nch) and want.dtype == dt and np.isfinite(want).all()
    return walk("arbitrary", "resample", x, want, A_LADDER, RS_SWITCHES, dt), want.shape, want.dtype


class _Shape:
    def __init__(self, shape, dtype):
        self.shape, self.dtype = shape, dtype


@pytest.mark.parametrize("case", R_CASES, ids=_rid)
def test_resampler_ladder(case):
    """a rational rate down the ladder: 32-row MFMA tiles, 16-row tiles, the row kernel's MFMA and scalar paths,
    k_resample_tiled2, k_resample_tiled, k_resample"""
    rows, shape, dtype = resampler_case(case)
    hold(rows, "resample", _Shape(shape, dtype), case[4])
    skip_cap(rows)
    by = {r["rung"]: r for r in rows}
    if case[:5] == (44100, 16000, 7257, 4, F32):  # (a long period: R0 is the 16-row form -- the 32-row one has no instantiation)
        assert by["R0"]["step"][0] == "k_resample_periodic" and by["R2"]["step"][0] == "k_resample_rows", [(r["rung"], r["step"]) for r in rows]
    assert by["R6"]["step"][0] == "k_resample", by["R6"]["step"]


@pytest.mark.parametrize("case", A_CASES, ids=_rid)
def test_arbitrary_rate_ladder(case):
    """a rate without a period: the persistent k_resample_arb, k_resample_tiled2, k_resample_tiled, k_resample"""
    rows, shape, dtype = arbitrary_case(case)
    hold(rows, "resample", _Shape(shape, dtype), case[4])
    skip_cap(rows)
    assert [r["step"][0] for r in rows][-1] == "k_resample"


# ---- 2. the IIR ladder (tables and trees: forms_corpus.py) ------------------------------------------------------------
I_NAMES = {"I0": "k_rsos", "I1": "k_sos", "I3": "k_sos", "I4": "k_sos_exact", "I5": "k_sos", **{"I2_%d" % c: "k_sos" for c in CHUNKS}}


@functools.lru_cache(maxsize=None)
def filter_case(case):
    f, nch, dt = case
    x = filter_tree(case)
    want = oracle_sink(x)
    assert want.shape == (NFRAMES, nch) and want.dtype == dt and np.isfinite(want).all()
    rows = walk("filter", "filter", x, want, filter_rungs(case), SOS_SWITCHES, dt)
    xn = x | so.Normpower
    wantn = oracle_sink(xn)
    assert wantn.shape == want.shape and np.isfinite(wantn).all()
    return rows, walk("filter|norm", "filter", xn, wantn, N_LADDER, SOS_SWITCHES, dt)


@pytest.mark.parametrize("case", I_CASES, ids=_iid)
def test_iir_ladder(case):
    """a plain filter down its ladder: one pass of k_rsos, the three passes of k_sos in every chunk regime, k_sos_onepass,
    k_sos_exact; and below a Normpower the fused pass, the exact block scan and the scan without it"""
    f, nch, dt = case
    rows, nrows = filter_case(case)
    want = _Shape((NFRAMES, nch), np.dtype(dt))
    hold(rows, "filter", want, dt, exact=("I4",))
    hold(nrows, "filter", want, dt)
    skip_cap(rows + nrows)
    by = {r["rung"]: r for r in rows}
    # the aligned tile steps move no chunk border and so no rounding (SosGeom::align_rows): I5 owes the bits of I1
    assert by["I5"]["sha"] == by["I1"]["sha"]
    for r in rows:
        assert r["step"][0] == I_NAMES[r["rung"]], (r["rung"], r["steps"])
        if r["rung"] == "I2_20032":  # one chunk: a single launch (per group of eight sections; three launches otherwise)
            assert r["step"][1] == (FILTERS[f][1] + 7) // 8, r["step"]


# ---- result views of the filter ---------------------------------------------------------------------------------------
VIEW_RUNGS = [r for r in I_LADDER if r[0] in ("I1", "I2_64", "I4", "I5")]


@functools.lru_cache(maxsize=None)
def view_case(view):
    """Bandstop 0.5-2 kHz on 5 channels into: a device tensor [nch][n + 37], the same from element 1 on (row starts off
    their 128-byte lines: align_rows gets a non-zero head), a Float32 result of the Float64 filter (the narrowing store).
    (The planar host result is test_iir_ladder's.)  Per rung: (rung, step, norm, block, bit-equal, pad kept, bytes)"""
    import torch

    nch, n, pad = 5, NFRAMES, 37
    x = filter_tree(("bandstop5", nch, F64))
    want = oracle_sink(x)
    rdt = F32 if view == "float32" else F64
    rows = []
    for rung, kv in VIEW_RUNGS:
        if view == "float32":
            res = np.full((n, nch), np.nan, dtype=F32, order="F")
            ptr, read, kept = res.ctypes.data, (lambda: res), (lambda: True)
        else:
            flat = torch.full((nch * (n + pad) + 1,), float("nan"), dtype=torch.float64, device="cuda")
            off = 1 if view == "device+1" else 0
            t = flat[off:off + nch * (n + pad)].view(nch, n + pad)
            ptr = t.data_ptr()
            read = lambda: np.asfortranarray(t[:, :n].t().cpu().numpy())  # noqa: E731
            kept = lambda: bool(torch.isnan(t[:, n:]).all()) and bool(torch.isnan(flat[:off]).all()) and bool(torch.isnan(flat[off + nch * (n + pad):]).all())  # noqa: E731
        with rung_env(SOS_SWITCHES, kv):
            p = so.Plan(so.ToChannels(x, nch), (n, nch), rdt, (1, n) if view == "float32" else (1, n + pad), view != "float32")
            try:
                p.execute(ptr, torch.cuda.current_stream().cuda_stream)
                p.check(torch.cuda.current_stream().cuda_stream)
                step = [(s["name"], s["launches"]) for s in p.steps() if s["name"] in STAGE_STEPS][0]
            finally:
                p.close()
        got = read()
        w = want.astype(rdt)
        rows.append({"rung": rung, "step": step, "nan": bool(np.isnan(got).any()), "norm": norm_err(got, w), "block": block_err(got, w),
                     "equal": bool(np.array_equal(got, w)), "kept": kept(), "bytes": got.tobytes(), "shape": got.shape, "dtype": got.dtype})
        print("view %-9s %-6s %-12s norm %.2e block %.2e" % (view, rung, step[0], rows[-1]["norm"], rows[-1]["block"]))
        record("filter view " + view, rung, rdt, "normwise", rows[-1]["norm"])
        record("filter view " + view, rung, rdt, "blockwise", rows[-1]["block"])
    return rows


@pytest.mark.parametrize("view", ["device", "device+1", "float32"])
def test_iir_result_views(view):
    rows = view_case(view)
    rdt = F32 if view == "float32" else F64
    nb, bb = bounds("filter", rdt)
    by = {r["rung"]: r for r in rows}
    for r in rows:
        assert r["step"][0] == I_NAMES[r["rung"]], r["step"]
        assert r["shape"] == (NFRAMES, 5) and r["dtype"] == rdt and not r["nan"], r["rung"]
        assert r["kept"], (r["rung"], "wrote outside the result")
        assert r["norm"] <= nb and r["block"] <= bb, (r["rung"], r["norm"], r["block"])
    if rdt == F64:
        assert by["I4"]["equal"]
        for r in rows:
            assert norm_err(np.frombuffer(r["bytes"]), np.frombuffer(by["I1"]["bytes"])) <= RUNGS_TWO, r["rung"]
    # rows off their lines or on them, the aligned steps move no rounding
    assert by["I5"]["bytes"] == by["I1"]["bytes"]


# ---- 3. execute modes over the executor's corpus ------------------------------------------------------------------------
CORPUS = corpus()
EXACT = {"array_plus_one", "cut_after_until", "pad_zero_after", "pad_cycle", "pad_mirror", "pad_lastframe_array", "mix_65_channels",
         "reverse_channels", "padded_mix", "padded_amplify", "addchannel_extend", "select_channel", "offset_append_sum",
         "float32_append_pad", "sub_div", "negate", "strided_array", "gain_db", "empty_signal"}  # test_gpu_parity.py
# Float64 bound against the oracle of the trees beyond tests/cases.py, from the test named beside each in forms_corpus.py
# (0: bit-equal); every other tree: test_gpu_parity.py's 1e-9.  A Float32 result of a Float64 tree: the oracle's values
# rounded once, 1e-7 (test_gpu_parity.py::test_float64_filter_into_float32_result); Float32 trees: 1e-6.
TOL = {"append3_three_pass": 1e-9, "append3_one_pass": 1e-9, "rsos_f64": 1e-9, "rsos_f32_result": 1e-9, "rsos_two_arrays": 1e-9,
       "three_windows": 1e-9, "exact_cascade": 0, "state_pass": 1e-9, "resample_rows": 1e-9, "resample_fixups": 1e-9}
INTENDED = {"append3_three_pass", "append3_one_pass", "three_windows", "sine_source_batch"}  # appended filtered children
OWN_REFERENCE = {  # nodes the oracle does not have: their NumPy definitions, bit for bit (test_gpu_comb.py, _cumsum.py, _sampleat.py)
    "sample_at_array": lambda a: sampleat_np(a[0], POS),
    "sample_at_tree": lambda a: sampleat_np(a[0], cumsum_ref(np.abs(POS) / 4000), wrap=True),
    "comb": lambda a: comb(a[0], 257, 0.7),
    "cumsum_two_chunks": lambda a: cumsum_ref(a[0]),
}
SCHEDULING = ("SIGOPS_SINGLE_STREAM", "SIGOPS_NO_GRAPH", "SIGOPS_NO_WINDOW_ALIAS")
# (tree, switch): the sentence of DESIGN.md that documents a different rounding -- the comparison is then 1e-11
DOCUMENTED = {}
starts = functools.lru_cache(maxsize=None)(seed_starts)


def execute_three_times(tree, view, graph=True):
    """a fresh plan executed three times into the same result, NaN-filled before each: the bytes (all three equal) and the
    values; the counters are held to what the plan is eligible for (executor.cpp plan_execute: a device result, device
    leaves, four steps or more -> direct launches, a capture, a replay)"""
    import torch

    v = ResultView(tree, **view)
    plan = v.plan()
    try:
        stream = torch.cuda.current_stream().cuda_stream
        shots = []
        for _ in range(3):
            v.clear()
            plan.execute(v.ptr, stream)
            plan.check(stream)
            shots.append(v.bytes())
        assert shots[1] == shots[0], "the captured graph's first launch differs from the direct launches"
        assert shots[2] == shots[0], "the replay differs from the direct launches"
        nodes = plan.lowered.nodes
        eligible = graph and v.is_dev and len(plan.steps()) >= 4 and all(nodes[i].i0 for i, _ in plan.lowered.array_nodes)
        c = plan.counters()
        got = (c["direct_executes"], c["graph_captures"], c["graph_replays"])
        assert got == ((1, 1, 1) if eligible else (3, 0, 0)), (got, eligible, [s["name"] for s in plan.steps()])
        return shots[0], v.array()
    finally:
        plan.close()


@pytest.mark.parametrize("k", range(len(CORPUS)), ids=[c[0] for c in CORPUS])
def test_execute_modes(k):
    name, build, view, kv = CORPUS[k]
    with at_seed(starts()[k], host=True) as made:
        host_tree = build()
        leaves = list(made)
    # the oracle (or the NumPy definition) on the same data from host leaves
    try:
        if name in OWN_REFERENCE:
            want = OWN_REFERENCE[name](leaves)
        elif name in INTENDED:
            with oracle_semantics("intended"):
                want = oracle_sink(host_tree)
        else:
            want = oracle_sink(host_tree)
    except so.ErrorException:
        want = None
    with env(**kv):
        with at_seed(starts()[k]):
            tree = build()
        if want is None:  # a tree the reference refuses is refused by the engine
            with pytest.raises(so.ErrorException):
                execute_three_times(tree, view)
            return
        ref, got = execute_three_times(tree, view)
        others = {}
        for sw in SCHEDULING:
            with env(**{sw: 1}):
                others[sw] = execute_three_times(tree, view, graph=sw != "SIGOPS_NO_GRAPH")
    # against the reference
    rdt = np.dtype(view.get("dt") or want.dtype)
    assert got.shape == want.shape and got.dtype == rdt
    assert np.array_equal(np.isnan(got), np.isnan(want.astype(rdt)))
    if name in EXACT or name in OWN_REFERENCE or (TOL.get(name) == 0 and rdt == F64):
        err, tol = (0.0 if np.array_equal(got, want) else max(norm_err(got, want), 1e-300)), 0.0
    elif rdt == F32 and want.dtype == F64:
        err, tol = norm_err(got, want.astype(F32)), 1e-7
    else:
        err, tol = norm_err(got, want), (1e-6 if rdt == F32 else TOL.get(name, 1e-9))
    print("%s: %.3e against the reference (bound %g)" % (name, err, tol))
    record("corpus", "default", rdt, "normwise", err)
    assert err <= tol, (name, err, tol)
    # the switches change scheduling and who writes a window, not arithmetic
    for sw, (b, a) in others.items():
        if (name, sw) in DOCUMENTED:
            assert norm_err(a, got) <= 1e-11, (name, sw, norm_err(a, got))
        else:
            assert b == ref, (name, sw, norm_err(a, got))


@pytest.mark.parametrize("which", ["R0", "I1"])
def test_ladder_heads_execute_three_times(which):
    """rung R0 of every resampler case and rung I1 of every filter case: three executes of one plan, bit-identical"""
    cases = [(resampler_tree(c), {}) for c in R_CASES] if which == "R0" else [(filter_tree(c), _I1) for c in I_CASES]
    for tree, kv in cases:
        with rung_env(RS_SWITCHES + SOS_SWITCHES, kv):
            _, step, shots, counters, _ = run_host(tree, nexec=3)
        assert shots[0] == shots[1] == shots[2], step
        assert counters["direct_executes"] == 3 and counters["graph_captures"] == 0, counters  # (a host result: never a graph)


# ---- evidence that a rung is the rung ---------------------------------------------------------------------------------
BY_VALUE_ONLY = """by value only (step names cannot tell them apart):
  the row kernel's scalar and MFMA paths (R2 / R3: k_resample_rows both)
  16-row and 32-row tiles where both fit (R0 / R1: k_resample_periodic both)
  the three chunk regimes of k_sos beyond "1 launch or 3" (I2_*)
by geometry only: I5 (SIGOPS_SOS_NOALIGN moves no rounding: it owes the bits of I1, on rows on and off their cache lines)"""


def test_every_rung_was_the_rung():
    """over all cases: the six resampler steps are all seen, every rung is live (its step or its bytes differ from the rungs
    above it) for at least one case, and the table of observed (step, launches) is written beside the recorded maxima"""
    table, live = [], {}

    def note(ladder, cid, rows):
        for r in rows:
            live[r["rung"]] = live.get(r["rung"], False) or r["live"]
            table.append("%-11s %-36s %-9s %-22s %2d%s" % (ladder, cid, r["rung"], r["step"][0], r["step"][1], "" if r["live"] else "  (as a rung above)"))

    seen = set()
    for c in R_CASES:
        rows = resampler_case(c)[0]
        note("resample", _rid(c), rows)
        seen |= {r["step"][0] for r in rows}
    for c in A_CASES:
        rows = arbitrary_case(c)[0]
        note("arbitrary", _rid(c), rows)
        seen |= {r["step"][0] for r in rows}
    for c in I_CASES:
        rows, nrows = filter_case(c)
        note("filter", _iid(c), rows)
        note("filter|norm", _iid(c), nrows)
    for view in ("device", "device+1", "float32"):
        for r in view_case(view):
            table.append("%-11s %-36s %-9s %-22s %2d" % ("filter view", "bandstop5-5xfloat64-" + view, r["rung"], r["step"][0], r["step"][1]))
    assert seen >= {"k_resample_periodic", "k_resample_rows", "k_resample_arb", "k_resample_tiled2", "k_resample_tiled", "k_resample"}, seen
    # (I5 is live by geometry: test_iir_result_views runs it on rows off their 128-byte lines and holds it to I1's bits)
    dead = sorted(r for r, ok in live.items() if not ok and r != "I5")
    assert not dead, dead
    path = os.environ.get("SIGOPS_RECORD_RELERR")
    if path:
        with open(os.path.join(os.path.dirname(os.path.abspath(path)), "forms_rungs.txt"), "w") as f:
            f.write("ladder      case                                 rung      step                   launches\n" + "\n".join(table) + "\n\n" + BY_VALUE_ONLY + "\n")
