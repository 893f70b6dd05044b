"""The fused resampler + IIR kernel (k_rsos.hip) over filter designs x rate pairs: tests/rsos_matrix.py's matrix, CORE x every
rate joined with every design x four rates.  Nothing here forces a geometry: a case takes what the planner picks for a real rate
pair and a real design under `SIGOPS_RSOS_MINGROUPS=1`, `SIGOPS_RSOS_RANGES=4`, asserts that the fused step is what ran, and
holds the result to

  * the CPU oracle, 1e-9 norm-wise (test_gpu_rsos.py's bound) and 1e-8 over blocks of 1024 frames (test_gpu_forms.py's metric
    and bound: one bad sample at a range boundary must not hide in the norm);
  * the engine's two kernels (`SIGOPS_NO_RSOS=1`), 1e-11;
  * each form's opt-out, at the bound the form's own file asserts: folded against `SIGOPS_RSOS_NOFOLD=1` (different bytes, below
    1e-12, four MFMAs fewer per block; a plan the gate declined: the same bytes), projected warm-up against
    `SIGOPS_RSOS_NOWPROJ=1` (1e-11), the chain wave's 4x4x4 shape against `SIGOPS_RSOS_CHAIN16=1` (the same bytes).

Input: 8 channels of seeded normal noise, Fortran order, an odd number of frames -- 20 001, or as many as give four ranges each
longer than its warm-up (`wp` of `plan.rsos_geometry()`), at most 100 000.  A pair the fused step does not run is an entry of
rsos_matrix.DECLINED with its reason, asserted NOT fused and held to the oracle on the two kernels (and on what runs by default:
the resampler's kernel and the plain filter's one-pass form); a pair that would need more than 100 000 frames is declared too, and
held on 20 001 frames, where its ranges are shorter than their warm-up.

A check, not a tautology: with the largest entry of the folded table (of V) off by 1e-6 of its size in a scratch build, every folded
(projected) CORE case at 16 -> 48 and 9.6 -> 16 kHz missed its opt-out bound -- 8e-8 .. 4e-5 against 1e-12 (2e-10 .. 1.5e-7 against
1e-11) -- and the two kernels' 1e-11; all 18 folded cases and 24 of the 26 projected ones missed the oracle's 1e-9 as well (the two
hp1@0.0005, 2.6e-10, did not: one entry of 12 x 12 400).

`SIGOPS_RECORD_RSOS_MATRIX=<file>` writes one line per case with its geometry and measured errors (profiles/r18/rsos_matrix.txt)."""
import os
import re
import time
from fractions import Fraction

import numpy as np
import pytest

import sigops_amd as so
import rsos_matrix as rm
from oracle_bridge import oracle_sink, relerr
from test_gpu_forms import block_err
from test_gpu_rsos import F, env
from test_rsos_fold_host import fold_tables

pytestmark = pytest.mark.gpu

N0 = 20_001
NMAX = 100_000
BASE = dict(SIGOPS_RSOS_MINGROUPS=1, SIGOPS_RSOS_RANGES=4)
ORACLE, ORACLE_BLOCK, TWO_KERNELS = 1e-9, 1e-8, 1e-11
FOLD_CEILING, WPROJ_CEILING = 1e-12, 1e-11                # test_gpu_rsos_fold.py, test_gpu_rsos_wproj.py
F32_ORACLE, F32_BLOCK, F32_VS_F64_PRODUCTS = 1e-6, 2e-6, 3e-7  # test_gpu_rsos_f32m.py / test_gpu_rsos.py
MATRIX = rm.matrix()
T0 = [None]
_rows = {}

LINE = re.compile(r"resampler \+ IIR fused \(k_rsos\): (\d+) ranges of (\d+) periods \(\+(\d+) warm-up\), (\d+) groups of (\d+) ch x (\d+) ranges, "
                  r"ks=(\d+) ring=(\d+) chunk=(\d+) waves=(\d+) cyc=(-?\d+)")
AMP = re.compile(r"folded block (taken|declined): amp ([0-9.eE+\-infa]+)")


def record(name, **kv):
    """SIGOPS_RECORD_RSOS_MATRIX=<file>: the rows so far rewritten there (how profiles/r18/rsos_matrix.txt was made)"""
    _rows[name] = kv
    path = os.environ.get("SIGOPS_RECORD_RSOS_MATRIX")
    if not path:
        return
    cols = ["n", "nsec", "ng", "ks", "waves", "cyc", "wp", "pr", "ranges", "own", "fold", "amp", "wproj", "wproj_frames", "oracle", "oracle_block",
            "two_kernels", "vs_nofold", "vs_nowproj", "note"]
    with open(path, "w") as f:
        f.write("k_rsos over designs x rates (tests/test_gpu_rsos_matrix.py): geometry and measured errors per case; bounds: oracle 1e-9, "
                "oracle_block 1e-8, two_kernels 1e-11, vs_nofold 1e-12, vs_nowproj 1e-11 (Float32 rows: 1e-6, 2e-6, 3e-7)\n")
        f.write(f"{len(_rows)} rows in {time.time() - T0[0]:.0f} s wall\n")
        f.write("case " + " ".join(cols) + "\n")
        for k, v in _rows.items():
            f.write(k + " " + " ".join(_fmt(v.get(c)) for c in cols) + "\n")


def _fmt(v):
    if v is None:
        return "-"
    if isinstance(v, float):
        return f"{v:.3g}" if v >= 1 else f"{v:.2e}"
    return str(v).replace(" ", "_")


@pytest.fixture(autouse=True)
def _clock():
    if T0[0] is None:
        T0[0] = time.time()


# ---- inputs, trees, plans ------------------------------------------------------------------------------------------------
_noise = {}


def noise(n, nch=8, dt=np.float64):
    key = (n, nch, np.dtype(dt).name)
    if key not in _noise:
        if len(_noise) > 24:
            _noise.clear()
        _noise[key] = F(np.random.default_rng(1800 + nch).standard_normal((n, nch)).astype(dt))
    return _noise[key]


def source(rate, n, nch=8, dt=np.float64, mix=False):
    src = so.Signal(noise(n, nch, dt), rate[0] * so.kHz)
    if mix:  # a fused sine: what puts groups of two and four channels on sixteen waves
        src = so.Mix(so.Signal(so.sin, ω=1 * so.kHz), src) | so.Until(n * so.frames)
    return src


def run(x, dtype=np.float64, **kv):
    """(result, facts) of a fresh plan with a host result; facts: steps, counters, geometry"""
    n, nch = so.nframes(x), so.nchannels(x)
    out = np.empty((n, nch), dtype=dtype, order="F")
    with env(**{**BASE, **kv}):
        p = so.Plan(so.ToChannels(x, nch), (n, nch), dtype, (1, n), False)
        try:
            p.execute(out.ctypes.data)
            facts = dict(steps=[s["name"] for s in p.steps()], **p.counters(), **{"g_" + k: v for k, v in p.rsos_geometry().items()})
        finally:
            p.close()
    return out, facts


def planned(x, capfd, dtype=np.float64, **kv):
    """what the planner says of `x` (no execute): facts as `run`'s, and the fields of its k_rsos line"""
    n, nch = so.nframes(x), so.nchannels(x)
    capfd.readouterr()
    with env(**{**BASE, **kv, "SIGOPS_DEBUG_PLAN": 1}):
        p = so.Plan(so.ToChannels(x, nch), (n, nch), dtype, (1, n), False)
        try:
            facts = dict(steps=[s["name"] for s in p.steps()], **p.counters(), **{"g_" + k: v for k, v in p.rsos_geometry().items()})
        finally:
            p.close()
    facts.update(parse(capfd.readouterr().err))
    return facts


def parse(log):
    out = dict(fused_line=False, own="own taps" in log, amp=None, gate=None)
    m = LINE.search(log)
    if m:
        v = [int(t) for t in m.groups()]
        out.update(fused_line=True, ranges=v[0], pr=v[1], wp=v[2], groups=v[3], ct=v[4], rgs=v[5], ks=v[6], ring=v[7], waves=v[9], cyc=v[10])
    m = AMP.search(log)
    if m:
        out.update(gate=m.group(1), amp=float(m.group(2)))
    return out


def frames_for(wp, M):
    """input frames that give four ranges, each longer than its warm-up of wp periods of M frames: odd"""
    return max(N0, ((4 * wp + 8) * M) | 1)


_probe = {}


def probe(case, capfd, nch=8, dt=np.float64, mix=False, **kv):
    """the planner's choice for a case, from a plan over N0 frames (what it depends on -- rate, design, channels, type -- is
    the key; none of ks, waves, cyc, wp, M depends on the length), and the frames the case runs on"""
    key = (rm.case_id(case), nch, np.dtype(dt).name, mix, tuple(sorted(kv.items())))
    if key not in _probe:
        rate, d = case
        f = planned(d.tree(source(rate, N0, nch, dt, mix), rate), capfd, dt, **kv)
        # (k_rsos alone in the steps is not enough: behind a resampler kernel it is the plain filter's one-pass form)
        f["fused"] = f["fused_line"] and f["steps"] == ["k_rsos"]
        f["n"] = frames_for(f["g_wp"], f["g_M"]) if f["fused"] else N0
        if f["fused"]:
            f["ng"] = int(Fraction(f["g_M"]) * Fraction(str(rate[1])) / Fraction(str(rate[0])) / 16)
        _probe[key] = f
    return _probe[key]


def two_kernels(x, dtype=np.float64):
    out, f = run(x, dtype, SIGOPS_NO_RSOS=1, SIGOPS_RS_NO_F32MFMA=1 if dtype == np.float32 else None)
    assert "k_rsos" not in f["steps"]
    return out


def errors(got, want, two, dt=np.float64):
    return dict(oracle=float(relerr(got, want)), oracle_block=block_err(got, want), two_kernels=float(relerr(got, two)))


def hold(e, dt=np.float64):
    if np.dtype(dt) == np.float32:
        assert e["oracle"] < F32_ORACLE and e["oracle_block"] < F32_BLOCK and e["two_kernels"] < F32_VS_F64_PRODUCTS, e
    else:
        assert e["oracle"] < ORACLE and e["oracle_block"] < ORACLE_BLOCK and e["two_kernels"] < TWO_KERNELS, e


def fused_case(name, case, capfd, nch=8, dt=np.float64, mix=False, forms=True, **kv):
    """one (rate, design) on the fused kernel: identified, held to the oracle, the two kernels and every form's opt-out;
    the row is recorded before anything is asserted.  -> (result, row)"""
    rate, d = case
    pb = probe(case, capfd, nch, dt, mix, **kv)
    n = pb["n"]
    x = d.tree(source(rate, n, nch, dt, mix), rate)
    f = planned(x, capfd, dt, **kv)
    got, c = run(x, dt, **kv)
    want = oracle_sink(x)
    assert want.dtype == np.dtype(dt) and got.shape == want.shape
    e = errors(got, want, two_kernels(x, dt), dt)
    row = dict(n=n, nsec=len(d.sos(rate)[0]), ng=pb.get("ng"), ks=f.get("ks"), waves=f.get("waves"), cyc=f.get("cyc"), wp=f.get("wp"), pr=f.get("pr"),
               ranges=f.get("ranges"), own=int(f["own"]), fold=c["fold"], amp=f["amp"], wproj=c["wproj"], wproj_frames=c["g_wproj_frames"], **e)
    vs = {}
    if forms and c["steps"] == ["k_rsos"] and f["fused_line"]:
        if c["fold"] == 1 or f["gate"] == "declined":
            vs["nofold"], vs["c_nofold"] = run(x, dt, SIGOPS_RSOS_NOFOLD=1, **kv)
            if c["fold"] == 1:
                row["vs_nofold"] = float(relerr(got, vs["nofold"]))
        if c["wproj"] == 1:
            vs["nowproj"], vs["c_nowproj"] = run(x, dt, SIGOPS_RSOS_NOWPROJ=1, **kv)
            row["vs_nowproj"] = float(relerr(got, vs["nowproj"]))
        vs["chain16"], vs["c_chain16"] = run(x, dt, SIGOPS_RSOS_CHAIN16=1, **kv)
    record(name, **row)
    print(name, {k: _fmt(v) for k, v in row.items()})

    assert c["steps"] == ["k_rsos"] and f["fused_line"], (c["steps"], "the fused step did not run")
    assert n <= NMAX and n % 2 == 1 and n % 16 != 0
    assert f["ranges"] >= 4 and f["pr"] > f["wp"] and (f["pr"], f["wp"]) == (c["g_pr"], c["g_wp"]), f
    assert (f["ks"], f["waves"], f["cyc"], f["wp"]) == (pb["ks"], pb["waves"], pb["cyc"], pb["wp"])  # (the probe's length did not matter)
    hold(e, dt)
    if not forms:
        return got, row
    if c["fold"] == 1:
        assert f["gate"] == "taken" and f["amp"] <= 256.0  # (as the planner prints it: three digits)
        assert vs["c_nofold"]["fold"] == 0 and vs["c_nofold"]["fused_mfmas_per_block"] == c["fused_mfmas_per_block"] + 4
        assert not np.array_equal(got, vs["nofold"])  # (the folded block ran: another association of the same sums)
        assert row["vs_nofold"] < FOLD_CEILING
    elif f["gate"] == "declined":  # the gate's decision: the unfolded kernel, bit for bit
        assert f["amp"] >= 256.0 and vs["c_nofold"]["fold"] == 0
        assert np.array_equal(got, vs["nofold"])
    else:  # never offered to the gate: the geometry's (sixteen waves, a Float32 ring or result)
        assert f["gate"] is None and (f["waves"] == 16 or np.dtype(dt) == np.float32), f
    if c["wproj"] == 1:
        assert f["wp"] * c["g_M"] + 4 * f["ks"] <= 16384 and c["g_wproj_frames"] > 0
        assert vs["c_nowproj"]["wproj"] == 0
        assert row["vs_nowproj"] < WPROJ_CEILING
    assert c["chain4"] == 1 and vs["c_chain16"]["chain4"] == 0
    assert np.array_equal(got, vs["chain16"])
    return got, row


# ---- the matrix --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MATRIX, ids=rm.case_id)
def test_matrix(case, capfd):
    rate, d = case
    why = rm.declined(case)
    name = rm.case_id(case)
    if not why:
        _, row = fused_case(name, case, capfd)
        assert rm.GEOMETRY[rm.rate_id(rate)] == (row["ng"], 4 * row["ks"], probe(case, capfd)["g_M"])
        if d in rm.CORE:
            assert rm.CORE_WP[(rm.rate_id(rate), d.name)] == row["wp"]
        return
    pb = probe(case, capfd)
    if why.startswith("too slow"):  # the fused step would take it, on more than NMAX frames: held on N0 frames whatever runs them
        assert pb["fused"] and pb["n"] > NMAX, pb
    else:
        assert not pb["fused"], (why, pb)
    x = d.tree(source(rate, N0), rate)
    got, c = run(x)
    e = errors(got, oracle_sink(x), two_kernels(x))
    record(name, n=N0, nsec=len(d.sos(rate)[0]), wp=pb.get("wp") if pb["fused"] else None, fold=c["fold"], wproj=c["wproj"], note="declined: " + why, **e)
    assert (c["steps"] == ["k_rsos"]) == why.startswith("too slow"), c["steps"]  # (the resampler's kernel runs on its own)
    hold(e)


def test_declined_within_its_cap():
    keys = {(rm.rate_id(r), d.name) for r, d in MATRIX}
    for (rid, name), why in rm.DECLINED.items():
        assert name == "*" or (rid, name) in keys, (rid, name)
        assert why.split(":")[0] in ("no super-period of whole blocks", "a window longer than 20 k-steps", "a warm-up that does not converge", "exact",
                                     "too slow for a small case", "the input ring does not hold the windows in flight"), why
    gone = [c for c in MATRIX if rm.declined(c)]
    assert 4 * len(gone) <= len(MATRIX), (len(gone), len(MATRIX))
    assert not [rm.case_id(c) for c in gone if c[0] in rm.HEADLINE_RATES and c[1] in rm.CORE]


# (ks, waves, cyc) of every fused case of the matrix
REACHED = {(13, 12, 1), (12, 8, 1), (12, 12, 1), (12, 12, 2)}


def test_instantiations_reached(capfd):
    """The (window k-steps, waves, phase groups per y wave) the matrix reaches, as the planner chooses them for 8 channels of
    Float64: cyc = ng / gcd(y waves, ng) with ten y waves (twelve and sixteen waves) or six (eight waves), and the rates give
    ng = 10 blocks per period (44.1 -> 48, 22.05 -> 24, 9.6 -> 16), 20 (22.05 -> 48), 3 (32 -> 48, 16 -> 48: eight waves) and 1 (x 2).

    rsos_instantiated() x {12, 13, 14, 16, 20} k-steps are 43 kernels.  Four are reached here and three more below:
    (13, 8, 5) and (12, 12, 0) in test_forced_instantiations, (13, 16, 1) in test_channels_and_float32.  Not reached:
      * ks = 14, 16, 20, all 27 of them: no pair of RATES has windows of 53 .. 80 slots.  The upsampling pairs fit 12 k-steps
        (13 where the resampler stage's table is trimmed: 38 taps + a span of 14); the downsampling pairs, whose windows are
        longer, decline (rsos_matrix.DECLINED; 48 -> 32 kHz would be ks = 20 on one block: its window fits, its ring does not).
      * (13, 12, 0): SIGOPS_RSOS_LDSTAPS=1 at 44.1 -> 48 -- table and ring do not fit together and the planner keeps the two kernels.
        (13, 12, 2), (13, 8, 0 / 1 / 2 / 3): 13 k-steps come from the ten-group table of 44.1 -> 48 alone: cyc is 1 or 5.
      * (12, 8, 0): SIGOPS_RSOS_NWAVES=8 with SIGOPS_RSOS_LDSTAPS=1.  (12, 8, 5): SIGOPS_RSOS_NWAVES=8 at 9.6 -> 16.
        (12, 8, 2), (12, 8, 3): six y waves and ng = 4 or 9, say: no pair of RATES.
      * (12, 16, 1): two or four channels with a fused step at a pair with 12 k-steps whose ng divides 10 (24 -> 48, 9.6 -> 16);
        test_channels_and_float32 runs 44.1 -> 48 (sixteen waves, 13 k-steps) and 32 -> 48 (ng = 3: eight waves)."""
    got = {}
    for case in MATRIX:
        if not rm.declined(case) or rm.declined(case).startswith("too slow"):
            pb = probe(case, capfd)
            got.setdefault((pb["ks"], pb["waves"], pb["cyc"]), set()).add(rm.rate_id(case[0]))
    print({k: sorted(v) for k, v in got.items()})
    assert set(got) == REACHED


@pytest.mark.parametrize("name", ["lp1@0.25", "bs3w", "bs6n"])
@pytest.mark.parametrize("switch, rate, tup", [("SIGOPS_RSOS_NWAVES", (44.1, 48.0), (13, 8, 5)), ("SIGOPS_RSOS_LDSTAPS", (24.0, 48.0), (12, 12, 0))])
def test_forced_instantiations(switch, rate, tup, name, capfd):
    """eight waves (44.1 -> 48 kHz: five phase groups per y wave) and the taps read from LDS (24 -> 48 kHz: at 44.1 kHz table and ring
    do not fit together and the planner keeps the two kernels), through the planner's own switches: one, three and six sections,
    held to the matrix's bounds"""
    case = (rate, rm.BY_NAME[name])
    kv = {switch: 8 if switch.endswith("NWAVES") else 1}
    _, row = fused_case(f"{switch[12:].lower()}/{rm.case_id(case)}", case, capfd, **kv)
    assert (row["ks"], row["waves"], row["cyc"]) == tup


# ---- the projection cap ------------------------------------------------------------------------------------------------
# first-order high-passes at 44.1 -> 48 kHz (Hz): warm-ups of 111 and 112 periods of 147 frames, 16 369 and 16 516 frames with the window
CAP_BELOW, CAP_ABOVE = 16.7, 16.6


@pytest.mark.parametrize("hz, projected", [(CAP_BELOW, True), (CAP_ABOVE, False)])
def test_projection_cap(hz, projected, capfd):
    rate = (44.1, 48.0)
    d = rm.Design(f"hp1@{hz}Hz", "highpass", ("butterworth", 1), (hz,), True)
    _, row = fused_case(f"cap/{d.name}", (rate, d), capfd)
    span = row["wp"] * 147 + 4 * row["ks"]
    print("span", span)
    assert (span <= 16384) == projected and row["wproj"] == int(projected)
    assert abs(span - 16384) < 2 * 147  # (the two nearest warm-up lengths)


# ---- the fold gate -----------------------------------------------------------------------------------------------------
def nearest_to_the_gate(rate):
    """(admitted, declined) designs of the grid nearest to amp = 256 at this rate, with their amp"""
    tab = np.zeros((1, 48, 16))
    amps = [(fold_tables(*d.sos(rate), tab)[2], d) for d in rm.DESIGNS]
    below = max((a for a in amps if a[0] <= 256.0), key=lambda a: a[0])
    above = min((a for a in amps if a[0] > 256.0), key=lambda a: a[0])
    return below, above


@pytest.mark.parametrize("rate", rm.HEADLINE_RATES, ids=rm.rate_id)
def test_fold_gate(rate, capfd):
    (a_in, d_in), (a_out, d_out) = nearest_to_the_gate(rate)
    print(f"nearest to the gate at {rm.rate_id(rate)}: {d_in.name} {a_in:.4g} admitted, {d_out.name} {a_out:.4g} declined")
    _, row = fused_case(f"gate/{rm.rate_id(rate)}/{d_in.name}", (rate, d_in), capfd)
    assert row["fold"] == 1 and abs(row["amp"] - a_in) <= 1e-2 * a_in and row["vs_nofold"] < FOLD_CEILING
    _, row = fused_case(f"gate/{rm.rate_id(rate)}/{d_out.name}", (rate, d_out), capfd)  # (bit-equal to the unfolded block: asserted there)
    assert row["fold"] == 0 and abs(row["amp"] - a_out) <= 1e-2 * a_out


# ---- fewer channels and Float32 ----------------------------------------------------------------------------------------
VARIANTS = {"ch2mix": dict(nch=2, mix=True), "ch4mix": dict(nch=4, mix=True), "ch3": dict(nch=3), "float32": dict(dt=np.float32)}


@pytest.mark.parametrize("d", rm.CORE, ids=lambda d: d.name)
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("rate", [(44.1, 48.0), (32.0, 48.0)], ids=rm.rate_id)
def test_channels_and_float32(rate, variant, d, capfd):
    kw = VARIANTS[variant]
    name = f"{variant}/{rm.case_id((rate, d))}"
    if variant != "float32":
        _, row = fused_case(name, (rate, d), capfd, **kw)
        if kw.get("mix") and rate == (44.1, 48.0):
            assert row["waves"] == 16
        return
    got, row = fused_case(name, (rate, d), capfd, **kw)
    assert got.dtype == np.float32
    x = d.tree(source(rate, row["n"], 8, np.float32), rate)
    ref, c = run(x, np.float32, SIGOPS_RSOS_NO_F32MFMA=1)
    assert c["steps"] == ["k_rsos"]
    assert relerr(got, ref) < F32_VS_F64_PRODUCTS


# ---- a window of the result --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", rm.CORE, ids=lambda d: d.name)
@pytest.mark.parametrize("rate", rm.HEADLINE_RATES, ids=rm.rate_id)
def test_window_inside_the_second_range(rate, d, capfd):
    """After(a) | Until(n) with `a` inside the whole plan's second range: the slice of the whole result, to 1e-11"""
    pb = probe((rate, d), capfd)
    x = d.tree(source(rate, pb["n"]), rate)
    pr, L = planned(x, capfd)["pr"], pb["ng"] * 16
    a, n = pr * L + L // 2 + 37, 4 * L + 1001
    assert pr * L < a < 2 * pr * L and a + n < so.nframes(x)
    whole, c = run(x)
    part, cw = run(x | so.After(a * so.frames) | so.Until(n * so.frames))
    err = float(relerr(part, whole[a:a + n]))
    record(f"window/{rm.case_id((rate, d))}", n=pb["n"], two_kernels=err, note=f"After({a})|Until({n}):{'+'.join(cw['steps'])}")
    assert c["steps"] == ["k_rsos"]
    assert part.shape == (n, 8) and err < TWO_KERNELS
