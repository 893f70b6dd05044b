"""The host side of tests/rsos_matrix.py's designs x rates, without a device:

  a. admission -- every design, at every rate pair it runs at, is inside what the Float64 DF2T cascade itself delivers: the
     recurrence of test_rsos_fold_host.py's block_maps over 8 192 frames of noise in Float64 against long double, 1e-10
     norm-wise, a tenth of what test_gpu_rsos_matrix.py holds the kernel to (the CPU oracle is such a Float64 recurrence);
  b. the folded tables (so_rsos_fold_tables) for every case, at the table shape (ng, kw) its rate gives on the device:
     E . T = D, the folded table against T[TIME] . Tap^T, the gate's decision against amp as defined -- and designs on both
     sides of the gate;
  c. the projection matrix (so_rsos_wproj_matrix) for CORE x every (ng, kw, M), at that design's wp on the device: V . x against
     the block walk, test_rsos_wproj_host.py's bound.

The (ng, kw, M) per rate and wp per CORE design are rsos_matrix.GEOMETRY / CORE_WP: read off the device, asserted there."""
import numpy as np
import pytest

import rsos_matrix as rm
from test_rsos_fold_host import LD, TIME, block_maps, fold_tables
from test_rsos_chain4_host import chain_blocks
from test_rsos_wproj_host import block_maps as walk_maps
from test_rsos_wproj_host import wproj_matrix

MATRIX = rm.matrix()
ADMISSION = 1e-10
NFRAMES = 8192


def cascades(designs, x, dt):
    """the DF2T cascades of `designs` [(sos, gain)] over x side by side, in dt: [frames][designs]"""
    nd = len(designs)
    co = np.zeros((6, 5, nd), dtype=dt)
    co[:, 0, :] = 1  # (sections a cascade does not have: y = x, exactly)
    g = np.zeros(nd, dtype=dt)
    for k, (sos, gain) in enumerate(designs):
        for f, r in enumerate(sos):
            co[f, :, k] = [r[0], r[1], r[2], r[4], r[5]]
        g[k] = gain
    s0 = [np.zeros(nd, dtype=dt) for _ in range(6)]
    s1 = [np.zeros(nd, dtype=dt) for _ in range(6)]
    y = np.empty((len(x), nd), dtype=dt)
    for t in range(len(x)):
        v = np.full(nd, x[t], dtype=dt)
        for f in range(6):
            b0, b1, b2, a1, a2 = co[f]
            xi = v
            v = s0[f] + b0 * xi
            s0[f] = s1[f] + b1 * xi - a1 * v
            s1[f] = b2 * xi - a2 * v
        y[t] = v * g
    return y


_admission = {}


def admission():
    """{(rate id, design name): Float64 against long double} for the issue's whole grid, the removed designs included"""
    if not _admission:
        cases = [(rate, d) for rate in rm.RATES for d in (rm.ALL_GRID if rate in rm.FULL_RATES else [c for c in rm.ALL_GRID if c.name in rm.CORE_NAMES])]
        x = np.random.default_rng(5).standard_normal(NFRAMES)
        des = [d.sos(rate) for rate, d in cases]
        yl = cascades(des, x.astype(LD), LD)
        y6 = cascades(des, x, np.float64)
        err = np.sqrt(((y6.astype(LD) - yl) ** 2).sum(axis=0) / (yl ** 2).sum(axis=0))
        for (rate, d), e in zip(cases, err):
            _admission[(rm.rate_id(rate), d.name)] = float(e)
    return _admission


def test_the_matrix_is_what_the_issue_lists():
    assert len(rm.RATES) == 14 and len(set(rm.RATES)) == 14 and set(rm.FULL_RATES) < set(rm.RATES)
    assert len(rm.ALL_GRID) == 24 + 9 + 24 + 4 + 4 and len(rm.BY_NAME) == len(rm.ALL_GRID)
    assert len(MATRIX) == len(rm.DESIGNS) * 4 - 1 + len(rm.CORE) * 10 and len(set(map(rm.case_id, MATRIX))) == len(MATRIX)
    assert {len(d.sos((44.1, 48.0))[0]) for d in rm.CORE} == {1, 2, 3, 4, 5, 6}
    assert {d.kind for d in rm.CORE} == {"lowpass", "highpass", "bandpass", "bandstop"} and {d.method[0] for d in rm.CORE} == {"butterworth", "chebyshev1"}
    for d in rm.ALL_GRID:
        assert 1 <= len(d.sos((44.1, 48.0))[0]) <= 6
    sos, _ = rm.BY_NAME["lp1@0.25"].sos((44.1, 16.0))  # (fmin = fs_out: the cutoff at a quarter of the rate, the pole at 0)
    assert len(sos) == 1 and abs(sos[0][4]) < 1e-15 and sos[0][5] == 0.0


@pytest.mark.parametrize("case", MATRIX, ids=rm.case_id)
def test_admission(case):
    e = admission()[(rm.rate_id(case[0]), case[1].name)]
    print(f"Float64 against long double: {e:.3e}")
    assert e <= ADMISSION


def test_what_the_admission_removed():
    """a design is left out of DESIGNS exactly where one of its rates misses the bound; the worst figures, for the record"""
    worst = {}
    for (rid, name), e in admission().items():
        worst[name] = max(worst.get(name, 0.0), e)
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:3]
    print("worst:", ", ".join(f"{k} {v:.2e}" for k, v in top))
    assert {n for n, e in worst.items() if not e <= ADMISSION} == set(rm.NOT_ADMITTED)
    for n, e in rm.NOT_ADMITTED.items():
        assert 0.5 * e <= worst[n] <= 2 * e, (n, worst[n])  # (the figure in its comment)
    assert [d.name for d in rm.DESIGNS] == [d.name for d in rm.ALL_GRID if d.name not in rm.NOT_ADMITTED]


# ---- b. folded tables ----------------------------------------------------------------------------------------------------
FUSED = [c for c in MATRIX if rm.rate_id(c[0]) in rm.GEOMETRY]


def random_table(ng, kw, seed):
    rng = np.random.default_rng(seed)
    tab = rng.standard_normal((ng, kw, 16)) / np.sqrt(kw)
    tab[:, :3, :] = 0.0
    return tab


@pytest.mark.parametrize("case", FUSED, ids=rm.case_id)
def test_folded_tables(case):
    rate, d = case
    ng, kw, _ = rm.GEOMETRY[rm.rate_id(rate)]
    sos, gain = d.sos(rate)
    ns = len(sos)
    tab = random_table(ng, kw, ns + ng)
    E, ft, amp, fold = fold_tables(sos, gain, tab)
    T, _, D, _ = block_maps(sos, gain)
    assert np.isfinite(amp) and fold == int(amp <= 256.0)
    assert not E[2 * ns:].any()
    scale = np.abs(D).sum(axis=1).max()
    got = E[: 2 * ns].astype(LD) @ T
    err = float(np.abs(got - D).max() / scale)
    want_amp = float((np.abs(E[: 2 * ns].astype(LD)) @ np.abs(T)).sum(axis=1).max() / scale)
    want = np.einsum("mt,gkt->gkm", T[TIME], tab.astype(LD))
    terr = float(np.abs(ft - want).max() / np.abs(want).max())
    print(f"amp {amp:.4g} fold {fold}  E.T - D: {err:.3e}  folded table: {terr:.3e}")
    assert abs(amp - want_amp) <= 1e-12 * want_amp
    assert err <= 1e-15 * amp
    assert terr <= 4e-16


@pytest.mark.parametrize("rate", rm.FULL_RATES, ids=rm.rate_id)
def test_both_sides_of_the_gate(rate):
    tab = np.zeros((1, 48, 16))
    amps = sorted((fold_tables(*d.sos(rate), tab)[2], d.name) for d in rm.DESIGNS)
    below, above = [a for a in amps if a[0] <= 256.0], [a for a in amps if a[0] > 256.0]
    assert len(below) >= 10 and len(above) >= 10
    print(f"nearest to the gate at {rm.rate_id(rate)}: {below[-1][1]} {below[-1][0]:.4g} admitted, {above[0][1]} {above[0][0]:.4g} declined")
    core = [fold_tables(*d.sos(rate), tab)[3] for d in rm.CORE]
    assert 0 in core and 1 in core


# ---- c. the projection matrix ----------------------------------------------------------------------------------------------
WPROJ = [(rid, name) for (rid, name) in rm.CORE_WP]


def span(key):
    ng, kw, M = rm.GEOMETRY[key[0]]
    return rm.CORE_WP[key] * M + kw


@pytest.mark.parametrize("key", WPROJ, ids=lambda k: f"{k[0]}/{k[1]}")
def test_projection_is_the_block_walk(key):
    rid, name = key
    rate = next(r for r in rm.RATES if rm.rate_id(r) == rid)
    ng, kw, M = rm.GEOMETRY[rid]
    wp = rm.CORE_WP[key]
    sos, gain = rm.BY_NAME[name].sos(rate)
    ns = len(sos)
    rng = np.random.default_rng(ns + ng)
    tab = random_table(ng, kw, 7 * ns + ng)
    # (test_rsos_wproj_host.py's windows, scaled: group g ends where its last output's newest input lies, half a window on)
    jend = np.array([(16 * g + 15) * M // (16 * ng) + (19 * kw) // 52 for g in range(ng)], dtype=np.int32)
    V, j0, K = wproj_matrix(sos, gain, tab, jend, M, wp)
    lo = int(jend.min()) - (kw - 1)
    assert j0 == lo and K == (wp - 1) * M + int(jend.max()) - lo + 1
    assert not V[2 * ns:].any()
    # V is the map of the KERNEL's walk: the Float64 D and A^16 the kernel holds, multiplied out in long double.  So is this walk --
    # A^16 the library's own doubles (so_rsos_chain_blocks), D by the Float64 recurrence, the arithmetic in long double.  In Float64,
    # as test_rsos_wproj_host.py walks its 220 blocks, the walk's own rounding over the thousands of blocks of a slow high-pass
    # (hp7@0.005 at 16 -> 48 kHz: 389 periods x 3 blocks, A^16 next to the identity) reaches 8.5e-13: the reference missing the
    # bound, not V.  (Against the long double A^16 both differ by up to 7e-12 there: what rounding A^16 to Float64 costs a walk.)
    D = walk_maps(sos)[0].astype(LD)
    A = chain_blocks(sos, gain)[0][: 2 * ns, : 2 * ns].astype(LD)
    x = rng.standard_normal((K, 3)).astype(LD)
    tabl = tab.astype(LD)
    s = np.zeros((2 * ns, 3), dtype=LD)
    for p in range(wp):
        for g in range(ng):
            o = p * M + int(jend[g]) - (kw - 1) - j0
            s = D @ (tabl[g].T @ x[o:o + kw]) + A @ s
    got = V[: 2 * ns].astype(LD) @ x
    err = (np.sqrt(((got - s) ** 2).sum(axis=0)) / np.sqrt((s ** 2).sum(axis=0))).astype(np.float64)
    print(f"wp {wp} span {wp * M + kw} frames: {err.max():.3e}")
    assert (err <= 1e-13).all()


def test_the_longest_span_is_among_them():
    assert WPROJ
    longest = max(WPROJ, key=span)
    print("longest span:", longest, span(longest))
    assert longest[1] == "hp1@0.0005" and 12000 < span(longest) <= 16384  # (the cap's two sides: test_gpu_rsos_matrix.py, test_projection_cap)
