"""The folded block of the fused resampler + IIR kernel (csrc/stages.cpp rsos_fold_tables, through the C-ABI's host-only
diagnostic so_rsos_fold_tables): the zero-state response T of the cascade over a block is folded into the tap table,
M_g = T . Tap_g^T, so that a block's resampling product IS its zero-state output Z = T . X, and the chain wave's share of the
next state comes from Z through E = D . T^-1 (E . Z = D . X).  Checked against NumPy in long double: E . T = D, the folded
table with the kernel's row permutation, the two block walks in Float64 side by side, and the planner's gate
amp = max_i sum_j (|E| |T|)_ij / max_i sum_j |D|_ij <= 256."""
import ctypes as C

import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import FilterFn, _capi

LD = np.longdouble
# MFMA row m = gq + 4 v of a folded block holds output time 2 gq + (v & 1) + 8 (v >> 1) of the block
TIME = np.array([2 * (m & 3) + ((m >> 2) & 1) + 8 * (m >> 3) for m in range(16)])

BANDSTOP = ("bandstop", ("butterworth", 5), (500.0, 2000.0))  # the headline's filter
HIGHPASS = ("highpass", ("butterworth", 7), (200.0,))


def block_maps(sos, gain):
    """T [16 x 16], C [16 x 2 ns], D [2 ns x 16], A^16 [2 ns x 2 ns] of the DF2T cascade over one block, in long double"""
    ns = len(sos)
    sos = np.asarray(sos, dtype=LD)

    def run(x, st):
        st = st.copy()
        y = np.zeros(16, dtype=LD)
        for t in range(16):
            v = x[t]
            for f in range(ns):
                b0, b1, b2, _, a1, a2 = sos[f]
                xi = v
                v = st[2 * f] + b0 * xi
                st[2 * f] = st[2 * f + 1] + b1 * xi - a1 * v
                st[2 * f + 1] = b2 * xi - a2 * v
            y[t] = v * LD(gain)
        return y, st

    eye16, eyes, z16, zs = np.eye(16, dtype=LD), np.eye(2 * ns, dtype=LD), np.zeros(16, dtype=LD), np.zeros(2 * ns, dtype=LD)
    cols = [run(eye16[t], zs) for t in range(16)]
    T = np.stack([c[0] for c in cols], axis=1)
    D = np.stack([c[1] for c in cols], axis=1)
    cols = [run(z16, eyes[d]) for d in range(2 * ns)]
    Cm = np.stack([c[0] for c in cols], axis=1)
    A = np.stack([c[1] for c in cols], axis=1)
    return T, Cm, D, A


def fold_tables(sos, gain, tab):
    """(E [12 x 16] with natural time columns, folded table [ng][kw][16] with lane m = MFMA row, amp, decision)"""
    ng, kw, _ = tab.shape
    e = np.zeros((12, 16))
    ft = np.zeros((ng, kw, 16))
    amp, fold = C.c_double(), C.c_int32()
    dp = C.POINTER(C.c_double)
    sos_c, tab_c = np.ascontiguousarray(sos, dtype=np.float64), np.ascontiguousarray(tab)
    st = _capi.lib().so_rsos_fold_tables(sos_c.ctypes.data_as(dp), len(sos), gain, tab_c.ctypes.data_as(dp), ng, kw, e.ctypes.data_as(dp),
                                         ft.ctypes.data_as(dp), C.byref(amp), C.byref(fold))
    assert st == 0, _capi.last_error()
    return e, ft, amp.value, fold.value


def random_table(seed):
    rng = np.random.default_rng(seed)
    ng, kw = 10, 52  # 44.1 -> 48 kHz: ten blocks of 16 outputs per period, windows of 13 k-steps
    tab = rng.standard_normal((ng, kw, 16)) / np.sqrt(kw)
    tab[:, :3, :] = 0.0
    return tab, rng


@pytest.mark.parametrize("design", [BANDSTOP, HIGHPASS])
def test_e_times_t_is_d(design):
    sos, gain = so.design_iir(FilterFn(*design), 48000.0)
    ns = len(sos)
    tab, _ = random_table(ns)
    E, _, amp, fold = fold_tables(sos, gain, tab)
    T, _, D, _ = block_maps(sos, gain)
    assert fold == 1 and amp <= 256.0
    assert not E[2 * ns:].any()  # (rows of states the cascade does not have)
    got = E[: 2 * ns].astype(LD) @ T
    scale = np.abs(D).sum(axis=1).max()
    err = float(np.abs(got - D).max() / scale)
    print(f"E.T - D: {err:.3e} (amp {amp:.3g})")
    assert err <= 1e-15 * amp
    # amp as defined: max row sum of |E| |T| over max row sum of |D|
    want_amp = float((np.abs(E[: 2 * ns].astype(LD)) @ np.abs(T)).sum(axis=1).max() / scale)
    assert abs(amp - want_amp) <= 1e-12 * want_amp


@pytest.mark.parametrize("design", [BANDSTOP, HIGHPASS])
def test_folded_table_is_t_times_taps_permuted(design):
    sos, gain = so.design_iir(FilterFn(*design), 48000.0)
    tab, _ = random_table(len(sos) + 10)
    _, ft, _, _ = fold_tables(sos, gain, tab)
    T, _, _, _ = block_maps(sos, gain)
    # tab[g][kk][t]: tap of output t of the block at window slot kk; folded: row m is output TIME[m] of T . Tap_g^T
    want = np.einsum("mt,gkt->gkm", T[TIME], tab.astype(LD))
    err = float(np.abs(ft - want).max() / np.abs(want).max())
    print(f"folded table: {err:.3e}")
    assert err <= 4e-16  # (long double sums rounded once to Float64: half an ulp of the largest entry, with room for denormal rows)


@pytest.mark.parametrize("design", [BANDSTOP, HIGHPASS])
def test_the_two_block_walks_agree(design):
    """the plain block walk (X, D . X, T . X + C . S) and the folded one (Z, E . Z, Z + C . S) in Float64 over 4 000 blocks
    of random windows: their outputs differ by rounding, below 1.5e-13 norm-wise"""
    sos, gain = so.design_iir(FilterFn(*design), 48000.0)
    ns = len(sos)
    tab, rng = random_table(len(sos) + 20)
    E, ft, _, fold = fold_tables(sos, gain, tab)
    assert fold == 1
    T, Cm, D, A = (m.astype(np.float64) for m in block_maps(sos, gain))
    E = E[: 2 * ns]
    Ep, Cp = E[:, TIME], Cm[TIME]  # (the kernel's operands: columns of E and rows of C in MFMA-row order)
    back = np.argsort(TIME)
    ng, kw, _ = tab.shape
    nblocks, rows = 4000, 4
    s0 = np.zeros((2 * ns, rows))
    s1 = s0.copy()
    y0 = np.empty((nblocks, 16, rows))
    y1 = np.empty_like(y0)
    for b in range(nblocks):
        g = b % ng
        win = rng.standard_normal((kw, rows))
        X = tab[g].T @ win
        y0[b] = T @ X + Cm @ s0
        s0 = D @ X + A @ s0
        Z = ft[g].T @ win
        y1[b] = (Z + Cp @ s1)[back]
        s1 = Ep @ Z + A @ s1
    d = float(np.linalg.norm(y1 - y0) / np.linalg.norm(y0))
    print(f"folded vs plain walk: {d:.3e}")
    assert d < 1.5e-13


@pytest.mark.parametrize("design, fs, admitted", [(BANDSTOP, 48000.0, True), (HIGHPASS, 48000.0, True), (BANDSTOP, 16000.0, True),
                                                  (("lowpass", ("butterworth", 7), (5000.0,)), 48000.0, False),
                                                  (("lowpass", ("butterworth", 5), (4000.0,)), 16000.0, False),
                                                  (("lowpass", ("butterworth", 5), (20000.0,)), 48000.0, False)])
def test_gate(design, fs, admitted):
    sos, gain = so.design_iir(FilterFn(*design), fs)
    tab, _ = random_table(3)
    _, _, amp, fold = fold_tables(sos, gain, tab)
    print(f"amp {amp:.4g} fold {fold}")
    assert (amp <= 256.0) == admitted and fold == int(admitted)


def test_bad_arguments():
    sos, gain = so.design_iir(FilterFn(*BANDSTOP), 48000.0)
    tab, _ = random_table(4)
    e = np.zeros((12, 16))
    amp, fold = C.c_double(), C.c_int32()
    dp = C.POINTER(C.c_double)
    sos_c = np.ascontiguousarray(sos, dtype=np.float64)
    st = _capi.lib().so_rsos_fold_tables(sos_c.ctypes.data_as(dp), 7, gain, tab.ctypes.data_as(dp), 10, 52, e.ctypes.data_as(dp), None,
                                         C.byref(amp), C.byref(fold))
    assert st != 0
