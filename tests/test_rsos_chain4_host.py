"""The chain wave's recurrence matrix on the 4 x 4 x 4 matrix shape (csrc/stages.cpp rsos_chain4_operands, through the C-ABI's
host-only diagnostic so_rsos_chain_blocks).  A^16 -- the map from the DF2T state entering a block of 16 samples to the state
behind it -- is block lower triangular in 4 x 4 blocks for a cascade in cascade order, so the kernel applies it block by
block, one v_mfma_f64_4x4x4_4b_f64 per block (r, c), c <= r.  Checked here without a device, for cascades of 1 .. 6 sections:
the blocks above the diagonal are EXACTLY zero (low-, high-, band-pass, band-stop, the headline's filter); the block
recurrence in the kernel's order equals A^16 . S + d to rounding over 1 000 steps; the table the kernel reads has the
instruction's A-operand layout and holds the doubles of A^16 themselves."""
import ctypes as C

import numpy as np
import pytest

import rsos_matrix
import sigops_amd as so
from sigops_amd import FilterFn, _capi

LD = np.longdouble
# (r, c) of the table's six blocks; lane l of a block holds A_b[i][k] with i = l & 3, k = l >> 4, the same for all four b
BLOCKS = [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)]
# the kernel's order within a step: every accumulate chain spaced, every B operand of the next step ready early
ORDER = [(2, 0), (1, 0), (0, 0), (2, 1), (1, 1), (2, 2)]

HEADLINE = ("bandstop", ("butterworth", 5), (500.0, 2000.0))
DESIGNS = [HEADLINE] + [("bandstop", ("butterworth", n), (500.0, 2000.0)) for n in (1, 2, 3, 4, 6)] \
    + [("bandpass", ("butterworth", n), (1000.0, 4000.0)) for n in (1, 2, 3, 4, 5, 6)] \
    + [("lowpass", ("butterworth", n), (3000.0,)) for n in (1, 2, 3, 5, 7, 8, 9, 11, 12)] \
    + [("highpass", ("butterworth", n), (200.0,)) for n in (2, 4, 6, 7, 10, 12)] \
    + [("lowpass", ("chebyshev1", 9, 1.0), (5000.0,))]
# the Chebyshev and the slow high-pass designs of the fused kernel's matrix (tests/rsos_matrix.py), at 44.1 -> 48 kHz: cutoffs in Hz
# at 48 kHz.  (Appended: the designs above keep their test ids.)
MATRIX_DESIGNS = [(d.kind, d.method, d.hz((44.1, 48.0))) for d in rsos_matrix.DESIGNS
                  if d.method[0] == "chebyshev1" or (d.kind == "highpass" and not d.absolute and d.bounds[0] <= 0.005)]
assert len(MATRIX_DESIGNS) == 4 + 6
DESIGNS = DESIGNS + MATRIX_DESIGNS


def chain_blocks(sos, gain):
    """(A^16 [12 x 12], table [6][64], taken?)"""
    a16, blocks, ok = np.zeros((12, 12)), np.zeros((6, 64)), C.c_int32()
    dp = C.POINTER(C.c_double)
    sos_c = np.ascontiguousarray(sos, dtype=np.float64)
    st = _capi.lib().so_rsos_chain_blocks(sos_c.ctypes.data_as(dp), len(sos), gain, a16.ctypes.data_as(dp), blocks.ctypes.data_as(dp), C.byref(ok))
    assert st == 0, _capi.last_error()
    return a16, blocks, ok.value


def a16_reference(sos):
    """A^16 in long double: the DF2T recurrence over 16 zero samples from unit states"""
    ns = len(sos)
    sos = np.asarray(sos, dtype=LD)
    A = np.zeros((2 * ns, 2 * ns), dtype=LD)
    for d in range(2 * ns):
        st = np.zeros(2 * ns, dtype=LD)
        st[d] = 1
        for _ in range(16):
            v = LD(0)
            for f in range(ns):
                b0, b1, b2, _, a1, a2 = sos[f]
                xi = v
                v = st[2 * f] + b0 * xi
                st[2 * f] = st[2 * f + 1] + b1 * xi - a1 * v
                st[2 * f + 1] = b2 * xi - a2 * v
        A[:, d] = st
    return A


def ids(d):
    return f"{d[0]}-{d[1][0]}{d[1][1]}" + (f"@{d[2][0]:g}Hz" if d in MATRIX_DESIGNS else "")


@pytest.mark.parametrize("design", DESIGNS, ids=ids)
def test_blocks_above_the_diagonal_are_exactly_zero(design):
    sos, gain = so.design_iir(FilterFn(*design), 48000.0)
    ns = len(sos)
    assert 1 <= ns <= 6
    a16, blocks, ok = chain_blocks(sos, gain)
    assert ok == 1
    for r in range(3):
        for c in range(r + 1, 3):
            assert not a16[4 * r:4 * r + 4, 4 * c:4 * c + 4].any(), (r, c)  # (== 0.0, not small)
    assert not a16[2 * ns:].any() and not a16[:, 2 * ns:].any()  # (states the cascade does not have)
    want = a16_reference(sos)
    err = float(np.abs(a16[:2 * ns, :2 * ns] - want).max() / np.abs(want).max())
    print(f"A^16 against long double: {err:.3e}")
    assert err <= 1e-12  # (16 steps of a Float64 recurrence with poles inside the unit circle)


def test_sections_cover_one_to_six():
    seen = {len(so.design_iir(FilterFn(*d), 48000.0)[0]) for d in DESIGNS}
    assert seen == {1, 2, 3, 4, 5, 6}


@pytest.mark.parametrize("design", DESIGNS, ids=ids)
def test_table_layout_round_trips(design):
    """entry l of block (r, c) is A^16[4 r + (l & 3)][4 c + (l >> 4)] -- the same 4 x 4 in all four 16-lane groups -- bit for bit"""
    sos, gain = so.design_iir(FilterFn(*design), 48000.0)
    a16, blocks, ok = chain_blocks(sos, gain)
    assert ok == 1
    back = np.zeros((12, 12))
    for t, (r, c) in enumerate(BLOCKS):
        for lane in range(64):
            i, k = lane & 3, lane >> 4
            assert blocks[t, lane] == a16[4 * r + i, 4 * c + k]
            back[4 * r + i, 4 * c + k] = blocks[t, lane]
    assert np.array_equal(back, a16)


def mfma4(a_lanes, b_lanes, c_lanes):
    """v_mfma_f64_4x4x4_4b_f64 as the device's lane probe prints it (tools/micro/mfma64_chain.hip): A_b[i][k] in lane
    16 k + 4 b + i, B_b[k][j] in lane 16 k + 4 b + j, D_b[i][j] in lane 16 i + 4 b + j; the k sum in ascending order"""
    A, B = a_lanes.reshape(4, 4, 4), b_lanes.reshape(4, 4, 4)  # [k][b][i], [k][b][j]
    d = c_lanes.reshape(4, 4, 4).copy()                         # [i][b][j]
    for k in range(4):
        d = d + np.einsum("bi,bj->ibj", A[k], B[k])
    return d.reshape(64)


@pytest.mark.parametrize("design", [HEADLINE, ("bandstop", ("butterworth", 1), (500.0, 2000.0)), ("highpass", ("butterworth", 7), (200.0,)),
                                    ("bandpass", ("butterworth", 6), (1000.0, 4000.0)), ("lowpass", ("butterworth", 5), (3000.0,))], ids=ids)
def test_block_recurrence_in_the_kernels_order(design):
    """1 000 steps of S' = d + A^16 . S for 16 sequences, the kernel's way -- a row block of the state one value per lane
    (lane 16 i + s: state row 4 r + i of sequence s), one instruction per block in ORDER, D . x the C operand of a row
    block's first instruction -- against the dense product in long double"""
    sos, gain = so.design_iir(FilterFn(*design), 48000.0)
    ns = len(sos)
    nk = (2 * ns + 3) // 4
    a16, blocks, ok = chain_blocks(sos, gain)
    assert ok == 1
    tab = {rc: blocks[t] for t, rc in enumerate(BLOCKS)}
    rng = np.random.default_rng(5 + ns)
    S = np.zeros((3, 64))
    Sref = np.zeros((12, 16), dtype=LD)
    A = a16.astype(LD)
    worst = 0.0
    for step in range(1000):
        d = np.zeros((12, 16))
        d[:2 * ns] = rng.standard_normal((2 * ns, 16))
        acc = {r: d[4 * r:4 * r + 4].reshape(64).copy() for r in range(nk)}  # (row i of the block, sequence s -> lane 16 i + s)
        for r, c in ORDER:
            if r < nk and c < nk:
                acc[r] = mfma4(tab[(r, c)], S[c], acc[r])
        for r in range(nk):
            S[r] = acc[r]
        Sref = d.astype(LD) + A @ Sref
        got = np.concatenate([S[r].reshape(4, 16) for r in range(3)])
        worst = max(worst, float(np.abs(got - Sref).max() / max(1.0, float(np.abs(Sref).max()))))
    print(f"block recurrence against dense long double, 1 000 steps: {worst:.3e}")
    # (each step adds a few ulps of the state's size; the recurrence contracts them at the filter's own rate)
    assert worst <= 1e-12
