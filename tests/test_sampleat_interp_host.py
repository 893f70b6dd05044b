"""`SampleAt(x, pos, interp="cubic" | "sinc")` and `Delay(..., interp=)` above the C-ABI (signals.py, lowering.py): the
keywords, every refusal, the lowered node, currying -- and the definition itself (tests/sampleat_interp_ref.py): its array
form held to its loop form bit for bit on the inputs the device tests read, the tap tables' properties, and what the
feature is for: the interpolation error of the reference against an analytic sine, and the attenuation `cutoff` buys a
read at speed 2.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import _capi as K
from sigops_amd import lowering as LW
from sigops_amd import signals as S
from sampleat_interp_ref import (KINDS, N_CHANNELS, N_TABLE, P, positions, same_bits, sampleat_interp, sampleat_interp_loops, table,
                                 tap_table)

FS = 10 * so.kHz


def _x(n=100, c=2, dtype=np.float64, fs=FS):
    return so.Signal(np.asfortranarray(np.arange(n * c, dtype=dtype).reshape(c, n).T), fs)


# ---- 1. the two forms of the definition ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", N_TABLE)
def test_the_array_form_equals_the_loop_form_bit_for_bit(N):
    for interp, kw in KINDS:
        for Cn, L in ((1, 1001), (3, 65)):
            x, pos = table(N, Cn), positions(N, L, Cn)
            for mode in ({}, {"left": -7.5, "right": np.inf}, {"wrap": True}, {"relative": True}, {"relative": True, "wrap": True}):
                a = sampleat_interp(x, pos, interp, **kw, **mode)
                b = sampleat_interp_loops(x, pos, interp, **kw, **mode)
                assert same_bits(a, b), (N, interp, kw, mode, np.flatnonzero(~((a == b) | (np.isnan(a) & np.isnan(b))).ravel())[:5])
        xn = table(N, 2, nonfinite=True)
        for mode in ({}, {"wrap": True}):
            assert same_bits(sampleat_interp(xn, positions(N, 1001), interp, **kw, **mode), sampleat_interp_loops(xn, positions(N, 1001), interp, **kw, **mode))
        x32, p32 = table(N, 2, np.float32, nonfinite=True), positions(N, 257, 1, np.float32)
        assert same_bits(sampleat_interp(x32, p32, interp, **kw, left=0.25), sampleat_interp_loops(x32, p32, interp, **kw, left=0.25))


def test_integer_positions_return_the_table_by_value_and_non_finite_values_poison_their_support():
    x = table(65, 2)
    n = np.arange(65, dtype=np.float64).reshape(-1, 1)
    for interp, kw in (("cubic", {}), ("sinc", {}), ("sinc", {"taps": 4}), ("sinc", {"taps": 64})):
        for mode in ({}, {"wrap": True}):
            assert same_bits(sampleat_interp(x, n, interp, **kw, **mode), x), (interp, kw, mode)
        # ... but a zero comes back positive: the sum of the other taps' zeros decides its sign
        z = np.asfortranarray(np.where(np.arange(65).reshape(-1, 1) == 30, -0.0, x[:, :1]))
        got = sampleat_interp(z, n, interp, **kw)
        assert got[30, 0] == 0.0 and not np.signbit(got[30, 0]) and same_bits(np.delete(got, 30, 0), np.delete(z, 30, 0))
        # an Inf at frame 30 makes NaN of every output whose support holds it, integer positions included (0 * Inf)
        y = x.copy()
        y[30, 0] = np.inf
        taps = 4 if interp == "cubic" else kw.get("taps", 16)
        got = sampleat_interp(y, n, interp, **kw)[:, 0]
        lo, hi = 30 - taps // 2, 30 + taps // 2 - 1  # j - K/2 + 1 <= 30 <= j + K/2
        assert np.isfinite(np.delete(got, range(lo, hi + 1))).all(), (interp, kw)
        # (on the Inf itself the sinc's impulse row gives 1 * Inf + zeros = Inf; the cubic's coefficients are NaN already)
        assert np.isnan(np.delete(got, 30)[lo:hi]).all() and (np.isnan(got[30]) if interp == "cubic" else got[30] == np.inf), (interp, kw)
    # with cutoff < 1 an integer position is filtered like any other
    assert not np.array_equal(sampleat_interp(x, n, "sinc", cutoff=0.5), x)


# ---- 2. the tap tables -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K_", [4, 6, 10, 16, 32, 64])
def test_the_tap_tables(K_):
    for cutoff in (1.0, 0.5, 0.123):
        h, dh = tap_table(K_, cutoff)
        assert h.shape == (P + 1, K_) and dh.shape == (P, K_) and h.dtype == dh.dtype == np.float64
        assert np.isfinite(h).all() and np.isfinite(dh).all()
        # a row was divided by its sum: what is left is the rounding of K quotients and of their sum
        assert np.abs(h.sum(axis=1) - 1.0).max() <= K_ * np.finfo(np.float64).eps
        assert np.array_equal(dh, h[1:] - h[:-1])
        if cutoff == 1.0:
            e0, eP = np.zeros(K_), np.zeros(K_)
            e0[K_ // 2 - 1] = eP[K_ // 2] = 1.0
            assert same_bits(h[0], e0) and same_bits(h[P], eP)
        # the package's builder is this one, byte for byte
        hp, dhp = S.sampleat_taps(K_, cutoff)
        assert same_bits(hp, h) and same_bits(dhp, dh) and hp.flags.c_contiguous and dhp.flags.c_contiguous


# ---- 3. keywords, refusals, the node ---------------------------------------------------------------------------------
def test_keywords_and_currying():
    x = _x()
    pos = so.Signal(np.zeros((40, 1)), FS)
    y = so.SampleAt(x, pos, interp="cubic")
    assert isinstance(y, so.SampleAtSignal) and (y.interp, y.taps, y.cutoff) == ("cubic", 0, 0.0)
    assert so.nframes(y) == 40 and so.nchannels(y) == 2 and so.sampletype(y) == np.float64
    y = so.SampleAt(x, pos, interp="sinc")
    assert (y.interp, y.taps, y.cutoff) == ("sinc", 16, 1.0)
    y = x | so.SampleAt(pos, left=1.0, wrap=True, interp="sinc", taps=32, cutoff=0.25)
    assert isinstance(y, so.SampleAtSignal) and y.signal is x and y.pos is pos
    assert (y.left, y.wrap, y.interp, y.taps, y.cutoff) == (1.0, True, "sinc", 32, 0.25)
    assert (so.SampleAt(x, pos).interp, so.SampleAt(x, pos, interp="linear").taps) == ("linear", 0)
    d = x | so.Delay(3, interp="cubic")
    assert so.nframes(d) == 100 and d.signal.interp == "cubic" and d.signal.relative
    d = so.Delay(x, 2.5, interp="sinc", taps=8, cutoff=0.5)
    assert (d.signal.interp, d.signal.taps, d.signal.cutoff) == ("sinc", 8, 0.5)
    assert so.Delay(x, so.Signal(np.full((60, 1), 1.5), FS), interp="sinc").signal.signal.interp == "sinc"  # (Until(Pad(SampleAt)))
    # ToFramerate hands an unknown rate to pos and keeps the kind
    z = so.ToFramerate(so.SampleAt(_x(fs=44.1 * so.kHz), so.Signal(np.zeros((40, 1))), interp="sinc", taps=8, cutoff=0.5), 8 * so.kHz)
    assert isinstance(z, so.SampleAtSignal) and (z.interp, z.taps, z.cutoff) == ("sinc", 8, 0.5) and z.pos.fs == 8000.0


def test_refusals_name_the_argument():
    x = _x()
    pos = so.Signal(np.zeros((40, 1)), FS)
    cases = [
        (lambda: so.SampleAt(x, pos, taps=16), "SampleAt", "taps"),
        (lambda: so.SampleAt(x, pos, cutoff=1.0), "SampleAt", "cutoff"),
        (lambda: so.SampleAt(x, pos, interp="linear", taps=16), "SampleAt", "taps"),
        (lambda: so.SampleAt(x, pos, interp="cubic", taps=4), "SampleAt", "taps"),
        (lambda: so.SampleAt(x, pos, interp="cubic", cutoff=0.5), "SampleAt", "cutoff"),
        (lambda: x | so.SampleAt(pos, interp="cubic", cutoff=0.5), "SampleAt", "cutoff"),
        (lambda: so.SampleAt(x, pos, interp="sinc", taps=15), "SampleAt", "taps"),
        (lambda: so.SampleAt(x, pos, interp="sinc", taps=2), "SampleAt", "taps"),
        (lambda: so.SampleAt(x, pos, interp="sinc", taps=66), "SampleAt", "taps"),
        (lambda: so.SampleAt(x, pos, interp="sinc", taps=16.0), "SampleAt", "taps"),
        (lambda: so.SampleAt(x, pos, interp="sinc", taps=True), "SampleAt", "taps"),
        (lambda: so.SampleAt(x, pos, interp="sinc", cutoff=0.0), "SampleAt", "cutoff"),
        (lambda: so.SampleAt(x, pos, interp="sinc", cutoff=1.0000001), "SampleAt", "cutoff"),
        (lambda: so.SampleAt(x, pos, interp="sinc", cutoff=-0.5), "SampleAt", "cutoff"),
        (lambda: so.SampleAt(x, pos, interp="sinc", cutoff=float("nan")), "SampleAt", "cutoff"),
        (lambda: so.SampleAt(x, pos, interp="sinc", cutoff="half"), "SampleAt", "cutoff"),
        (lambda: so.SampleAt(x, pos, interp="lanczos"), "SampleAt", "interp"),
        (lambda: so.SampleAt(x, pos, interp=None), "SampleAt", "interp"),
        (lambda: so.SampleAt(x, pos, interp=2), "SampleAt", "interp"),
        (lambda: so.Delay(x, 3, taps=16), "Delay", "taps"),
        (lambda: so.Delay(x, 3, interp="cubic", cutoff=0.5), "Delay", "cutoff"),
        (lambda: x | so.Delay(3, interp="sinc", taps=7), "Delay", "taps"),
        (lambda: so.Delay(x, 3, interp="nearest"), "Delay", "interp"),
    ]
    for make, who, words in cases:
        with pytest.raises(so.ErrorException) as e:
            make()
        assert who in str(e.value) and words in str(e.value), str(e.value)


def _bytes(lw):
    return bytes(C.string_at(C.addressof(lw.nodes), C.sizeof(lw.nodes)))


def test_the_lowered_node():
    x = _x(100, 2, np.float32)
    pos = so.Signal(np.zeros((40, 1)), FS)
    lw = LW.lower(so.SampleAt(x, pos, left=-1.5, right=2.5, relative=True, interp="cubic"))
    nd = lw.nodes[lw.root]
    assert nd.kind == K.NODE_SAMPLEAT and nd.i0 == 1 and nd.i1 == 1 and (nd.d0, nd.d1, nd.d2) == (-1.5, 2.5, 0.0)
    assert (nd.i2, nd.i3, nd.l0, nd.l1, nd.s0, nd.s1) == (0,) * 6 and not nd.p0 and not nd.p1
    assert nd.n_children == 2 and nd.nch == 2 and nd.dtype == K.SO_F64 and nd.nframes == 40
    for taps, cutoff in ((16, 1.0), (64, 0.5), (6, 0.25)):
        lw = LW.lower(so.SampleAt(x, pos, wrap=True, interp="sinc", taps=taps, cutoff=cutoff))
        nd = lw.nodes[lw.root]
        assert nd.kind == K.NODE_SAMPLEAT and nd.i0 == 2 and nd.i1 == 2 and nd.i2 == taps and nd.d2 == cutoff
        assert nd.s0 == (2 * P + 1) * taps and nd.p0 and (nd.i3, nd.l0, nd.l1, nd.s1) == (0,) * 4 and not nd.p1
        tab = np.ctypeslib.as_array(C.cast(nd.p0, C.POINTER(C.c_double)), shape=(nd.s0,))
        h, dh = tap_table(taps, cutoff)
        assert same_bits(tab[:(P + 1) * taps].reshape(P + 1, taps), h) and same_bits(tab[(P + 1) * taps:].reshape(P, taps), dh)
    # "linear" spelled out is the node it always was, byte for byte (the two leaves are the same objects: the same pointers)
    a = LW.lower(so.SampleAt(x, pos, left=-1.5, right=2.5, relative=True))
    b = LW.lower(so.SampleAt(x, pos, left=-1.5, right=2.5, relative=True, interp="linear"))
    assert a.n == b.n and a.root == b.root
    for i in range(a.n):
        for name, _ in K.so_node_t._fields_:
            if name != "children":
                assert getattr(a.nodes[i], name) == getattr(b.nodes[i], name), (i, name)
        assert list(a.nodes[i].children[:a.nodes[i].n_children]) == list(b.nodes[i].children[:b.nodes[i].n_children])
    assert (a.nodes[a.root].i1, a.nodes[a.root].i2, a.nodes[a.root].s0, a.nodes[a.root].d2) == (0, 0, 0, 0.0) and not a.nodes[a.root].p0
    lw = LW.lower(so.Delay(x, 3, interp="sinc", taps=8))
    kinds = [lw.nodes[i].kind for i in range(lw.n)]
    assert kinds == [K.NODE_ARRAY, K.NODE_CONST, K.NODE_SAMPLEAT, K.NODE_UNTIL] and (lw.nodes[2].i0, lw.nodes[2].i1, lw.nodes[2].i2) == (1, 2, 8)


def test_an_integer_delay_is_x_behind_zeros_by_value():
    """the definition at the positions Delay(x, k) lowers to: n - k, relative to the frames of x, zeros on the left"""
    x = table(65, 2)
    for interp, kw in KINDS:
        if kw.get("cutoff", 1.0) != 1.0:
            continue
        for k in (0, 1, 7, 64, 65):
            d = so.Delay(so.Signal(x, FS), k, interp=interp, **kw)
            sa = d.signal
            assert isinstance(sa.pos, so.NumberSig) and sa.pos.val == -float(k) and sa.relative and (sa.left, sa.right) == (0.0, 0.0)
            got = sampleat_interp(x, np.full((65, 1), sa.pos.val), interp, relative=True, **kw)
            want = np.zeros_like(x)
            want[k:] = x[:max(65 - k, 0)]
            assert np.array_equal(got, want), (interp, kw, k)


# ---- 4. what the feature is for ----------------------------------------------------------------------------------------
def _read_error(freq, interp, **kw):
    """the norm-wise relative error of a table of 4096 frames of sin(2 pi freq n), read at 64 + 0.7319 n over the positions
    64 frames clear of both ends, against the analytic sine"""
    n = np.arange(4096, dtype=np.float64)
    x = np.sin(2 * np.pi * freq * n).reshape(-1, 1)
    p = 64.0 + 0.7319 * np.arange(8192, dtype=np.float64)
    p = p[p <= 4095.0 - 64.0].reshape(-1, 1)
    want = np.sin(2 * np.pi * freq * p)
    got = np.interp(p[:, 0], n, x[:, 0]).reshape(-1, 1) if interp == "linear" else sampleat_interp(x, p, interp, **kw)
    return np.linalg.norm(got - want) / np.linalg.norm(want)


def test_quality_against_an_analytic_sine():
    e = {(f, k): _read_error(f, k) for f in (0.15, 0.3) for k in ("linear", "cubic", "sinc")}
    for key, v in e.items():
        print(f"read error {key}: {v:.3e}")
    assert e[0.15, "cubic"] <= e[0.15, "linear"] / 2
    assert e[0.15, "sinc"] <= e[0.15, "cubic"] / 100
    assert e[0.3, "sinc"] <= e[0.3, "cubic"] / 100


def test_cutoff_attenuates_what_a_fast_read_would_fold_back():
    """a sine at 0.45 cycles per frame read at speed 2 lies at 0.9 cycles per output frame, above the new Nyquist: it folds
    to 0.1.  With taps=64, cutoff=0.5 ends the pass band at 0.25 cycles per frame of the table; the reference measured
    -112.4 dB of output power against cutoff=1.0 (DESIGN.md "SampleAt"); half of that in dB is asserted."""
    n = np.arange(4096, dtype=np.float64)
    x = np.sin(2 * np.pi * 0.45 * n).reshape(-1, 1)
    p = (64.0 + 2.0 * np.arange(1984, dtype=np.float64) + 0.25).reshape(-1, 1)
    full = sampleat_interp(x, p, "sinc", taps=64, cutoff=1.0)
    half = sampleat_interp(x, p, "sinc", taps=64, cutoff=0.5)
    db = 10 * np.log10(np.mean(half ** 2) / np.mean(full ** 2))
    print(f"cutoff=0.5 against cutoff=1.0 at speed 2: {db:.1f} dB, full power {np.mean(full ** 2):.3f}")
    assert np.mean(full ** 2) > 0.4  # the unfiltered read passes the sine (power 1/2) almost whole
    assert db <= -112.4 / 2
