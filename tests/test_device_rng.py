"""Host side of counter-based device noise (`so.DeviceRNG`, include/sigops.h SO_FN_RANDN), no GPU: the Philox known
answers of the NumPy restatement the GPU tests compare with (philox_ref.py), the generator object's value semantics,
and the lowered node table -- one FUNC node that carries the seed and the stream, no host array."""
import re
import os

import numpy as np
import pytest

import sigops_amd as so
from sigops_amd import _capi as K

import philox_ref as R


def _words(c, k):
    return [int(w[0]) for w in R.philox4x32_10(c, k)]


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds"""
    assert _words((0, 0, 0, 0), (0, 0)) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert _words((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert _words((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_restatement_is_a_function_of_the_frame_index():
    z = R.randn(2024, 1, 0, 4096)
    for a in (1, 2, 333, 3996):
        assert np.array_equal(R.randn(2024, 1, a, 100), z[a:a + 100])
    assert not np.array_equal(R.randn(2024, 2, 0, 64), z[:64]) and not np.array_equal(R.randn(2025, 1, 0, 64), z[:64])
    u1, u2 = R.uniforms(0xDEADBEEFCAFEF00D, (1 << 32) + 7, np.arange(1 << 16))
    assert u1.min() > 0.0 and u1.max() <= 1.0 and u2.min() >= 0.0 and u2.max() < 1.0
    assert np.isfinite(z).all() and np.abs(z).max() < 8.58


def test_value_semantics_and_spawn():
    g = so.DeviceRNG(2024)
    assert (g.seed, g.stream) == (2024, 0)
    assert g == so.DeviceRNG(2024, 0) and hash(g) == hash(so.DeviceRNG(2024, 0))
    assert g != so.DeviceRNG(2024, 1) and g != so.DeviceRNG(2025) and g != 2024
    assert g.spawn(3) == so.DeviceRNG(2024, 3) and g.spawn(3).spawn(4) == g.spawn(7) and g.spawn(0) == g
    assert len({g, so.DeviceRNG(2024), g.spawn(1)}) == 2
    big = so.DeviceRNG((1 << 64) - 1, (1 << 64) - 1)
    assert big.spawn(1).stream == 0
    with pytest.raises(AttributeError):
        g.seed = 1
    for bad in (-1, 1 << 64, 1.5, "7", True):
        with pytest.raises(so.ErrorException):
            so.DeviceRNG(bad)
        with pytest.raises(so.ErrorException):
            so.DeviceRNG(0, bad)


def _rows(lw):
    return [lw.nodes[i] for i in range(lw.n)]


@pytest.mark.parametrize("seed, stream", [(2024, 0), (0xDEADBEEFCAFEF00D, (1 << 32) + 7), ((1 << 64) - 1, 1 << 63)])
def test_lowered_table_is_one_func_node(seed, stream):
    g = so.DeviceRNG(seed, stream)
    x = so.Signal(so.randn, 44.1 * so.kHz, rng=g) | so.Until(1 * so.s)
    rows = _rows(so.lower(x))
    assert [r.kind for r in rows] == [K.NODE_FUNC, K.NODE_UNTIL]
    f = rows[0]
    assert f.i0 == 3 == K.FN["randn"] and f.nch == 1 and f.dtype == K.SO_F64 and f.fs == 44100.0
    assert f.l0 & ((1 << 64) - 1) == seed and f.l1 & ((1 << 64) - 1) == stream
    assert not f.p0 and f.nframes == K.SO_LEN_INF
    assert rows[1].l0 == 44100


def test_leaf_survives_toframerate_and_is_memoised():
    g = so.DeviceRNG(5, 9)
    n = so.Signal(so.randn, rng=g)
    y = so.ToFramerate(n, 8 * so.kHz)
    assert isinstance(y, so.FuncSig) and y.rng == g and y.fs == 8000.0
    lw = so.lower(so.Mix(y, y) | so.Until(10 * so.frames))
    assert [r.kind for r in _rows(lw)].count(K.NODE_FUNC) == 1   # the same leaf object: one node, like any other leaf
    two = so.lower(so.Mix(so.Signal(so.randn, 8 * so.kHz, rng=g), so.Signal(so.randn, 8 * so.kHz, rng=g.spawn(1))) | so.Until(10 * so.frames))
    fn = [r for r in _rows(two) if r.kind == K.NODE_FUNC]
    assert [(r.l0, r.l1) for r in fn] == [(5, 9), (5, 10)]


def test_sink_level_device_rng_is_refused():
    x = so.Signal(so.randn, 1 * so.kHz) | so.Until(10 * so.frames)
    with pytest.raises(so.ErrorException, match=r"Signal\(randn, rng="):
        so.lower(x, rng=so.DeviceRNG(1))
    with pytest.raises(so.ErrorException, match=r"Signal\(randn, rng="):
        so.sink(x, rng=so.DeviceRNG(1))


def test_numpy_generator_leaf_lowers_as_before():
    d = np.random.default_rng(42).standard_normal(300)
    for kw in (dict(), dict(rng=np.random.default_rng(42))):
        x = so.Signal(so.randn, 1 * so.kHz, **kw) | so.Until(300 * so.frames)
        lw = so.lower(x, rng=None if kw else np.random.default_rng(42))
        rows = _rows(lw)
        assert [r.kind for r in rows] == [K.NODE_ARRAY, K.NODE_PAD, K.NODE_UNTIL]
        assert rows[0].l0 == 300 and rows[0].nframes == K.SO_LEN_UNCHECKED
        data = np.ctypeslib.as_array((K.C.c_double * 300).from_address(rows[0].p0))
        assert np.array_equal(data, d)


def test_header_and_binding_agree():
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sigops.h")).read()
    assert int(re.search(r"SO_FN_RANDN\s*=\s*(\d+)", h).group(1)) == K.FN["randn"] == K.SO_FN_RANDN == 3
