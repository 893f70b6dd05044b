"""What the oracle makes of the spoiled inputs of tests/forms_corpus.py: the facts tests/test_gpu_forms_nonfinite.py leans on,
asserted with the oracle alone, so that a change of a seed or of a plant cannot empty the assertions made on the device.

A resampler's output is non-finite where its own taps reach a non-finite sample: short runs, in the planted channels only.  A
filter's channel is non-finite from its first such output to its end (0 * NaN is NaN: also behind a pole at 0), and the
reference filters the frames in front of a window too (src/cutting.jl:160-173), so a plant far before a window spoils the
whole window.  Below a `Normpower` one plant makes every sample of every channel NaN."""
import functools

import numpy as np
import pytest

import sigops_amd as so
from oracle_bridge import oracle_sink
from forms_corpus import (A_CASES, FW_AFTER, FW_CASES, FW_PLANTS, FW_UNTIL, I_CASES, NFRAMES, OVERFLOW_CASE, R_CASES, arbitrary_tree,
                          arbitrary_tree_spoiled, filter_tree, filter_tree_spoiled, filter_window_tree, forgotten, overflow_tree, resampler_tree,
                          resampler_tree_spoiled, rs_nf_cap)
from forms_corpus import filter_id as _iid, resampler_id as _rid


def runs(mask):
    """the maximal runs of True in a vector as (first, last)"""
    idx = np.nonzero(mask)[0]
    if idx.size == 0:
        return []
    cuts = np.nonzero(np.diff(idx) > 1)[0]
    return list(zip(idx[np.r_[0, cuts + 1]].tolist(), idx[np.r_[cuts, idx.size - 1]].tolist()))


def same_outside(bad, want, clean):
    """outside the set the spoiled input gives what the clean input gives, bit for bit, in a resampler (an FIR forgets)"""
    return np.array_equal(want[~bad], clean[~bad])


@pytest.mark.parametrize("case", [c for c in R_CASES if not c[5]], ids=_rid)
def test_resampler_plants(case):
    fi, fo, nout, nch, dt, _ = case
    x, plants = resampler_tree_spoiled(case)
    want = oracle_sink(x)
    bad = ~np.isfinite(want)
    assert want.shape == (nout, nch) and want.dtype == dt
    planted = {p[0] for p in plants}
    assert planted == ({0, nch - 1} | ({3} if nch >= 4 else set())) and len(planted) < nch
    for c in range(nch):
        assert bad[:, c].any() == (c in planted), c
    r0 = runs(bad[:, 0])
    assert len(r0) == 1 and r0[0][0] == 0 and 19 <= r0[0][1] + 1 <= 39, r0  # the first outputs
    last = runs(bad[:, nch - 1])
    if nch != 4:
        assert len(last) == 2 and last[1][1] == nout - 1 and 55 <= bad[:, nch - 1].sum() <= 115, last  # the middle and the end
    else:  # (channel 3 carries the plant at frame 4999 as well)
        assert len(last) == 3 and last[2][1] == nout - 1 and 55 <= bad[last[1][0]:, 3].sum() <= 115, last
    assert same_outside(bad, want, oracle_sink(resampler_tree(case)))


@pytest.mark.parametrize("case", A_CASES, ids=_rid)
def test_arbitrary_rate_plants(case):
    fi, fo, nout, nch, dt = case
    x, plants = arbitrary_tree_spoiled(case)
    want = oracle_sink(x)
    bad = ~np.isfinite(want)
    assert want.shape == (nout, nch) and want.dtype == dt
    planted = {p[0] for p in plants}
    for c in range(nch):
        assert bad[:, c].any() == (c in planted), c
    assert len(planted) < nch
    r0, last = runs(bad[:, 0]), runs(bad[:, nch - 1])
    assert len(r0) == 1 and r0[0][0] == 0 and r0[0][1] < 200, r0
    assert len(last) == 2 and last[1][1] == nout - 1 and bad[:, nch - 1].sum() < 600, last
    if nch >= 4:
        assert len(runs(bad[:, 3])) == 1
    assert same_outside(bad, want, oracle_sink(arbitrary_tree(case)))


@pytest.mark.parametrize("case", [c for c in R_CASES if c[5]], ids=_rid)
def test_resampler_window_plants(case):
    """an FIR forgets: the plant far before the window and the one beyond its reach leave no trace in it"""
    fi, fo, nout, nch, dt, _ = case
    x, plants = resampler_tree_spoiled(case)
    want = oracle_sink(x)
    bad = ~np.isfinite(want)
    assert want.shape == (9001, nch)
    near, inside = (3 if nch > 3 else nch - 2), (5 if nch >= 6 else nch - 1)
    expect = {c: [] for c in range(nch)}
    expect[near] = expect[near] + [(0, 8)]
    expect[inside] = expect[inside] + [(3962, 4002)]
    assert [p[0] for p in plants][:3] == [0, near, inside] and (nch != 8 or plants[3][:2] == (7, 30000))
    for c in range(nch):
        assert runs(bad[:, c]) == expect[c], (c, runs(bad[:, c]))
    assert same_outside(bad, want, oracle_sink(resampler_tree(case)))


@functools.lru_cache(maxsize=None)
def _filter_oracle(case):
    x, plants = filter_tree_spoiled(case)
    return oracle_sink(x), plants


@pytest.mark.parametrize("case", I_CASES, ids=_iid)
def test_filter_plants(case):
    """every one of the six filters, the pole at 0 included: non-finite from the plant to frame 20000, nothing else"""
    f, nch, dt = case
    want, plants = _filter_oracle(case)
    bad = ~np.isfinite(want)
    assert want.shape == (NFRAMES, nch) and want.dtype == dt
    first = {ch: frame for ch, frame, _ in plants}
    assert len(first) == len(plants) and (nch < 3 or len(first) < nch)
    assert {5: {0: 0, 1: 4095, 3: 4096, 4: 20000}, 4: {0: 4095, 2: 4096, 3: 20000}, 1: {0: 12319}}[nch] == first
    for c in range(nch):
        assert runs(bad[:, c]) == ([(first[c], NFRAMES - 1)] if c in first else []), (c, runs(bad[:, c]))
    # in front of a plant a channel holds what the clean input gives
    clean = oracle_sink(filter_tree(case))
    assert np.array_equal(want[~bad], clean[~bad])


@pytest.mark.parametrize("case", I_CASES, ids=_iid)
def test_normpower_spreads_one_plant_everywhere(case):
    x, _ = filter_tree_spoiled(case)
    want = oracle_sink(x | so.Normpower)
    assert want.shape == (NFRAMES, case[1]) and np.isnan(want).all()


@pytest.mark.parametrize("case", FW_CASES, ids=_iid)
def test_filter_window_plants(case):
    """the reference filters the skipped frames: a NaN at frame 100 spoils a window that begins at frame 30000"""
    x, plants = filter_window_tree(case)
    assert plants == FW_PLANTS and (FW_AFTER, FW_UNTIL) == (30000, 5001)
    want = oracle_sink(x)
    assert want.shape == (FW_UNTIL, 5) and want.dtype == np.float64
    bad = ~np.isfinite(want)
    assert [runs(bad[:, c]) for c in range(5)] == [[(0, 5000)], [(0, 5000)], [], [(2000, 5000)], []]
    # the window is the whole filtered signal's frames
    whole = oracle_sink(filter_window_tree(case, window=False)[0])
    assert np.array_equal(want, whole[FW_AFTER:FW_AFTER + FW_UNTIL], equal_nan=True)
    # with the plant at frame 100 replaced by 0.0 (what a filter started from rest behind it sees): channel 0 is finite
    less = oracle_sink(filter_window_tree(case, forgotten(plants))[0])
    bad = ~np.isfinite(less)
    assert [runs(bad[:, c]) for c in range(5)] == [[], [(0, 5000)], [], [(2000, 5000)], []]
    assert np.array_equal(less[:, [2, 4]], want[:, [2, 4]]) and np.array_equal(less[:2000, 3], want[:2000, 3])


def test_overflow_inputs():
    fi, fo, nout, nch, dt, _ = OVERFLOW_CASE
    want = oracle_sink(overflow_tree()[0])
    bad = ~np.isfinite(want)
    assert want.shape == (nout, nch) and bad[:, 5].all() and not bad[:, [0, 1, 2, 3, 4, 6, 7]].any()
    # one list entry per tile of 32 rows / 8 channels = 4 periods of 2 outputs that holds a non-finite output
    tiles = len(set((np.nonzero(bad[:, 5])[0] // 8).tolist()))
    assert tiles > 2 * rs_nf_cap(), (tiles, rs_nf_cap())
    half = oracle_sink(overflow_tree(half=True)[0])
    bad = ~np.isfinite(half)
    r = runs(bad[:, 5])
    assert len(r) == 1 and r[0][0] == 0 and 20000 <= r[0][1] < 20100 and not bad[:, [0, 1, 2, 3, 4, 6, 7]].any(), r
    assert len(set((np.nonzero(bad[:, 5])[0] // 8).tolist())) > rs_nf_cap()
    assert np.array_equal(half[r[0][1] + 1:], oracle_sink(resampler_tree(OVERFLOW_CASE))[r[0][1] + 1:])
