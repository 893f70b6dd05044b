"""The executor's corpus of small trees, and the result views they are sunk into: shared by tools/plan_fingerprint.py (which
prints what the executor does for each of them, to compare two builds) and tests/test_gpu_forms.py (which asserts it).

The trees: every entry of tests/cases.py's CASES, then one per launch routine of csrc/executor.cpp that those do not reach,
built as the tests named beside them build theirs.  Inputs are seeded: every array leaf takes the next seed of a counter,
so a tree's data depend on how many leaves were made before it (`at_seed` sets the counter; `seed_starts` lists where each
entry of `corpus()` begins when the entries are built in order, as the tool builds them)."""
import os

import numpy as np

import sigops_amd as so
from cases import CASES

FS = 44.1 * so.kHz
_seed = [0]
_host = [False]  # every array leaf on the host, whatever its `dev=` says (the oracle's copy of a tree)
_made = []       # the host arrays of the leaves made since the last `at_seed`, in order


class env:
    """with env(NAME=value, OTHER=None): ... -- environment switches set (or, None, unset) for the block, then put back"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class at_seed:
    """with at_seed(k, host=True): ... -- leaves made in the block take the seeds k + 1, k + 2, ...; `host`: all on the host"""

    def __init__(self, seed, host=False):
        self.new = (seed, host)

    def __enter__(self):
        self.old = (_seed[0], _host[0])
        _seed[0], _host[0] = self.new
        del _made[:]
        return _made

    def __exit__(self, *a):
        _seed[0], _host[0] = self.old


def noise(n, nch, dt=np.float64, dev=True):
    """seeded noise as an array leaf: device-resident [nch][n] (planar, time fastest), or a column-major host array"""
    _seed[0] += 1
    a = np.asfortranarray(np.random.default_rng(_seed[0]).standard_normal((n, nch)).astype(dt))
    _made.append(a)
    if dev and not _host[0]:
        import torch

        return torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t()
    return a


def sig(n, nch=2, dt=np.float64, fs=FS, dev=True):
    return so.Signal(noise(n, nch, dt, dev), fs)


def tone(n, hz=200.0, nch=2):
    return so.Signal(so.sin, FS, ω=hz * so.Hz) | so.Until(n * so.frames) | so.ToChannels(nch)


BS = lambda: so.Filt(so.Bandstop, 0.5 * so.kHz, 2 * so.kHz)  # noqa: E731
LP = lambda **k: so.Filt(so.Lowpass, 3 * so.kHz, **k)  # noqa: E731
IRR = lambda **k: sig(40000, fs=1000 * so.Hz, **k) | so.ToFramerate(1000 * np.pi * so.Hz)  # noqa: E731  (a rate without a period)
POS = np.asfortranarray(np.random.default_rng(99).uniform(0, 4000, (6000, 1)))  # (positions of the SampleAt entries: a host leaf)


def extra():
    """(name, tree builder, result: dtype / where / layout / pad, environment)"""
    scenes = lambda f: so.Append(*[f(n) for n in (5001, 7777, 12345)])  # noqa: E731
    yield "append3_three_pass", lambda: scenes(lambda n: sig(n) | BS()), {}, {"SIGOPS_RSOS_BATCH": 0}  # test_gpu_sos_batch.py
    yield "append3_one_pass", lambda: scenes(lambda n: sig(n) | BS()), {}, {"SIGOPS_RSOS_BATCH": 1}  # test_gpu_rsos_batch.py
    fused = {"SIGOPS_RSOS_MINGROUPS": 1}  # test_gpu_rsos.py, test_gpu_rsos_two_arrays.py
    yield "rsos_f64", lambda: sig(20000) | BS() | so.ToFramerate(48 * so.kHz), {}, fused
    yield "rsos_f32_result", lambda: sig(20000) | BS() | so.ToFramerate(48 * so.kHz), {"dt": np.float32}, fused
    yield "rsos_two_arrays", lambda: so.Mix(sig(20000), sig(20000)) | BS() | so.ToFramerate(48 * so.kHz), {}, fused
    yield "narrow_filter", lambda: sig(10007) | LP(), {"dt": np.float32}, {}  # (alias_narrow)
    yield "narrow_resampler", lambda: sig(20000, 4) | so.ToFramerate(48 * so.kHz), {"dt": np.float32}, {}
    yield "alias_skip", lambda: sig(10007) | so.Filt(so.Bandpass, 1 * so.kHz, 3 * so.kHz) | so.After(100 * so.frames), {}, {}
    # (filters of three orders keep launches of their own: four steps, device leaves -- the plan is replayed as a graph)
    yield "three_windows", lambda: so.Append(*[sig(n) | LP(order=o) | so.Ramp(5 * so.ms) for n, o in ((9999, 2), (12001, 4), (8000, 6))]), {"pad": 5}, {}  # test_gpu_window_alias.py
    yield "exact_scan", lambda: sig(20000) | LP() | so.Normpower | so.After(1000 * so.frames), {}, {}
    yield "one_pass", lambda: sig(20000) | LP(), {}, {"SIGOPS_SOS_ONEPASS": 1}
    yield "exact_cascade", lambda: sig(10007) | LP(order=5), {}, {"SIGOPS_SOS_EXACT": 1}  # (test_gpu_fences.py: k_sos_exact)
    yield "state_pass", lambda: so.Mix(tone(40000, 1000.0, 8), sig(40000, 8)) | BS() | so.ToFramerate(96 * so.kHz), {}, {"SIGOPS_FUSE_STATE": 1}  # test_gpu_iir_onepass.py
    yield "sine_source", lambda: so.Mix(tone(20000), sig(20000)) | BS(), {}, {}
    yield "sine_source_batch", lambda: scenes(lambda n: so.Mix(tone(n, 200.0 + n % 7), sig(n)) | BS()), {}, {"SIGOPS_RSOS_BATCH": 0}
    yield "resample_rows", lambda: sig(20000, 4, np.float32) | so.ToFramerate(16 * so.kHz), {"dt": np.float32}, {"SIGOPS_RS_NOQ1": 1}  # test_gpu_accumulator.py
    yield "resample_tiled", lambda: IRR(), {}, {"SIGOPS_RS_NOARB": 1, "SIGOPS_RS_NOPAIR": 1}
    yield "resample_tiled2", lambda: IRR(), {}, {"SIGOPS_RS_NOARB": 1}
    yield "resample_arb", lambda: IRR(), {}, {"SIGOPS_ARB_MIN": 1}
    yield "resample_plain", lambda: IRR(), {}, {"SIGOPS_RS_NOTILED": 1}
    yield "resample_fixups", lambda: sig(20000, 3, fs=44100 * so.Hz) | so.ToFramerate(12000 * so.Hz), {}, {}
    yield "sample_at_array", lambda: so.SampleAt(sig(4001), so.Signal(POS, FS)), {}, {}
    yield "sample_at_tree", lambda: so.SampleAt(sig(4001), so.Cumsum(so.Signal(np.abs(POS) / 4000, FS)), wrap=True), {}, {}
    yield "comb", lambda: so.Comb(sig(10007), 257, 0.7), {}, {}
    yield "cumsum_two_chunks", lambda: so.Cumsum(sig(16385)), {}, {}
    yield "norm_direct", lambda: sig(10007) | so.Normpower, {}, {}
    for layout in ("planar", "interleaved", "strided"):
        yield "host_" + layout, lambda: sig(5001, dev=False) | LP() | so.Ramp(5 * so.ms), {"where": "host", "layout": layout}, {}
    yield "chan_stride", lambda: sig(10007, 3) | LP(), {"pad": 37}, {}
    yield "mono", lambda: sig(10007, 1) | LP(), {}, {}
    yield "mono_chan_stride", lambda: sig(10007, 1) | LP(), {"pad": 37}, {}


def corpus():
    """every tree as (name, tree builder, result view, environment), in the order the tool prints them"""
    return [(name, CASES[name], {"where": "host"}, {}) for name in sorted(CASES)] + list(extra())


def seed_starts():
    """where the leaf counter stands before each entry of `corpus()` when they are built one after the other from 0"""
    starts = []
    with at_seed(0, host=True):
        for _, build, _, _ in corpus():
            starts.append(_seed[0])
            try:
                build()
            except Exception:  # (a tree the engine refuses: it made the leaves it made)
                pass
    return starts


class ResultView:
    """A result for `tree` to be sunk into -- dtype `dt` (the tree's own by default); where="dev": a device tensor
    [nch][n + pad], time fastest, filled with NaN; where="host": a NumPy array in `layout` ("planar", "interleaved", or
    "strided": every second frame of a planar array twice as long) -- with what `so.Plan` needs to write it.

    .tree (sink parameters resolved), .n, .nch, .dt, .res, .strides, .ptr, .is_dev; bytes() the result's bytes, frames x
    channels in C order for a host result, the whole padded tensor for a device result; array() the n x nch values;
    clear() fills the whole buffer with NaN again (same address: a captured graph stays valid)"""

    def __init__(self, tree, dt=None, where="dev", layout="planar", pad=0):
        self.tree = so.engine.process_sink_params(tree)
        n, nch = so.nframes(self.tree), so.nchannels(self.tree)
        self.n, self.nch, self.pad, self.is_dev = n, nch, pad, where == "dev"
        self.dt = dt = np.dtype(dt or so.sampletype(self.tree))
        if where == "dev":  # [nch][n + pad], time fastest
            import torch

            self.res = torch.full((nch, n + pad), float("nan"), dtype=torch.float32 if dt == np.float32 else torch.float64, device="cuda")
            self.strides, self.ptr = (1, n + pad), self.res.data_ptr()
        else:
            self.res = res = {"planar": lambda: np.empty((n, nch), dt, order="F"), "interleaved": lambda: np.empty((n, nch), dt, order="C"),
                              "strided": lambda: np.empty((2 * n, nch), dt, order="F")[::2]}[layout]()
            self.strides, self.ptr = (res.strides[0] // res.itemsize, res.strides[1] // res.itemsize), res.ctypes.data

    def plan(self):
        return so.Plan(so.ToChannels(self.tree, self.nch), (self.n, self.nch), self.dt, self.strides, self.is_dev)

    def bytes(self):
        return self.res.cpu().numpy().tobytes() if self.is_dev else np.ascontiguousarray(self.res).tobytes()

    def array(self):
        return np.asfortranarray(self.res[:, :self.n].t().cpu().numpy()) if self.is_dev else np.array(self.res, order="F")

    def clear(self):
        if self.is_dev:
            self.res.fill_(float("nan"))
        else:
            self.res[...] = np.nan
