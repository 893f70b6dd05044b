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


# ---- the ladders of tests/test_gpu_forms.py: one small input per case, one rung per form ---------------------------------
F64, F32 = np.float64, np.float32
NFRAMES = 20001
# every switch a ladder uses is cleared around a rung, so that a rung is its own environment and nothing else
RS_SWITCHES = ("SIGOPS_RS_NO_F32MFMA", "SIGOPS_RS_NO32ROWS", "SIGOPS_RS_NOQ1", "SIGOPS_RS_NOROWS_MFMA", "SIGOPS_RS_NOROWS",
               "SIGOPS_RS_NOPAIR", "SIGOPS_RS_NOTILED", "SIGOPS_RS_NOARB", "SIGOPS_ARB_MIN")
SOS_SWITCHES = ("SIGOPS_RSOS_MINGROUPS", "SIGOPS_NO_PLAIN_RSOS", "SIGOPS_NO_RSOS", "SIGOPS_SOS_CHUNK", "SIGOPS_SOS_ONEPASS",
                "SIGOPS_SOS_3PASS", "SIGOPS_SOS_EXACT", "SIGOPS_SOS_NOALIGN", "SIGOPS_NORM_EXACT_FILT", "SIGOPS_SOS_NOXSCAN")


def rung_env(switches, kv):
    return env(**{**{k: None for k in switches}, **kv})


def ladder_noise(seed, n, nch, dt):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((n, nch)).astype(dt))


# 1. the resampler ladder
RATES = [(44100, 48000, 21770), (48000, 44100, 18376), (44100, 16000, 7257), (8000, 16000, 40002), (48000, 16000, 6667), (44100, 12000, 5443)]
COMBOS = [(8, F64), (3, F64), (4, F32)]  # tiles of 8 channels; of one (no 16-row and no narrow-store form); the Float32 MFMA form
_R1 = {"SIGOPS_RS_NO32ROWS": 1}
_R2 = {**_R1, "SIGOPS_RS_NOQ1": 1}
_R4 = {**_R2, "SIGOPS_RS_NOROWS": 1}
R_LADDER = [("R0", {}), ("R0f", {"SIGOPS_RS_NO_F32MFMA": 1}), ("R1", _R1), ("R2", _R2), ("R3", {**_R2, "SIGOPS_RS_NOROWS_MFMA": 1}), ("R4", _R4),
            ("R5", {**_R4, "SIGOPS_RS_NOPAIR": 1}), ("R6", {**_R4, "SIGOPS_RS_NOTILED": 1})]
R_CASES = [(fi, fo, nout, nch, dt, False) for fi, fo, nout in RATES for nch, dt in COMBOS] + [(44100, 48000, 9001, nch, dt, True) for nch, dt in COMBOS]
A_RATES = [(1000.0, 1000.0 * np.pi, 125664), (48000.0, 44100.5, 36751)]
A_LADDER = [("A0", {"SIGOPS_ARB_MIN": 1}), ("A1", {"SIGOPS_RS_NOARB": 1}), ("A2", {"SIGOPS_RS_NOARB": 1, "SIGOPS_RS_NOPAIR": 1}), ("A3", {"SIGOPS_RS_NOTILED": 1})]
A_CASES = [(fi, fo, nout, nch, dt) for fi, fo, nout in A_RATES for nch, dt in ((8, F64), (3, F32))]


def resampler_rungs(case):
    return [r for r in R_LADDER if r[0] != "R0f" or case[4] == F32]


def resampler_tree(case):
    fi, fo, nout, nch, dt, window = case
    x = so.Signal(ladder_noise(1000 + nch, 40000 if window else NFRAMES, nch, dt), fi * so.Hz) | so.ToFramerate(fo * so.Hz)
    if window:  # a warm start and a non-zero initial phase
        x = x | so.After(12345 * so.frames) | so.Until(9001 * so.frames)
    return x


def arbitrary_tree(case):
    fi, fo, nout, nch, dt = case
    return so.Signal(ladder_noise(2000 + nch, 40000, nch, dt), fi * so.Hz) | so.ToFramerate(fo * so.Hz)


# 2. the IIR ladder
FILTERS = {  # name: (filter, sections)
    "lowpass1_pole0": (lambda: so.Filt(so.Lowpass, 11025 * so.Hz, method=so.Butterworth(1)), 1),  # pole at 0: forgets within a tile step
    "bandstop5": (lambda: so.Filt(so.Bandstop, 0.5 * so.kHz, 2 * so.kHz), 5),
    "lowpass6": (lambda: so.Filt(so.Lowpass, 5 * so.kHz, order=12), 6),  # the most k_rsos takes
    "bandpass8": (lambda: so.Filt(so.Bandpass, 1 * so.kHz, 3 * so.kHz, method=so.Butterworth(8)), 8),  # the NS = 8 instantiation
    "bandpass10": (lambda: so.Filt(so.Bandpass, 1 * so.kHz, 4 * so.kHz, order=10), 10),  # two cascaded groups
    "highpass_slow": (lambda: so.Filt(so.Highpass, 20 * so.Hz, order=3), 2),  # slow decay: the chunk length doubles
}
I_COMBOS = [(1, F64), (5, F64), (4, F32)]
CHUNKS = (32, 64, 512, 4096, 20032)  # more than 64 chunks (32, 64), 2 to 64 (512, 4096), one chunk and a single launch (20032)
_I1 = {"SIGOPS_NO_PLAIN_RSOS": 1}
I_LADDER = ([("I0", {"SIGOPS_RSOS_MINGROUPS": 1}), ("I1", _I1)] + [("I2_%d" % c, {**_I1, "SIGOPS_SOS_CHUNK": c}) for c in CHUNKS]
            + [("I3", {"SIGOPS_SOS_ONEPASS": 1}), ("I4", {"SIGOPS_SOS_EXACT": 1}), ("I5", {**_I1, "SIGOPS_SOS_NOALIGN": 1})])
_I6a = {"SIGOPS_RSOS_MINGROUPS": 1}
_I6b = {**_I6a, "SIGOPS_NORM_EXACT_FILT": 1}
N_LADDER = [("I6a", _I6a), ("I6b", _I6b), ("I6c", {**_I6b, "SIGOPS_SOS_NOXSCAN": 1})]
I_CASES = [(f, nch, dt) for f in FILTERS for nch, dt in I_COMBOS]


def filter_rungs(case):
    return [r for r in I_LADDER if r[0] != "I0" or FILTERS[case[0]][1] <= 6]  # (k_rsos takes at most six sections)


def filter_tree(case):
    f, nch, dt = case
    return so.Signal(ladder_noise(3000 + nch, NFRAMES, nch, dt), 44.1 * so.kHz) | FILTERS[f][0]()


def resampler_id(c):
    return "%g-%g-%dx%s%s" % (c[0], c[1], c[3], np.dtype(c[4]).name, "-window" if len(c) > 5 and c[5] else "")


def filter_id(c):
    return "%s-%dx%s" % (c[0], c[1], np.dtype(c[2]).name)


def ladders():
    """every (case, rung) of the four ladders as (name, tree builder, switches to clear, the rung's switches), sunk into a
    planar host result as test_gpu_forms.py's run_host sinks them"""
    for c in R_CASES:
        for rung, kv in resampler_rungs(c):
            yield "resample %s %s" % (resampler_id(c), rung), (lambda c=c: resampler_tree(c)), RS_SWITCHES, kv
    for c in A_CASES:
        for rung, kv in A_LADDER:
            yield "arbitrary %s %s" % (resampler_id(c), rung), (lambda c=c: arbitrary_tree(c)), RS_SWITCHES, kv
    for c in I_CASES:
        for rung, kv in filter_rungs(c):
            yield "filter %s %s" % (filter_id(c), rung), (lambda c=c: filter_tree(c)), SOS_SWITCHES, kv
    for c in I_CASES:
        for rung, kv in N_LADDER:
            yield "filter|norm %s %s" % (filter_id(c), rung), (lambda c=c: filter_tree(c) | so.Normpower), SOS_SWITCHES, kv


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


# ---- the ladders on spoiled inputs (tests/test_forms_nonfinite_host.py, tests/test_gpu_forms_nonfinite.py) ------------------
# The same seeds and the same `ladder_noise` as above, with a few samples replaced by NaN or +-Inf: a plant is (channel, input
# frame, value).  No large finite values: whether those overflow depends on the order of operations.  Everything above this
# line produces what it produced before these names were added (tools/plan_fingerprint.py compares builds with it).
NAN, INF = np.nan, np.inf
WINDOW_IN = 40000                # input frames of a window case
FW_AFTER, FW_UNTIL = 30000, 5001  # the filter window cases: After(30000) | Until(5001)
FW_CASES = [(f, 5, F64) for f in FILTERS]


def spoiled(a, plants):
    """a copy of `a` (frames x channels) with every plant (channel, frame, value) written into it"""
    b = a.copy(order="F")
    for ch, frame, v in plants:
        b[frame, ch] = v
    return b


def resampler_plants(case):
    fi, fo, nout, nch, dt, window = case
    if window:  # far before the window / just before it / inside it / beyond its reach
        plants = [(0, 100, NAN), (3 if nch > 3 else nch - 2, 11330, INF), (5 if nch >= 6 else nch - 1, 15000, NAN)]
        return plants + ([(nch - 1, 30000, NAN)] if nch == 8 else [])
    return edge_plants(NFRAMES, nch)


def edge_plants(n, nch):
    """the first frame of channel 0, the middle and the last frame of the last channel, and one more channel where there are four"""
    return [(0, 0, NAN), (nch - 1, 10007, INF), (nch - 1, n - 1, NAN)] + ([(3, 4999, -INF)] if nch >= 4 else [])


def resampler_tree_spoiled(case):
    """`resampler_tree(case)` on a spoiled copy of its noise: (tree, plants)"""
    fi, fo, nout, nch, dt, window = case
    plants = resampler_plants(case)
    x = so.Signal(spoiled(ladder_noise(1000 + nch, WINDOW_IN if window else NFRAMES, nch, dt), plants), fi * so.Hz) | so.ToFramerate(fo * so.Hz)
    if window:
        x = x | so.After(12345 * so.frames) | so.Until(9001 * so.frames)
    return x, plants


def arbitrary_tree_spoiled(case):
    """`arbitrary_tree(case)` on a spoiled copy of its noise: (tree, plants)"""
    fi, fo, nout, nch, dt = case
    plants = edge_plants(40000, nch)
    return so.Signal(spoiled(ladder_noise(2000 + nch, 40000, nch, dt), plants), fi * so.Hz) | so.ToFramerate(fo * so.Hz), plants


def filter_plants(case):
    """frames 4095 and 4096 are a chunk's end and start for the chunk lengths 32, 64, 512 and 4096"""
    f, nch, dt = case
    return {5: [(0, 0, NAN), (1, 4095, INF), (3, 4096, -INF), (4, NFRAMES - 1, NAN)],
            4: [(0, 4095, NAN), (2, 4096, INF), (3, NFRAMES - 1, NAN)],
            1: [(0, 12319, NAN)]}[nch]


def filter_data_spoiled(case):
    f, nch, dt = case
    return spoiled(ladder_noise(3000 + nch, NFRAMES, nch, dt), filter_plants(case))


def filter_tree_spoiled(case):
    """`filter_tree(case)` on a spoiled copy of its noise: (tree, plants)"""
    return so.Signal(filter_data_spoiled(case), 44.1 * so.kHz) | FILTERS[case[0]][0](), filter_plants(case)


FW_PLANTS = [(0, 100, NAN), (1, 29990, INF), (3, 32000, NAN)]  # a decay time and more before the window / just before it / inside it


def filter_window_data(case, plants=FW_PLANTS):
    f, nch, dt = case
    return spoiled(ladder_noise(4000 + nch, WINDOW_IN, nch, dt), plants)


def filter_window_tree(case, plants=FW_PLANTS, window=True):
    """a filter of the ladder on 40 000 frames behind After(30000) | Until(5001) (window=False: the whole filtered signal):
    (tree, plants)"""
    x = so.Signal(filter_window_data(case, plants), 44.1 * so.kHz) | FILTERS[case[0]][0]()
    if window:
        x = x | so.After(FW_AFTER * so.frames) | so.Until(FW_UNTIL * so.frames)
    return x, plants


OVERFLOW_CASE = (8000, 16000, 40002, 8, F64, False)  # rung R0: k_resample_periodic, two outputs per period


def overflow_tree(half=False):
    """the 8 -> 16 kHz case with a NaN at every fourth input frame of channel 5 (half: of its first half only): more (tile, group)
    entries than the periodic resampler's list holds (csrc/sigops_internal.h kRsNfCap).  (tree, plants)"""
    plants = [(5, k, NAN) for k in range(0, NFRAMES // 2 if half else NFRAMES, 4)]
    return so.Signal(spoiled(ladder_noise(1000 + 8, NFRAMES, 8, F64), plants), 8000 * so.Hz) | so.ToFramerate(16000 * so.Hz), plants


def rs_nf_cap():
    """kRsNfCap as the kernels have it"""
    import re

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "signaloperators.jl_amd", "csrc", "sigops_internal.h")).read()
    return int(re.search(r"constexpr uint32_t kRsNfCap = (\d+);", text).group(1))


def forgotten(plants):
    """the plants with every one at frame 100 replaced by 0.0: what a filter started from rest behind that frame sees of it"""
    return [(ch, frame, 0.0 if frame == 100 else v) for ch, frame, v in plants]
