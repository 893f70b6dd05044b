"""What the executor does for a fixed list of small trees, one JSON line per tree: to compare two builds of the library.

    python tools/plan_fingerprint.py > new.jsonl;  SIGOPS_LIB=/path/to/other/libsigops.so python tools/plan_fingerprint.py > old.jsonl

Every tree is planned once and executed THREE times into the same result, so that where the plan is eligible the direct
launches, the graph capture and a replay all run.  A line holds the SHA-256 of the result's bytes after each execute, the
plan's steps as (name, algorithmic bytes, launches) and the launch / stage / scratch / byte counts of `stats()`.  Every
kernel's summation order is fixed by the frame index, so two builds that launch the same kernels with the same arguments
print the same lines.  The trees: every entry of tests/cases.py's CASES, then one per launch routine of csrc/executor.cpp
that those do not reach, built as the tests named beside them build theirs.  Inputs are seeded.
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sigops_amd as so  # noqa: E402
from cases import CASES  # noqa: E402

FS = 44.1 * so.kHz
_seed = [0]


def noise(n, nch, dt=np.float64, dev=True):
    """seeded noise as an array leaf: device-resident [nch][n] (planar, time fastest), or a column-major host array"""
    _seed[0] += 1
    a = np.asfortranarray(np.random.default_rng(_seed[0]).standard_normal((n, nch)).astype(dt))
    return torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t() if dev else a


def sig(n, nch=2, dt=np.float64, fs=FS, dev=True):
    return so.Signal(noise(n, nch, dt, dev), fs)


def tone(n, hz=200.0, nch=2):
    return so.Signal(so.sin, FS, ω=hz * so.Hz) | so.Until(n * so.frames) | so.ToChannels(nch)


BS = lambda: so.Filt(so.Bandstop, 0.5 * so.kHz, 2 * so.kHz)  # noqa: E731
LP = lambda **k: so.Filt(so.Lowpass, 3 * so.kHz, **k)  # noqa: E731
IRR = lambda **k: sig(40000, fs=1000 * so.Hz, **k) | so.ToFramerate(1000 * np.pi * so.Hz)  # noqa: E731  (a rate without a period)


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
    pos = np.asfortranarray(np.random.default_rng(99).uniform(0, 4000, (6000, 1)))
    yield "sample_at_array", lambda: so.SampleAt(sig(4001), so.Signal(pos, FS)), {}, {}
    yield "sample_at_tree", lambda: so.SampleAt(sig(4001), so.Cumsum(so.Signal(np.abs(pos) / 4000, FS)), wrap=True), {}, {}
    yield "comb", lambda: so.Comb(sig(10007), 257, 0.7), {}, {}
    yield "cumsum_two_chunks", lambda: so.Cumsum(sig(16385)), {}, {}
    yield "norm_direct", lambda: sig(10007) | so.Normpower, {}, {}
    for layout in ("planar", "interleaved", "strided"):
        yield "host_" + layout, lambda: sig(5001, dev=False) | LP() | so.Ramp(5 * so.ms), {"where": "host", "layout": layout}, {}
    yield "chan_stride", lambda: sig(10007, 3) | LP(), {"pad": 37}, {}
    yield "mono", lambda: sig(10007, 1) | LP(), {}, {}
    yield "mono_chan_stride", lambda: sig(10007, 1) | LP(), {"pad": 37}, {}


def fingerprint(tree, dt=None, where="dev", layout="planar", pad=0):
    tree = so.engine.process_sink_params(tree)
    n, nch = so.nframes(tree), so.nchannels(tree)
    dt = np.dtype(dt or so.sampletype(tree))
    if where == "dev":  # [nch][n + pad], time fastest
        res = torch.full((nch, n + pad), float("nan"), dtype=torch.float32 if dt == np.float32 else torch.float64, device="cuda")
        strides, ptr, read = (1, n + pad), res.data_ptr(), lambda: res.cpu().numpy().tobytes()
    else:
        res = {"planar": lambda: np.empty((n, nch), dt, order="F"), "interleaved": lambda: np.empty((n, nch), dt, order="C"),
               "strided": lambda: np.empty((2 * n, nch), dt, order="F")[::2]}[layout]()
        strides, ptr, read = (res.strides[0] // res.itemsize, res.strides[1] // res.itemsize), res.ctypes.data, lambda: np.ascontiguousarray(res).tobytes()
    plan = so.Plan(so.ToChannels(tree, nch), (n, nch), dt, strides, where == "dev")
    try:
        hashes = []
        for _ in range(3):
            plan.execute(ptr, torch.cuda.current_stream().cuda_stream)
            plan.check(torch.cuda.current_stream().cuda_stream)
            hashes.append(hashlib.sha256(read()).hexdigest())
        st = plan.stats()
        return {"sha256": hashes, "steps": [(s["name"], s["algorithmic_bytes"], s["launches"]) for s in plan.steps()],
                "stats": {k: st[k] for k in ("n_launches", "n_stages", "scratch_bytes", "algorithmic_bytes")}, "executes": plan.counters()}
    finally:
        plan.close()


def main():
    todo = [(name, CASES[name], {"where": "host"}, {}) for name in sorted(CASES)] + list(extra())
    for name, build, result, env in todo:
        old = {k: os.environ.get(k) for k in env}
        os.environ.update({k: str(v) for k, v in env.items()})
        try:
            line = fingerprint(build(), **result)
        except Exception as e:  # (a tree the engine refuses is refused by both builds, in the same words)
            line = {"error": "%s: %s" % (type(e).__name__, e)}
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        print(json.dumps({"tree": name, **line}), flush=True)


if __name__ == "__main__":
    main()
