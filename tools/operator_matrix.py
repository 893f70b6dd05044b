"""One operator at a time over 1.25e7 frames x 8 channels (Float64): looking for cliffs outside the benches' shapes.
Per row: WARM untimed executes (default 20: the chip raises its clock over the first ~25 ms of a kernel after an idle gap, and
with 3 the matrix-heavy rows read 10 - 25 % above their steady state), then the mean of REPS (default 30) between two events."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import sigops_amd as so

nch, n = int(os.environ.get("NCH", "8")), int(float(os.environ.get("FRAMES", "12.5e6")))
fs = 44.1 * so.kHz
TDT, NDT = (torch.float32, np.float32) if os.environ.get("F32") else (torch.float64, np.float64)
x = torch.randn((nch, n), dtype=TDT, device="cuda").t()
y = torch.randn((nch, n), dtype=TDT, device="cuda").t()
z = torch.randn((nch, n // 2), dtype=TDT, device="cuda").t()
X, Y, Z = so.Signal(x, fs), so.Signal(y, fs), so.Signal(z, fs)
tone = so.Signal(so.sin, ω=1 * so.kHz)


def INTERP_TABLE(kn, kind):
    r = np.random.default_rng(kn)
    xp = np.linspace(-4.0, 4.0, kn) if kind == "uniform" else np.sort(r.uniform(-4.0, 4.0, kn))
    return xp, r.standard_normal(kn)


def POS(kind):
    """device-resident Float64 positions for the `sampleat` rows, n x nch (one row of positions per channel, so that a row
    streams what `Mix(x, y)` streams: two reads and one write per sample)"""
    p = torch.empty((nch, n), dtype=torch.float64, device="cuda")
    t = torch.arange(n, dtype=torch.float64, device="cuda")
    if kind == "identity":  # relative, a zero offset: every lane reads its own frame
        p.zero_()
    elif kind == "vibrato":  # relative: a delay of 1 .. 9 frames that moves at 0.5 Hz
        p[:] = -(5.0 + 4.0 * torch.sin(t * (2.0 * np.pi * 0.5 / 44100.0)))
    elif kind == "random":  # uniform over the whole table
        p.uniform_(0.0, float(n - 1))
    else:  # a wavetable of 2048 frames read at 1.37 frames per frame, a different phase per channel
        p[:] = t * 1.37 + 17.0 * torch.arange(nch, dtype=torch.float64, device="cuda").reshape(-1, 1)
    return so.Signal(p.t(), fs)


cases = {
    "copy (Until)": lambda: X | so.Until(n * so.frames),
    # `Cumsum(x)` (include/sigops.h SO_NODE_CUMSUM, csrc/k_cumsum.hip): reduce-then-scan, two reads and one write per sample
    # -- 1.5 x the bytes of the copy row above, its yardstick; `vco`: a 2048-frame wavetable read at the running sum of a
    # per-frame increment (1.37 frames +- 20 %, a different trajectory per channel), `SampleAt` over `Cumsum`
    "cumsum": lambda: so.Cumsum(X),
    "vco": lambda: so.SampleAt(so.Signal(x[:2048], fs), so.Cumsum(so.Signal((1.37 + 0.2 * x.t().clamp(-1.0, 1.0).to(torch.float64)).t(), fs)), wrap=True),
    # `Recur(a, b)` / `OnePole` / `PeakDecay` (include/sigops.h SO_NODE_RECUR, csrc/k_recur.hip): reduce-then-scan over Cumsum's
    # tree on pairs; a constant a streams what `cumsum` streams (two reads and one write per sample), a coefficient row per
    # channel (A, U[0.99, 1)) is read twice too: 40 bytes a sample against 24; `onepole` adds the map that scales x; the
    # yardsticks are the `cumsum` and `copy (Until)` rows above
    "recur const": lambda: so.Recur(0.999, X),
    "recur signal": lambda: so.Recur(A(), X),
    "onepole": lambda: so.OnePole(X, 1 * so.kHz),
    "peakdecay": lambda: so.PeakDecay(X, 50 * so.ms),
    # `Recur2(a1, a2, b)` / `Resonator` / `Sweep` (include/sigops.h SO_NODE_RECUR2, csrc/k_recur2.hip): reduce-then-scan over
    # Cumsum's tree on the affine maps of the state (y[n], y[n-1]); constants stream what `cumsum` streams (24 bytes a
    # sample), a row per channel of a1 (A1, a resonator's 2 r cos(theta)) and of a2 (A2, -r^2) is read twice too: 56 bytes a
    # sample; `resonator` adds the map that scales x, `sweep` an fc signal per channel: two delays (`sample_at`), the three
    # maps that form a1, a2 and b, then the scan (STEPS=1 prints their times: what fusing the maps into the scan's loads
    # would save); the yardsticks are the `cumsum`, `recur signal` and `copy (Until)` rows above
    "recur2 const": lambda: so.Recur2(1.8, -0.9, X),
    "recur2 signal": lambda: so.Recur2(A1(), A2(), X),
    "resonator": lambda: so.Resonator(X, 1 * so.kHz, 50 * so.Hz),
    "sweep": lambda: so.Sweep(X, so.Lowpass, FC(), 2.0),
    # `MovingMax(x, w)` / `MovingMin(x, w)` (include/sigops.h SO_NODE_MOVING, csrc/k_moving.hip): a window of 480 frames is the
    # one-launch form (a tile and its halo in LDS: 1 + 479 / 2048 reads and one write per sample), causal and centred; 48000
    # frames is the long form (block maxima, a sparse table, two blocks recomputed per tile: about three reads and one write);
    # the Float32 row moves half the bytes; the yardstick is the `copy (Until)` row above
    "movingmax 480": lambda: so.MovingMax(X, 480),
    "movingmax 480 ahead": lambda: so.MovingMax(X, 480, center=True),
    "movingmax 48000": lambda: so.MovingMax(X, 48000),
    "movingmin 480 f32": lambda: so.MovingMin(so.Signal(x.t().to(torch.float32).t(), fs), 480),
    # `MovingSum(x, w)` / `MovingMean` / `MovingRMS` (include/sigops.h SO_NODE_MOVSUM, csrc/k_movsum.hip): 480 frames is the
    # one-launch form (the tile, its halo and the lead-in to a multiple of the segment in LDS, two scans); the rms squares at
    # the load and divides and takes the root at the store; 48000 frames is the long form (block totals, the dyadic nodes'
    # levels, two images of three blocks a tile and the cover walk); the yardsticks are `copy (Until)` and `movingmax 480`
    "movingsum 480": lambda: so.MovingSum(X, 480),
    "movingrms 480": lambda: so.MovingRMS(X, 480),
    "movingmean 480 ahead": lambda: so.MovingMean(X, 480, center=True),
    "movingsum 48000": lambda: so.MovingSum(X, 48000),
    # `MovingMedian(x, w)` / `MovingQuantile(x, w, q)` (include/sigops.h SO_NODE_MOVRANK, csrc/k_movrank.hip): one form, a tile of
    # 2048 frames and its halo in LDS, every element counting its rank from window to window: about 3 (W - 1) LDS reads a
    # sample times (2048 + W - 1) / 2048, so 5 frames reads and writes each sample once like `movingmax 480`, and the time
    # grows with the window from there: 101, 480 and 1025 frames (the longest that is built) are bound by the LDS reads; the
    # Float32 row moves half the bytes; the yardsticks are `copy (Until)` and `movingmax 480`
    "movingmedian 5 center": lambda: so.MovingMedian(X, 5, center=True),
    "movingmedian 101 center": lambda: so.MovingMedian(X, 101, center=True),
    "movingquantile 480 0.1": lambda: so.MovingQuantile(X, 480, 0.1),
    "movingmedian 1025": lambda: so.MovingMedian(X, 1025),
    "movingmedian 5 f32": lambda: so.MovingMedian(so.Signal(x.t().to(torch.float32).t(), fs), 5),
    "Amplify(const)": lambda: X | so.Amplify(0.5),
    "Amplify(sin)": lambda: X | so.Amplify(tone) | so.Until(n * so.frames),
    "Mix(x, y)": lambda: so.Mix(X, Y),
    "Mix(x, y, sin) * 0.5": lambda: so.Mix(X, Y, tone) | so.Until(n * so.frames) | so.Amplify(0.5),
    "Amplify(x, y)": lambda: so.Amplify(X, Y),
    "Ramp 10 ms": lambda: X | so.Ramp(10 * so.ms),
    "RampOn 1 s": lambda: X | so.RampOn(1 * so.s),
    "FadeTo": lambda: so.FadeTo(X, Y, 1 * so.s),
    "After 1 s": lambda: X | so.After(1 * so.s),
    "Pad(zero) + 50 %": lambda: Z | so.Pad(so.zero) | so.Until(n * so.frames),
    "Pad(mirror) + 50 %": lambda: Z | so.Pad(so.mirror) | so.Until((n // 2 + n // 4) * so.frames),
    "Append(z, z)": lambda: so.Append(Z, Z),
    "Append of 16 pieces": lambda: so.Append(*[so.Signal(x[k * (n // 16):(k + 1) * (n // 16)], fs) for k in range(16)]),
    "Normpower": lambda: X | so.Normpower,
    "Normpower | Amplify(-20dB)": lambda: X | so.Normpower | so.Amplify(-20 * so.dB),
    "ToChannels(1) (sum)": lambda: X | so.ToChannels(1),
    "mono ToChannels(8)": lambda: so.Signal(x[:, :1], fs) | so.ToChannels(8),
    "Filt Lowpass o5": lambda: X | so.Filt(so.Lowpass, 3 * so.kHz),
    "Filt Lowpass o1": lambda: X | so.Filt(so.Lowpass, 3 * so.kHz, order=1),
    "Filt Bandpass o8": lambda: X | so.Filt(so.Bandpass, 1 * so.kHz, 4 * so.kHz, order=8),
    "Filt | Filt": lambda: X | so.Filt(so.Lowpass, 3 * so.kHz) | so.Filt(so.Highpass, 100 * so.Hz),
    "Filt | Normpower": lambda: X | so.Filt(so.Lowpass, 3 * so.kHz) | so.Normpower,
    "Filt FIR 101 taps": lambda: so.Filt(X, np.hanning(101) / 50.0),
    "ToFramerate 48k": lambda: X | so.ToFramerate(48 * so.kHz),
    "ToFramerate 48k | Filt": lambda: X | so.ToFramerate(48 * so.kHz) | so.Filt(so.Lowpass, 3 * so.kHz),
    "Mix(x, y) | ToFramerate": lambda: so.Mix(X, Y) | so.ToFramerate(48 * so.kHz),
    "Amplify(x, y) | ToFramerate": lambda: so.Amplify(X, Y) | so.ToFramerate(48 * so.kHz),
    "Mix(x, y) | Filt | ToFramerate": lambda: so.Mix(X, Y) | so.Filt(so.Lowpass, 3 * so.kHz) | so.ToFramerate(48 * so.kHz),
    "ToEltype(Float32)": lambda: so.ToEltype(X, np.float32),
    # `elementwise` closures (traced device programs, include/sigops.h SO_MAP_EXPR / SO_RAMP_EXPR)
    "closure tanh(2.5 x)": lambda: so.OperateOn(so.elementwise(lambda a: np.tanh(2.5 * a)), X),
    "closure hypot(x, y)": lambda: so.OperateOn(so.elementwise(lambda a, b: np.hypot(a, b)), X, Y),
    "Amplify(closure exp(-t/2))": lambda: so.Amplify(X, so.Signal(so.elementwise(lambda t: np.exp(-0.5 * t)), fs)) | so.Until(n * so.frames),
    "RampOn 1 s closure u^2": lambda: X | so.RampOn(1 * so.s, so.elementwise(lambda u: u ** 2)),
    # look-up tables (`np.interp` in a closure, include/sigops.h SO_EOP_INTERP): 17 / 1 024 / 65 536 knots over [-4, 4],
    # uniform (the search's first guess is the answer) and random (gallop + bisection); the yardstick is the tanh row above
    **{f"closure interp {kn} {kind}": (lambda t=INTERP_TABLE(kn, kind): so.OperateOn(so.elementwise(lambda a: np.interp(a, *t)), X))
       for kn in (17, 1024, 65536) for kind in ("uniform", "random")},
    # `SampleAt(x, pos)` (include/sigops.h SO_NODE_SAMPLEAT, csrc/k_sample_at.hip): the table read at device-resident
    # positions; the yardstick is the `Mix(x, y)` row above, which streams the same bytes
    "sampleat identity": lambda: so.SampleAt(X, POS("identity"), relative=True),
    "sampleat vibrato": lambda: so.SampleAt(X, POS("vibrato"), relative=True),
    "sampleat random": lambda: so.SampleAt(X, POS("random")),
    "sampleat wrap 2048": lambda: so.SampleAt(so.Signal(x[:2048], fs), POS("wavetable"), wrap=True),
    # `interp="cubic" | "sinc"` (csrc/k_sample_at_fir.hip): the same positions read through four points or through K taps of
    # the 512-phase table (K = 16 from LDS, K = 64 from L2); the yardstick of a row is the linear row of its position pattern
    "sampleat cubic identity": lambda: so.SampleAt(X, POS("identity"), relative=True, interp="cubic"),
    "sampleat cubic vibrato": lambda: so.SampleAt(X, POS("vibrato"), relative=True, interp="cubic"),
    "sampleat sinc16 vibrato": lambda: so.SampleAt(X, POS("vibrato"), relative=True, interp="sinc"),
    "sampleat sinc16 random": lambda: so.SampleAt(X, POS("random"), interp="sinc"),
    "sampleat sinc64 vibrato": lambda: so.SampleAt(X, POS("vibrato"), relative=True, interp="sinc", taps=64),
    "wavetable cubic": lambda: so.SampleAt(so.Signal(x[:2048], fs), POS("wavetable"), wrap=True, interp="cubic"),
    # `Comb(x, d, g)` / `Allpass(x, d, g)` (include/sigops.h SO_NODE_COMB, csrc/k_comb.hip): a lane per (frame mod D,
    # channel) -- an echo of 4800 frames fills the chip, a delay of 48 frames is 48 lanes a channel (the documented slow
    # corner); the yardstick is the `copy (Until)` row at the top, one read and one write per sample
    "comb 4800": lambda: so.Comb(X, 4800, 0.7),
    "comb 48": lambda: so.Comb(X, 48, 0.7),
    "allpass 347": lambda: so.Allpass(X, 347, 0.7),
    # counter-based device noise (`Signal(randn, rng=so.DeviceRNG(...))`, csrc/krand.h): the fill kernel, the same leaf as
    # an expression (hipRTC, K1's math instantiation: `case_env`), replicated to the channels, and the headline's tree
    # with the noise in place of its array leaf next to the array-leaf form (FRAMES=26.46e6 for the headline's own size)
    "noise fill (mono, n x nch)": lambda: NOISE() | so.Until(n * nch * so.frames),
    "noise expr hipRTC (mono)": lambda: NOISE() | so.Until(n * nch * so.frames),
    "noise expr K1 math (mono)": lambda: NOISE() | so.Until(n * nch * so.frames),
    "ToChannels(noise) fill": lambda: NOISE() | so.Until(n * so.frames) | so.ToChannels(nch),
    "headline, array leaf": lambda: so.Mix(tone, X) | so.Until(n * so.frames) | so.Filt(so.Bandstop, 0.5 * so.kHz, 2 * so.kHz) | so.ToFramerate(48 * so.kHz),
    "headline, noise leaf": lambda: so.Mix(tone, so.ToChannels(NOISE(), nch)) | so.Until(n * so.frames) | so.Filt(so.Bandstop, 0.5 * so.kHz, 2 * so.kHz) | so.ToFramerate(48 * so.kHz),
}
NOISE = lambda: so.Signal(so.randn, fs, rng=so.DeviceRNG(2024, 0))  # noqa: E731
A = lambda: so.Signal((0.99 + 0.01 * torch.rand((nch, n), dtype=torch.float64, device="cuda")).t(), fs)  # noqa: E731
R2 = lambda: 0.9 + 0.0999 * torch.rand((nch, n), dtype=torch.float64, device="cuda")  # noqa: E731
A1 = lambda: so.Signal((2.0 * R2() * torch.cos(3.0 * torch.rand((nch, n), dtype=torch.float64, device="cuda"))).t(), fs)  # noqa: E731
A2 = lambda: so.Signal((-R2() ** 2).t(), fs)  # noqa: E731
FC = lambda: so.Signal((1000.0 + 800.0 * torch.rand((nch, n), dtype=torch.float64, device="cuda")).t(), fs)  # noqa: E731
# environment of a case while its plan is created (the planner reads its knobs then)
case_env = {
    "noise expr hipRTC (mono)": {"SIGOPS_RANDN_NOFILL": "1", "SIGOPS_RTC": "1"},
    "noise expr K1 math (mono)": {"SIGOPS_RANDN_NOFILL": "1", "SIGOPS_RTC": "0"},
}
only = os.environ.get("ONLY")
# ONLY_ANY="copy (Until);comb": the rows whose name contains one of the pieces between semicolons (no row name has one), so
# that a row and its yardstick are timed in one process; ONLY keeps its meaning, one substring
only_any = [o for o in os.environ.get("ONLY_ANY", "").split(";") if o]
WARM, REPS = int(os.environ.get("WARM", "20")), int(os.environ.get("REPS", "30"))
for name, mk in cases.items():
    if only and only not in name:
        continue
    if only_any and not any(o in name for o in only_any):
        continue
    try:
        tree = mk()
        nout, co = so.nframes(tree), so.nchannels(tree)
        odt = np.float32 if ("Float32" in name or name.endswith(" f32") or NDT == np.float32) else np.float64
        tdt = torch.float32 if odt == np.float32 else torch.float64
        out = torch.empty((co, nout), dtype=tdt, device="cuda").t()
        saved = {k: os.environ.get(k) for k in case_env.get(name, {})}
        os.environ.update(case_env.get(name, {}))
        try:
            plan = so.Plan(so.ToChannels(tree, co), (nout, co), odt, (out.stride(0), out.stride(1)), True)
        finally:
            for k, v in saved.items():
                os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
        st = torch.cuda.current_stream().cuda_stream
        for _ in range(WARM):
            plan.execute(out.data_ptr(), st)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            plan.execute(out.data_ptr(), st)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / REPS
        stt = plan.stats()
        names = "+".join(s_["name"].replace("k_resample_", "rs_").replace("k_", "") for s_ in plan.steps())
        plan.close()
        print(f"{name:28s} {ms:8.3f} ms  {stt['algorithmic_bytes'] / ms / 1e9:6.2f} TB/s  [{names}]", flush=True)
        if os.environ.get("STEPS"):  # per-step device time of one profiled execute
            plan = so.Plan(so.ToChannels(tree, co), (nout, co), odt, (out.stride(0), out.stride(1)), True)
            plan.execute(out.data_ptr(), st)
            plan.set_profiling(1)
            plan.execute(out.data_ptr(), st)
            torch.cuda.synchronize()
            print("    " + "  ".join(f"{s_['name']} {s_['ms']:.3f}" for s_ in plan.steps()), flush=True)
            plan.close()
        del out
    except Exception as exc:  # (a case the mirror does not spell this way)
        print(f"{name:28s} skipped: {type(exc).__name__}: {str(exc)[:80]}", flush=True)

# Whole `sink` of white noise into a device-resident result, host wall clock: the counter-based generator against a NumPy
# generator (drawn on the host and uploaded).  Inside the timer: building the tree, `so.sink(tree, "torch")` -- lowering,
# plan creation, the result's allocation, the execute, the plan's check -- and a device synchronise.  SINKS sinks in a
# row in this process; the first pays the one-time costs (code object load).
if (not only or only in "whole sink of noise") and (not only_any or any(o in "whole sink of noise" for o in only_any)):
    import time

    secs, SINKS = float(os.environ.get("NOISE_SECONDS", "60")), int(os.environ.get("SINKS", "5"))
    for label, mk in (("DeviceRNG(0)", lambda: so.DeviceRNG(0)), ("np.random.default_rng(0)", lambda: np.random.default_rng(0))):
        ts = []
        for _ in range(SINKS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res, _ = so.sink(so.Signal(so.randn, fs, rng=mk()) | so.Until(secs * so.s) | so.ToChannels(nch), "torch")
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            del res
        print(f"whole sink of noise, {secs:g} s x {nch} ch, {label:26s} wall ms: " + " ".join(f"{t:.2f}" for t in ts), flush=True)
