"""The matrix of rate pairs and filter designs the fused resampler + IIR kernel (k_rsos.hip) is run over by
tests/test_gpu_rsos_matrix.py, and the host tables of it that tests/test_rsos_matrix_host.py checks without a device.

`RATES` x `CORE` and `FULL_RATES` x `DESIGNS` joined are the matrix (`matrix()`).  A design's cutoffs are fractions of
fmin = min(fs_in, fs_out), so every design is valid at every rate pair; the four filters of the older k_rsos files (`KNOWN`)
keep their frequencies in Hz and run at `FULL_RATES` only.  `x | Filt | ToFramerate` filters at the OUTPUT rate (the
resampler goes under the filter), so a design's sections are those of `design.fn(rate)` at `fs_out`.

The literal tables at the end -- `GEOMETRY`, `CORE_WP`, `DECLINED` -- are what the planner gave on the device when the matrix
was last recorded (profiles/r18/rsos_matrix.txt); test_gpu_rsos_matrix.py asserts that it still does."""
from collections import namedtuple

import sigops_amd as so
from sigops_amd import FilterFn

# fs_in -> fs_out, kHz
RATES = [(44.1, 48.0), (22.05, 24.0), (32.0, 48.0), (24.0, 48.0), (16.0, 48.0), (8.0, 16.0), (22.05, 44.1), (9.6, 16.0), (48.0, 96.0),
         (48.0, 24.0), (48.0, 32.0), (48.0, 44.1), (44.1, 16.0), (22.05, 48.0)]
# (the issue's fourth was 48 -> 24 kHz: the fused step declines every downsampling pair, so all 65 designs would have been declared
#  declines, more than a quarter of the matrix with the other three.  9.6 -> 16 kHz instead: the one pair that walks the resampler
#  stage's own ten blocks with 12 k-step windows.  48 -> 24 stays in RATES with CORE, a declared decline.)
FULL_RATES = [(44.1, 48.0), (32.0, 48.0), (24.0, 48.0), (9.6, 16.0)]
HEADLINE_RATES = [(44.1, 48.0), (32.0, 48.0), (24.0, 48.0)]

_TYPES = {"lowpass": so.Lowpass, "highpass": so.Highpass, "bandpass": so.Bandpass, "bandstop": so.Bandstop}


class Design(namedtuple("Design", "name kind method bounds absolute")):
    """bounds: fractions of fmin = min(fs_in, fs_out), or Hz where `absolute`"""

    def hz(self, rate):
        return tuple(float(b) if self.absolute else float(b) * min(rate) * 1000.0 for b in self.bounds)

    def fn(self, rate):
        return FilterFn(self.kind, self.method, self.hz(rate))

    def sos(self, rate):
        """(sections, gain) at the rate the filter runs at: the output's"""
        return so.design_iir(self.fn(rate), rate[1] * 1000.0)

    def filt(self, rate):
        return so.Filt(_TYPES[self.kind], *[b * so.Hz for b in self.hz(rate)], method=self.method)

    def tree(self, src, rate):
        return src | self.filt(rate) | so.ToFramerate(rate[1] * so.kHz)


def _bw(n):
    return ("butterworth", n)


NARROW, WIDE = (0.05, 0.06), (0.02, 0.3)
# Left out of the grid: outside what the Float64 DF2T cascade itself delivers (test_rsos_matrix_host.py, admission: Float64
# against long double over 8 192 frames of noise, norm-wise, to hold 1e-10).  name: the worst figure over its output rates.
NOT_ADMITTED = {}  # (none: the worst of the grid is hp7@0.0005 at 3.1e-12, then bs6w 1.3e-12 and hp3@0.0005 9.3e-13)

_GRID = [Design(f"lp{n}@{c}", "lowpass", _bw(n), (c,), False) for n in (1, 2, 4, 5, 8, 12) for c in (0.02, 0.1, 0.25, 0.45)] \
    + [Design(f"hp{n}@{c}", "highpass", _bw(n), (c,), False) for n in (1, 3, 7) for c in (0.0005, 0.005, 0.1)] \
    + [Design(f"{k}{n}{w[0]}", kind, _bw(n), b, False) for k, kind in (("bp", "bandpass"), ("bs", "bandstop")) for n in (1, 2, 3, 4, 5, 6)
       for w, b in (("narrow", NARROW), ("wide", WIDE))] \
    + [Design("cheb4lp", "lowpass", ("chebyshev1", 4, 0.1), (0.1,), False), Design("cheb4hp", "highpass", ("chebyshev1", 4, 0.1), (0.05,), False),
       Design("cheb9lp", "lowpass", ("chebyshev1", 9, 3.0), (0.1,), False), Design("cheb9hp", "highpass", ("chebyshev1", 9, 3.0), (0.05,), False)]
# the filters of test_gpu_rsos_fold.py, test_gpu_rsos_wproj.py and test_gpu_rsos_chain4.py: the known-good points
KNOWN = [Design("known-bs5", "bandstop", _bw(5), (500.0, 2000.0), True), Design("known-hp7", "highpass", _bw(7), (200.0,), True),
         Design("known-lp7", "lowpass", _bw(7), (5000.0,), True), Design("known-lp5", "lowpass", _bw(5), (3000.0,), True)]
ALL_GRID = _GRID + KNOWN  # (what the issue listed, the designs the admission removed included)
DESIGNS = [d for d in ALL_GRID if d.name not in NOT_ADMITTED]
BY_NAME = {d.name: d for d in ALL_GRID}

# Sections 1 .. 6 (1: lp1, lp2, hp1; 2: hp3, cheb4hp; 3: lp5, bp3w, bs3w; 4: hp7; 5: bs5n, cheb9lp; 6: bp6n, bs6n), every family,
# and both sides of the fold gate amp <= 256: lp1, hp*, bs*, cheb4hp are admitted (amp 1 .. 200), lp5, bp3w, bp6n, cheb9lp declined
# (500 .. 3e4), and lp2@0.1 sits on it: amp 266 at 44.1 -> 48 kHz, 251 at 32 -> 48, 228 at 24 -> 48
CORE_NAMES = ["lp1@0.25", "lp2@0.1", "lp5@0.25", "hp1@0.0005", "hp3@0.005", "hp7@0.005", "bp3w", "bp6n", "bs3w", "bs5n", "bs6n", "cheb4hp", "cheb9lp"]
CORE = [BY_NAME[n] for n in CORE_NAMES]


def rate_id(rate):
    return f"{rate[0]:g}->{rate[1]:g}"


def matrix():
    """[(rate, design)]: CORE x RATES joined with DESIGNS x FULL_RATES, every pair once, in a fixed order"""
    out, seen = [], set()
    for rate in RATES:
        for d in (DESIGNS if rate in FULL_RATES else CORE):
            if d.absolute and max(d.bounds) >= 0.49 * min(rate) * 1000.0:  # (known-lp7's 5 kHz at 9.6 kHz: beyond the input's Nyquist rate)
                continue
            if (rate, d.name) not in seen:
                seen.add((rate, d.name))
                out.append((rate, d))
    return out


def case_id(case):
    return f"{rate_id(case[0])}/{case[1].name}"


# ---- what the device gave (test_gpu_rsos_matrix.py asserts these; profiles/r18/rsos_matrix.txt is where they were read) -----
# rate: (phase groups = blocks of 16 outputs per period the kernel walks, window slots kw = 4 ks, input frames per period M)
# (9.6 -> 16 kHz, x 5/3, walks the resampler stage's own period of ten blocks -- 160 outputs, 96 inputs --, not a 5-block super-period of
#  the kernel's own; 22.05 -> 48 kHz walks twenty blocks, two phase groups per y wave.  Own tables: 32 -> 48, 16 -> 48 and the four x 2 pairs.)
GEOMETRY = {"44.1->48": (10, 52, 147), "22.05->24": (10, 52, 147), "32->48": (3, 48, 32), "24->48": (1, 48, 8), "16->48": (3, 48, 16), "8->16": (1, 48, 8),
            "22.05->44.1": (1, 48, 8), "9.6->16": (10, 48, 96), "48->96": (1, 48, 8), "22.05->48": (20, 48, 147)}
# (rate id, CORE design): warm-up periods wp -- per rate, in CORE_NAMES' order
_WP = {"44.1->48": (1, 1, 1, 85, 18, 42, 5, 51, 5, 31, 37, 5, 35),
       "22.05->24": (1, 1, 1, 85, 18, 42, 5, 51, 5, 31, 37, 5, 35),
       "32->48": (1, 3, 4, 387, 83, 191, 22, 238, 22, 142, 170, 21, 159),
       "24->48": (3, 12, 13, 1545, 332, 771, 89, 962, 89, 570, 684, 82, 650),
       "16->48": (2, 6, 6, 773, 166, 389, 46, 491, 46, 289, 346, 42, 343),
       "8->16": (3, 12, 13, 1545, 332, 771, 89, 962, 89, 570, 684, 82, 650),
       "22.05->44.1": (3, 12, 13, 1545, 332, 771, 89, 962, 89, 570, 684, 82, 650),
       "9.6->16": (1, 1, 2, 129, 29, 65, 8, 80, 8, 48, 57, 7, 54),
       "48->96": (3, 12, 13, 1545, 332, 771, 89, 962, 89, 570, 684, 82, 650),
       "22.05->48": (1, 1, 1, 85, 19, 42, 5, 54, 5, 32, 38, 5, 37)}
CORE_WP = {(rid, name): wp for rid, wps in _WP.items() for name, wp in zip(CORE_NAMES, wps)}
# (rate id, design name or "*" for every design of the rate): why the fused step does not run it.  Every downsampling pair declines:
#   48 -> 44.1: the resampler runs on rows of 147 outputs (k_resample_rows): no multiple of it up to 4 096 outputs is 1, 2, 3, 5, 6 or 10 blocks;
#   48 -> 32: the kernel's own table fits (taps 56 + span 23: 20 k-steps, one block), the ring does not -- the planner's line reads
#     "ring 640 frames (needs 827)" -- a reason the issue did not list;
#   48 -> 24, 44.1 -> 16: no line of the planner's says why.  Estimated from 48 -> 32's 56 taps at x 2/3: 16 outputs span 32 (44) inputs and
#     some 75 (100) taps, 27 (36) k-steps.
DECLINED = {("48->44.1", "*"): "no super-period of whole blocks",
            ("48->24", "*"): "a window longer than 20 k-steps", ("48->32", "*"): "the input ring does not hold the windows in flight",
            ("44.1->16", "*"): "a window longer than 20 k-steps"}
DECLINED.update({(r, n): "too slow for a small case" for r in ("44.1->48", "32->48", "24->48", "9.6->16") for n in ("hp3@0.0005", "hp7@0.0005")})


def declined(case):
    rate, d = case
    return DECLINED.get((rate_id(rate), d.name)) or DECLINED.get((rate_id(rate), "*"))
