"""Host-side mirror of the SignalOperators.jl operator API (layers L3-L5 of
SURVEY.md §1): lazy tree construction, traits / length algebra, promotion
(`Uniform`, `Format`) and the `ToFramerate` rewrite rules.  Nothing here computes
samples: `sink` hands the tree to the HIP engine through the C-ABI
(`lowering.py` -> include/sigops.h).

The reference host language is Julia; Julia is not present in this image
(SURVEY.md probe table), so the host side above the C-ABI is written in Python with
the same names, argument meaning and error behaviour as the reference so that the
parity tests read like test/runtests.jl.  Piping `x |> Until(5s)` is spelled
`x | Until(5*s)` (or `pipe(x, Until(5*s), ...)`).

Every class/function cites the reference definition it mirrors.
"""
import math
import operator

import numpy as np

from . import units as U
from .trace import Elementwise, elementwise  # noqa: F401
from .units import Quantity


class ErrorException(Exception):
    """Julia's ErrorException: what the reference's `error(msg)` throws."""


def error(msg):
    raise ErrorException(msg)


# --------------------------------------------------------------------------
# lengths: reference src/inflen.jl, src/signal.jl:28-37, src/numbers.jl:5-9
class _InfLen:
    def __repr__(self):
        return "inflen"


inflen = _InfLen()


class Extended:  # src/signal.jl:31-36
    def __init__(self, n):
        self.len = n

    def __repr__(self):
        return f"Extended({self.len})"


class _NumberExtended:  # src/numbers.jl:5-7
    def __repr__(self):
        return "numextend"


numextend = _NumberExtended()


def isknowninf(n):  # src/inflen.jl:21-22
    return n is inflen or isinstance(n, (Extended, _NumberExtended))


def isinf(n):
    return isknowninf(n)


def cleanextend(n):  # src/signal.jl:29,35 src/numbers.jl:9
    return inflen if isknowninf(n) else n


F32 = np.dtype("float32")
F64 = np.dtype("float64")
I64 = np.dtype("int64")


def promote_type(a, b):
    """Julia promote_type restricted to Float32 / Float64 / Int64"""
    if a == F64 or b == F64:
        return F64
    if a == F32 or b == F32:
        return F32
    return I64


def float_type(t):
    return F64 if t == I64 else t


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


# --------------------------------------------------------------------------
class AbstractSignal:
    """reference src/signal.jl:18-53 (IsSignal{T,Fs,L} traits as attributes)"""

    __array_ufunc__ = None
    fs = None  # framerate(x); None == missing
    nch = 1  # nchannels(x)
    dtype = F64  # sampletype(x)
    evaltrait = "computed"  # EvalTrait(x) src/signal.jl:154-175
    children = ()

    def nframes_helper(self):
        raise NotImplementedError

    def __init_subclass__(cls, **kw):
        # signals are immutable once built and their length is asked for again and again (every node of
        # every lowering, every block of so.stream): remember it per object
        super().__init_subclass__(**kw)
        f = cls.__dict__.get("nframes_helper")
        if f is not None and not getattr(f, "_memo", False):
            def helper(self, _f=f):
                d = self.__dict__
                if "_nframes_memo" not in d:
                    d["_nframes_memo"] = _f(self)
                return d["_nframes_memo"]
            helper._memo = True
            helper.__doc__ = f.__doc__
            cls.nframes_helper = helper

    def __or__(self, fn):  # x |> f
        if callable(fn):
            return fn(self)
        return NotImplemented


def nframes(x):  # src/signal.jl:27
    x = _assignal(x)
    return cleanextend(x.nframes_helper())


def nchannels(x):
    return _assignal(x).nch


def framerate(x):
    if isinstance(x, tuple) and len(x) == 2:
        return float(x[1])
    return _assignal(x).fs


def sampletype(x):
    return _assignal(x).dtype


def duration(x):
    x = _assignal(x)
    return x.duration()


class Curried:
    """`Until(5s)` etc. return functions in the reference; this wrapper also makes
    `array | Until(...)` work (numpy defers to __ror__)."""

    __array_ufunc__ = None

    def __init__(self, fn):
        self.fn = fn

    def __call__(self, x):
        return self.fn(x)

    def __ror__(self, x):
        return self.fn(x)


def pipe(x, *fns):
    for f in fns:
        x = f(x)
    return x


# --------------------------------------------------------------------------
# leaves
class ArraySig(AbstractSignal):
    """arrays and (array,fs) tuples as signals, reference src/arrays.jl:35-132"""

    evaltrait = "data"

    def __init__(self, data, fs=None):
        if _is_torch(data):
            shape = tuple(data.shape)
            dt = {"torch.float32": F32, "torch.float64": F64}.get(str(data.dtype))
            if dt is None:
                error("device arrays must be float32 or float64")
        else:
            data = np.asarray(data)
            shape = data.shape
            dt = data.dtype
            if dt.kind in "iu" or dt.kind == "b":
                dt = I64
        if len(shape) not in (1, 2):
            error("Array must have 1 or 2 dimensions to be treated as a signal.")
        self.data = data
        self.fs = None if fs is None else float(fs)
        self.nch = 1 if len(shape) == 1 else int(shape[1])
        self.n = int(shape[0])
        self.dtype = np.dtype(dt)
        self.container = None  # SampleBuf / AxisArray / DimensionalArray class the data came in (root type)
        self.virtual = None  # engine.BlockStream: (address frame 0 would have, frame stride, channel stride, first resident frame)

    def nframes_helper(self):
        return self.n

    def duration(self):
        return None if self.fs is None else self.n / self.fs


class NumberSig(AbstractSignal):
    """reference src/numbers.jl:1-64"""

    def __init__(self, val, fs=None, dB=False, dtype=None):
        if dtype is None:
            if isinstance(val, (bool, int, np.integer)):
                dtype = I64
            elif isinstance(val, np.floating) and val.dtype == F32:
                dtype = F32
            else:
                dtype = F64
        self.val = val
        self.fs = fs
        self.dB = dB
        self.dtype = np.dtype(dtype)
        self.nch = 1

    def nframes_helper(self):
        return numextend

    def duration(self):
        return inflen


SIN, COS, IDENTITY, RANDN = "sin", "cos", "identity", "randn"
OPAQUE = "opaque"  # any other callable: evaluated on the host at sink time and handed to the engine as an array leaf
EXPR = "expr"  # an `elementwise` closure: traced into a device program over the time argument (trace.py)


def _fn_code(fn):
    import builtins  # noqa: F401

    if fn in (SIN, COS, IDENTITY, RANDN):
        return fn
    if fn is np.sin or fn is math.sin:
        return SIN
    if fn is np.cos or fn is math.cos:
        return COS
    if fn is randn or fn is np.random.randn:
        return RANDN
    if getattr(fn, "__name__", "") == "identity":
        return IDENTITY
    return None


def identity(x):
    return x


def randn(*a):
    """marker for Signal(randn) (reference src/functions.jl:98-114)"""
    return np.random.randn(*a)


class DeviceRNG:
    """A counter-based generator for `Signal(randn, fs, rng=DeviceRNG(seed, stream))`: the noise is made on the GPU and
    frame `i` of the leaf is a pure function of `(seed, stream, i)` -- Philox4x32-10 on the pair index `i >> 1`, the
    two 53-bit uniforms through Box-Muller ("Device noise").  So a window, a block of `stream`, a time-range
    shard and a second execute of a plan all see the same samples, and nothing is drawn on the host or uploaded.

    The one deliberate difference from a stateful NumPy `Generator`: the object holds no state.  Two leaves with equal
    `(seed, stream)` are the SAME noise; independent noises take different streams (`g.spawn(k)` is
    `DeviceRNG(seed, stream + k)`).  `seed` and `stream` are unsigned 64-bit; the value is immutable, compares and
    hashes by `(seed, stream)`."""

    __slots__ = ("_seed", "_stream")

    def __init__(self, seed, stream=0):
        for name, v in (("seed", seed), ("stream", stream)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < 1 << 64:
                error(f"DeviceRNG: {name} must be an integer in [0, 2^64)")
        object.__setattr__(self, "_seed", int(seed))
        object.__setattr__(self, "_stream", int(stream))

    seed = property(lambda self: self._seed)
    stream = property(lambda self: self._stream)

    def __setattr__(self, name, value):
        raise AttributeError("DeviceRNG is immutable")

    def spawn(self, k):
        """the generator `k` streams further on (same seed): an independent noise"""
        return DeviceRNG(self._seed, (self._stream + int(k)) % (1 << 64))

    def __eq__(self, other):
        return isinstance(other, DeviceRNG) and (self._seed, self._stream) == (other._seed, other._stream)

    def __hash__(self):
        return hash(("DeviceRNG", self._seed, self._stream))

    def __repr__(self):
        return f"DeviceRNG(seed={self._seed}, stream={self._stream})"


class FuncSig(AbstractSignal):
    """SignalFunction, reference src/functions.jl:11-60,88-96"""

    def __init__(self, fn, fs=None, omega=None, phi=0.0, rng=None, pyfn=None):
        self.fn = fn  # code string
        self.pyfn = pyfn  # OPAQUE: the host callable itself
        self.fs = fs
        self.omega = omega
        self.phi = float(phi)
        self.rng = rng
        self.nch = 1
        self.dtype = F64

    def nframes_helper(self):
        return inflen

    def duration(self):
        return inflen


# --------------------------------------------------------------------------
class WrappedSignal(AbstractSignal):
    """reference src/wrapping.jl:3-19"""

    def __init__(self, child):
        self.signal = child
        self.children = (child,)
        self.fs = child.fs
        self.nch = child.nch
        self.dtype = child.dtype

    @property
    def evaltrait(self):
        return self.signal.evaltrait

    def nframes_helper(self):
        return self.signal.nframes_helper()

    def duration(self):
        return self.signal.duration()


def _tolen_arith(n):
    return n


class CutApply(WrappedSignal):
    """Until / After, reference src/cutting.jl:6-32,130-138"""

    def __init__(self, child, time, kind):
        super().__init__(child)
        self.time = time
        self.kind = kind  # "until" | "after"

    @property
    def evaltrait(self):
        if self.kind == "after":
            return "data"  # src/cutting.jl:138
        return self.signal.evaltrait

    def resolvelen(self):  # src/cutting.jl:32
        return U.inframes_int(U.maybeseconds(self.time), self.fs)

    def nframes_helper(self):
        n = self.signal.nframes_helper()
        L = self.resolvelen()
        if L is None or n is None:
            return None
        if self.kind == "until":  # :130
            L = max(0, L)
            return L if isknowninf(n) else min(n, L)
        if isknowninf(n):  # :134 (inflen - L == inflen)
            return n
        return min(max(n - L, 0), n)

    def duration(self):
        d = self.signal.duration()
        t = U.inseconds(U.maybeseconds(self.time), self.fs)
        if d is None or t is None:
            return None
        if self.kind == "until":
            t = max(0, t)
            return t if isknowninf(d) else min(d, t)
        if isknowninf(d):
            return d
        return min(max(d - t, 0), d)


class PaddedSignal(WrappedSignal):
    """Pad / Extend, reference src/padding.jl:3-19"""

    def __init__(self, child, pad, extending=False):
        super().__init__(child)
        self.pad = pad
        self.extending = extending

    def nframes_helper(self):
        if self.extending:
            return Extended(nframes(self.signal))
        return inflen

    def duration(self):
        return inflen


class AppendSignals(WrappedSignal):
    """reference src/appending.jl:3-17"""

    def __init__(self, signals, length, dtype):
        super().__init__(signals[0])
        self.signals = tuple(signals)
        self.children = self.signals
        self.len = length
        self.dtype = dtype

    def nframes_helper(self):
        return self.len

    def duration(self):
        ds = [c.duration() for c in self.signals]
        if any(d is None for d in ds):
            return None
        if any(isknowninf(d) for d in ds):
            return inflen
        return sum(ds)


class RampSignal(WrappedSignal):
    """reference src/ramps.jl:6-26 — a GAIN signal shaped like its child"""

    def __init__(self, direction, child, time, fn):
        super().__init__(child)
        self.direction = direction  # "on" | "off"
        self.time = time
        self.fn = fn  # "sinramp" | "identity"
        self.dtype = float_type(child.dtype)

    def resolvelen(self):  # :26
        n = U.inframes_int(U.maybeseconds(self.time), self.fs)
        return None if n is None else max(1, n)


class NormedSignal(WrappedSignal):
    """reference src/filters.jl:266-275"""

    def __init__(self, child):
        super().__init__(child)
        self.dtype = float_type(child.dtype)


class FilterFn:  # src/filters.jl:5-12
    def __init__(self, design, method, args):
        self.design = design  # "lowpass" | "highpass" | "bandpass" | "bandstop"
        self.method = method  # ("butterworth", order) | ("chebyshev1", order, ripple)
        self.args = tuple(args)  # Hz


class RawFilterFn:  # src/filters.jl:89-92
    def __init__(self, sos, gain=1.0):
        self.sos = np.ascontiguousarray(np.asarray(sos, dtype=np.float64).reshape(-1, 6))
        self.gain = float(gain)


class RawFirFn:
    """Filt(x, h) with FIR coefficients h: DF2TFilter(PolynomialRatio(h, [1])), y[n] = sum_k h[k] x[n-k]"""

    def __init__(self, h):
        self.h = np.ascontiguousarray(np.asarray(h, dtype=np.float64).ravel())


class ResamplerFn:  # src/util.jl:12-15
    def __init__(self, ratio, fs):
        self.ratio = ratio  # (num, den) tuple or float
        self.fs = fs


class FilteredSignal(WrappedSignal):
    """reference src/filters.jl:98-114,159-167"""

    evaltrait = "computed"

    def __init__(self, child, fn, blocksize, newfs):
        super().__init__(child)
        self.fn = fn
        self.blocksize = int(blocksize)
        self.fs = newfs
        self.dtype = float_type(child.dtype)

    @property
    def evaltrait(self):  # noqa: F811
        return "computed"

    def nframes_helper(self):  # :159-167
        cfs = self.signal.fs
        if cfs is None:
            return None
        n = self.signal.nframes_helper()
        if self.fs == cfs:
            return n
        if isknowninf(n) or n is None:
            return n
        return int(math.ceil(n * self.fs / cfs))

    def duration(self):
        return self.signal.duration()


def _need_x(self, n, skip):
    """demand rule: `x` up to frame n, from frame 0 (the recurrence, the sum, starts there: the frames before a window are
    computed too)"""
    return [(self.signal, n, 0)]


def _need_every_child(self, n, skip):
    """demand rule: every input up to frame n, from frame 0 (the recurrence starts there whatever window reads it)"""
    return [(c, n, 0) for c in self.children]


SCAN_CHUNK = 16384  # the chunk of Cumsum / Recur / Recur2 (csrc/kernels.h kCumsumChunk): the frames their state is carried at


def _scan_checkpoint(self, resume, need):
    """checkpoint rule of the scans: the first frame of the last chunk that holds a frame read, k1 = (need - 1) // chunk -- a
    push that ends exactly on a chunk boundary has not entered the next chunk --, and `resume` where that is no later"""
    return max(resume, (need - 1) // SCAN_CHUNK * SCAN_CHUNK) if need > 0 else resume


def _need_x_ahead(self, n, skip):
    """demand rule: the window of the last frame reaches `ahead` frames further; the frames before a window's `back` come
    along"""
    return [(self.signal, n + self.ahead, 0)]


class StageSignal(AbstractSignal):
    """A node the device computes in a stage of its own and nothing else knows how to compute (no reference counterpart;
    DESIGN.md "Where a device-only node lives").  `ToFramerate`, `lowering._demand`, `lowering.lower`, `engine._streamable`
    and `sharding` each treat all of them in one branch, from what a subclass declares:

    * `family`: the name refusals print;
    * `rebuild(f)`: the node of the same class and parameters with `f` applied to every child that takes a missing frame
      rate (a rate the node has is resampled like any computed signal's);
    * `demand(n, skip)`: `(child, frames, skip)` for every child the first `n` frames read -- `frames` is capped at the
      child's length, `None` is the child whole;
    * `node` and `fields()`: the `SO_NODE_*` kind by name and the node's `i* / l* / d* / p* / s*` fields (include/sigops.h;
      an array stands for the pointer to it and is kept alive by the lowering);
    * `not_streamable`: why a stream with nowhere to keep state refuses it; `shard_order`, `shard_tail`: where its
      multi-GPU refusal stands among those of a tree that holds several families (lowest first, the first one met among
      equals), and what the refusal adds after "is not built";
    * `stream_doubles()`: what a `BlockStream` carries for the node from one push to the next, in Float64 per channel --
      0: nothing (its frames depend on a window of the input, which the stream keeps); a positive count: the record of
      include/sigops.h "Carried state"; None: nothing would do, the node is not streamable;
    * `stream_checkpoint(resume, need)`, for a node that carries a record: the frame whose entering state the record it
      leaves holds when it resumed at `resume` and the frames `[0, need)` are read -- the planner's rule
      (`Plan::process_from_frame_0`), which a `BlockStream` holds the plan's report to.

    `carry` is not a declaration: a `BlockStream` sets it on the nodes of one push's tree, `(resume frame, address of the
    carry-in record, address of the carry-out record)`, and the lowering writes it into the node's `s0 / p0 / p1`.  A node
    nobody attached one to lowers as `fields()` says."""

    evaltrait = "computed"
    shard_tail = ""
    carry = None

    def _like(self, timed, nch, dtype):
        """the length, duration and frame rate of the child `timed`"""
        self._timed = timed
        self.fs = timed.fs
        self.nch = nch
        self.dtype = dtype

    def nframes_helper(self):
        return self._timed.nframes_helper()

    def duration(self):
        return self._timed.duration()


class SampleAtSignal(StageSignal):
    """`SampleAt(x, pos)`: the table `x` read at the positions the signal `pos` gives, with linear interpolation --
    `interp="cubic"`: Catmull-Rom; `interp="sinc"`: `taps` taps of a Kaiser-windowed sinc with its pass-band edge at
    `cutoff` of the table's Nyquist -- (no reference counterpart; include/sigops.h SO_NODE_SAMPLEAT, DESIGN.md
    "SampleAt").  It has the length and frame rate of `pos`, the channels of `x`, and is Float64 like `np.interp`."""

    family = "SampleAt"
    node = "SAMPLEAT"
    not_streamable = "reads its table at any position, and a stream keeps only a tail of its input resident"
    shard_order = 0

    def stream_doubles(self):  # (any frame of the table may be read)
        return None

    def __init__(self, x, pos, left=0.0, right=0.0, relative=False, wrap=False, interp="linear", taps=0, cutoff=0.0):
        self.interp = interp  # "linear" | "cubic" | "sinc"
        self.taps = int(taps)  # sinc only (0 otherwise)
        self.cutoff = float(cutoff)  # sinc only (0.0 otherwise)
        self.signal = x
        self.pos = pos
        self.children = (x, pos)
        self.left = float(left)
        self.right = float(right)
        self.relative = bool(relative)
        self.wrap = bool(wrap)
        self._like(pos, x.nch, F64)

    def rebuild(self, f):
        # a rate the positions do not have yet is theirs to take (never the table's: it is a table of frames, its own
        # rate is not consulted)
        return SampleAtSignal(self.signal, f(self.pos), self.left, self.right, self.relative, self.wrap, self.interp, self.taps, self.cutoff)

    def demand(self, n, skip):
        # the table whole (any frame of it may be read), the positions for the frames the sink reaches
        return [(self.signal, None, 0), (self.pos, n, skip)]

    def fields(self):
        r = dict(i0=(1 if self.relative else 0) | (2 if self.wrap else 0), d0=self.left, d1=self.right)
        if self.interp != "linear":  # ("linear": the node as it always was, i1 = 0)
            r["i1"] = SAMPLEAT_INTERP.index(self.interp)
        if self.interp == "sinc":  # the rows of h, then the rows of dh (include/sigops.h)
            tab = np.concatenate([a.ravel() for a in sampleat_taps(self.taps, self.cutoff)])
            r.update(i2=self.taps, p0=tab, s0=int(tab.size), d2=self.cutoff)
        return r


class CombSignal(StageSignal):
    """`Comb(x, d, g)` / `Allpass(x, d, g)`: a feedback delay line of `delay` frames over `x`,
    `y[n] = (b0 x[n] + bD x[n - D]) + a y[n - D]` (no reference counterpart; include/sigops.h SO_NODE_COMB, DESIGN.md
    "Comb").  It has the length, frame rate and channels of `x` and is Float64."""

    family = "Comb / Allpass"
    node = "COMB"
    not_streamable = "would have to carry the D frames of its delay line from one push to the next, and that is not built"
    shard_order = 1  # its frames depend on every frame before them: a rank cannot start in the middle, and handing the state on is not built
    demand = _need_x

    def stream_doubles(self):  # (x, y) of the last frame of each of the D residue classes
        return 2 * self.delay

    def stream_checkpoint(self, resume, need):  # where the push ended
        return need

    def __init__(self, x, delay, b0, bD, a):
        self.signal = x
        self.children = (x,)
        self.delay = int(delay)
        self.b0 = float(b0)
        self.bD = float(bD)
        self.a = float(a)
        self._like(x, x.nch, F64)

    def rebuild(self, f):
        # the delay is a number of frames (a time was converted with the rate x had): a missing rate goes to x
        return CombSignal(f(self.signal), self.delay, self.b0, self.bD, self.a)

    def fields(self):
        return dict(l0=self.delay, d0=self.b0, d1=self.bD, d2=self.a)


class CumsumSignal(StageSignal):
    """`Cumsum(x)`: the running sum of `x` per channel, summed over one fixed tree (no reference counterpart;
    include/sigops.h SO_NODE_CUMSUM, DESIGN.md "Cumsum").  It has the length, frame rate and channels of `x` and is
    Float64."""

    family = "Cumsum / Integrate"
    node = "CUMSUM"
    not_streamable = ("would have to carry its running sum (and its place in the summation tree) from one push to the next, "
                      "and that is not built")
    shard_order = 1  # (as Comb)
    demand = _need_x

    def stream_doubles(self):  # the running total that enters a chunk
        return 1

    stream_checkpoint = _scan_checkpoint

    def __init__(self, x):
        self.signal = x
        self.children = (x,)
        self._like(x, x.nch, F64)

    def rebuild(self, f):  # the sum runs over frames, whatever rate they have
        return CumsumSignal(f(self.signal))

    def fields(self):
        return {}


_HALO = ": a rank would need `back` frames of the rank before it and `ahead` of the one after (a halo exchange)"


class MovingSignal(StageSignal):
    """`MovingMax(x, w)` / `MovingMin(x, w)`: per channel the greatest (least) sample of `x` over the frames
    `[n - back, n + ahead]`, clipped to the signal (no reference counterpart; include/sigops.h SO_NODE_MOVING, DESIGN.md
    "Moving extrema").  It has the length, frame rate, channels and sample type of `x`."""

    family = "MovingMax / MovingMin"
    node = "MOVING"
    not_streamable = ("would have to keep the `back` input frames of its window from one push to the next and hold `ahead` "
                      "output frames back, and that is not built")
    shard_order = 2  # a rank's window reaches into its neighbours' frames
    shard_tail = _HALO
    demand = _need_x_ahead

    def stream_doubles(self):  # (a window of the input, which the stream keeps)
        return 0

    def __init__(self, x, back, ahead, is_min):
        self.signal = x
        self.children = (x,)
        self.back = int(back)
        self.ahead = int(ahead)
        self.is_min = bool(is_min)
        self._like(x, x.nch, x.dtype)

    def rebuild(self, f):  # the window is counted in frames, whatever rate they have
        return MovingSignal(f(self.signal), self.back, self.ahead, self.is_min)

    def fields(self):
        return dict(l0=self.back, l1=self.ahead, i0=1 if self.is_min else 0)


class MovingSumSignal(StageSignal):
    """`MovingSum(x, w)` / `MovingMean(x, w)` / `MovingRMS(x, w)`: per channel the sum (the mean, the root of the mean square)
    of `x` over the frames `[n - back, n + ahead]`, clipped to the signal, over one fixed summation tree (no reference
    counterpart; include/sigops.h SO_NODE_MOVSUM, DESIGN.md "Moving sums").  It has the length, frame rate and channels of
    `x` and is Float64.  `op`: 0 sum, 1 mean, 2 rms."""

    family = "MovingSum / MovingMean / MovingRMS"
    node = "MOVSUM"
    not_streamable = ("would have to keep the `back` input frames of its window from one push to the next, hold `ahead` output "
                      "frames back and keep its place in the summation tree, and that is not built")
    shard_order = 3  # (as Moving)
    shard_tail = _HALO + ", summed over the whole signal's tree"
    demand = _need_x_ahead

    def stream_doubles(self):  # (as Moving: the summation tree is fixed by the absolute frame)
        return 0

    def __init__(self, x, back, ahead, op):
        self.signal = x
        self.children = (x,)
        self.back = int(back)
        self.ahead = int(ahead)
        self.op = int(op)
        self._like(x, x.nch, F64)

    def rebuild(self, f):
        return MovingSumSignal(f(self.signal), self.back, self.ahead, self.op)

    def fields(self):
        return dict(l0=self.back, l1=self.ahead, i0=self.op)


class MovingRankSignal(StageSignal):
    """`MovingMedian(x, w)` / `MovingQuantile(x, w, q)`: per channel the sample of rank `floor(q (m - 1))` among the `m` samples
    of `x` over the frames `[n - back, n + ahead]`, clipped to the signal (no reference counterpart; include/sigops.h
    SO_NODE_MOVRANK, DESIGN.md "Moving ranks").  It has the length, frame rate, channels and sample type of `x`."""

    family = "MovingMedian / MovingQuantile"
    node = "MOVRANK"
    not_streamable = MovingSignal.not_streamable
    shard_order = 4  # (as Moving)
    shard_tail = _HALO
    demand = _need_x_ahead

    def stream_doubles(self):  # (as Moving)
        return 0

    def __init__(self, x, back, ahead, q):
        self.signal = x
        self.children = (x,)
        self.back = int(back)
        self.ahead = int(ahead)
        self.q = float(q)
        self._like(x, x.nch, x.dtype)

    def rebuild(self, f):
        return MovingRankSignal(f(self.signal), self.back, self.ahead, self.q)

    def fields(self):
        return dict(l0=self.back, l1=self.ahead, d0=self.q)


class RecurSignal(StageSignal):
    """`Recur(a, b)` / `OnePole` / `Smooth` / `PeakDecay`: per channel the first-order scan `y[n] = J(a[n], y[n-1], b[n])`,
    `y[0] = b[0]`, over one fixed tree (no reference counterpart; include/sigops.h SO_NODE_RECUR, DESIGN.md "Recur").
    `op` 0: `J = a y + b`; `op` 1: `J = max(a y, b)`.  The coefficient is the number `a` (then `coef` is None) or the signal
    `coef` of one channel or of `b`'s.  It has the length, frame rate and channels of `b` and is Float64."""

    family = "Recur / OnePole / Smooth / PeakDecay"
    node = "RECUR"
    not_streamable = ("would have to carry its last value (and its place in the tree of the scan) from one push to the next, "
                      "and that is not built")
    shard_order = 1  # (as Comb)
    demand = _need_every_child

    def stream_doubles(self):  # the carry C that enters a chunk
        return 1

    stream_checkpoint = _scan_checkpoint

    def __init__(self, a, b, op):
        self.signal = b
        if isinstance(a, AbstractSignal):
            self.coef, self.a = a, None
            self.children = (a, b)
        else:
            self.coef, self.a = None, float(a)
            self.children = (b,)
        self.op = int(op)
        self._like(b, b.nch, F64)

    def rebuild(self, f):  # the recurrence runs over frames, whatever rate they have
        return RecurSignal(self.a if self.coef is None else f(self.coef), f(self.signal), self.op)

    def fields(self):  # one child: b, the constant a in d0; two children: (a, b)
        return dict(i0=self.op, d0=0.0 if self.a is None else self.a)


class Recur2Signal(StageSignal):
    """`Recur2(a1, a2, b)` / `Resonator` / `Sweep`: per channel the second-order scan
    `y[n] = (a1[n] y[n-1] + a2[n] y[n-2]) + b[n]`, `y[0] = b[0]`, over one fixed tree (no reference counterpart;
    include/sigops.h SO_NODE_RECUR2, DESIGN.md "Recur2").  The coefficients are the numbers `a1`, `a2` (then `coefs` is None)
    or the two signals `coefs`, each of one channel or of `b`'s.  It has the length, frame rate and channels of `b` and is
    Float64."""

    family = "Recur2 / Resonator / Sweep"
    node = "RECUR2"
    not_streamable = ("would have to carry its last two values (and its place in the tree of the scan) from one push to the "
                      "next, and that is not built")
    shard_order = 1  # (as Comb)
    demand = _need_every_child

    def stream_doubles(self):  # the state (s0, s1) that enters a chunk
        return 2

    stream_checkpoint = _scan_checkpoint

    def __init__(self, a1, a2, b):
        self.signal = b
        if isinstance(a1, AbstractSignal):
            self.coefs, self.a1, self.a2 = (a1, a2), None, None
            self.children = (a1, a2, b)
        else:
            self.coefs, self.a1, self.a2 = None, float(a1), float(a2)
            self.children = (b,)
        self._like(b, b.nch, F64)

    def rebuild(self, f):
        if self.coefs is None:
            return Recur2Signal(self.a1, self.a2, f(self.signal))
        return Recur2Signal(f(self.coefs[0]), f(self.coefs[1]), f(self.signal))

    def fields(self):  # one child: b, the constants a1 in d0 and a2 in d1; three children: (a1, a2, b)
        return dict(d0=self.a1 if self.coefs is None else 0.0, d1=self.a2 if self.coefs is None else 0.0)


# map functions (src/mapsignal.jl:308,333,360,389; src/reformatting.jl:148-184)
ADD, MUL, SUB, DIV = "add", "mul", "sub", "div"
TUPLECAT, GETCHAN, AS1CHANNEL, ASNCHANNELS, TOELTYPE, REVERSECH = (
    "tuplecat", "getchan", "as1channel", "asnchannels", "toeltype", "reversech")


def _map_code(fn):
    table = {operator.add: ADD, operator.mul: MUL, operator.sub: SUB,
             operator.truediv: DIV, operator.neg: SUB, "+": ADD, "*": MUL, "-": SUB,
             "/": DIV, reversed: REVERSECH, "reverse": REVERSECH}
    if isinstance(fn, tuple):
        return fn
    if isinstance(fn, str) and fn in (ADD, MUL, SUB, DIV, TUPLECAT, AS1CHANNEL, REVERSECH):
        return fn
    if isinstance(fn, (OpaqueFn, ExprFn)):
        return fn
    if isinstance(fn, Elementwise):
        # a closure marked pure and elementwise: traced into a device program (trace.py; include/sigops.h SO_MAP_EXPR)
        return ExprFn(fn)
    try:
        if fn in table:
            return table[fn]
    except TypeError:
        pass
    if callable(fn):
        # an arbitrary closure (reference src/mapsignal.jl:131-145): the map is evaluated on the host at
        # sink time -- its operands by the engine, the closure by NumPy -- and enters the tree as an
        # array leaf (lowering.py)
        return OpaqueFn(fn)
    error(f"OperateOn: {fn!r} is not a function")


class OpaqueFn:
    """a host callable used as a map function"""

    def __init__(self, fn):
        self.fn = fn

    def __repr__(self):
        return f"OpaqueFn({self.fn!r})"


class ExprFn:
    """an `elementwise` closure used as a map function (traced, never called per sample)"""

    def __init__(self, fn):
        self.fn = fn  # the Elementwise marker (callable)

    def __repr__(self):
        return f"ExprFn({self.fn!r})"


def default_pad(fn):  # src/mapsignal.jl:274-276
    if isinstance(fn, (OpaqueFn, ExprFn)):
        return zero
    return one if fn in (MUL, DIV) else zero


class MapSignal(AbstractSignal):
    """reference src/mapsignal.jl:8-30"""

    def __init__(self, fn, signals, fs, padding, bychannel, extra=0, blocksize=4096):
        self.fn = fn
        self.extra = extra
        self.signals = tuple(signals)
        self.children = self.signals
        self.fs = fs
        self.padding = padding
        self.bychannel = bychannel
        self.blocksize = blocksize
        # test-value type inference, src/mapsignal.jl:139-143,190
        dts = [c.dtype for c in self.signals]
        t = dts[0]
        for d in dts[1:]:
            t = promote_type(t, d)
        if isinstance(fn, (OpaqueFn, ExprFn)):
            # test-value type inference (src/mapsignal.jl:139-143): the closure applied to ones
            try:
                if bychannel:
                    v = fn.fn(*[np.ones((), dtype=c.dtype)[()] for c in self.signals])
                else:
                    v = fn.fn(*[tuple(np.ones(c.nch, dtype=c.dtype)) for c in self.signals])
                    v = np.asarray(v).reshape(-1)
                    self._opaque_nch = int(v.size)
                t = np.asarray(v).dtype
                t = F32 if t == F32 else (I64 if np.issubdtype(t, np.integer) else F64)
            except Exception as e:  # noqa: BLE001
                error(f"OperateOn: could not apply {fn.fn!r} to test values: {e}")
            self.dtype = t
            self.nch = self.signals[0].nch if bychannel else self._opaque_nch
            if isinstance(fn, ExprFn):  # the device program(s): one, or one per output channel (bychannel=false)
                self.programs, odt = fn.fn.program([c.dtype for c in self.signals], bychannel,
                                                   [c.nch for c in self.signals])
                tdt = F32 if odt == F32 else F64
                if tdt != t or len(self.programs) != (1 if bychannel else self.nch):
                    error(f"OperateOn: the traced program of {fn.fn!r} yields {len(self.programs)} x {tdt}, its test "
                          f"values {self.nch} x {t}")
            return
        if fn == DIV and t == I64:
            t = F64
        if fn == TOELTYPE:
            t = np.dtype(extra)
        self.dtype = t
        if bychannel:
            self.nch = self.signals[0].nch
        elif fn == TUPLECAT:
            self.nch = sum(c.nch for c in self.signals)
        elif fn in (GETCHAN, AS1CHANNEL):
            self.nch = 1
        elif fn == ASNCHANNELS:
            self.nch = int(extra)
        else:
            self.nch = self.signals[0].nch

    def nframes_helper(self):  # src/mapsignal.jl:147-154
        def tolen(x):
            if isinstance(x, Extended):
                return x.len
            if x is numextend:
                return 0
            return x

        lens = [c.nframes_helper() for c in self.signals]
        acc = lens[0]
        for y in lens[1:]:
            if acc is numextend and y is numextend:
                continue
            a, b = tolen(acc), tolen(y)
            if a is None or b is None:
                acc = None
            elif a is inflen or b is inflen:
                acc = inflen
            else:
                acc = max(a, b)
        return acc

    def duration(self):
        n = nframes(self)
        if n is None or self.fs is None:
            return None
        return inflen if isknowninf(n) else n / self.fs


# pad markers (src/padding.jl:110-148)
def zero(x=None):
    return 0


def one(x=None):
    return 1


def lastframe(x):
    error("Must be passed as argument to `Pad`.")


def cycle(x, i, j):
    return x[(i - 1) % x.shape[0], j]


def mirror(x, i, j):
    n = x.shape[0]
    count, rem = divmod(i - 1, n)
    return x[rem if count % 2 == 0 else n - rem - 1, j]


def sinramp(x):  # src/ramps.jl:4
    return math.sin(math.pi * 0.5 * x)


# --------------------------------------------------------------------------
# Signal() coercion: reference src/signal.jl:96-149, src/arrays.jl:35-46,
# src/numbers.jl:47-49, src/functions.jl:88-96,109-110
def _assignal(x):
    if isinstance(x, AbstractSignal):
        return x
    return Signal(x)


def _isconsistent(fs, _fs):
    return fs is None or U.inHz(_fs) == U.inHz(fs)


def Signal(x=None, fs=None, *, ω=None, frequency=None, ϕ=0, phase=None, omega=None,
           phi=None, rng=None):
    # Signal(fs::Quantity) / Signal(;kwds...) curried forms, src/signal.jl:98-99
    if isinstance(x, Quantity) and x.unit in ("Hz", "kHz") and fs is None:
        rate = x
        return Curried(lambda y: Signal(y, rate))
    if x is None:
        kw = dict(ω=ω, frequency=frequency, ϕ=ϕ, phase=phase, omega=omega, phi=phi, rng=rng)
        return Curried(lambda y: Signal(y, fs, **kw))
    fs = U.inHz(fs)
    if omega is not None:
        ω = omega
    if phi is not None:
        ϕ = phi
    if isinstance(x, AbstractSignal):  # src/signal.jl:139-147
        if x.fs is None:
            return ToFramerate(x, fs)
        if not _isconsistent(fs, x.fs):
            error(f"Signal expected to have frame rate of {fs} Hz.")
        return x
    from .arraytypes import _Container

    if isinstance(x, _Container):  # src/SampledSignals.jl:3-9, src/AxisArrays.jl:30-36, src/DimensionalData.jl:6-14
        if not _isconsistent(fs, x.framerate):
            error(f"Signal expected to have frame rate of {fs} Hz.")
        a = ArraySig(x.signal_view(), x.framerate)
        a.container = type(x)
        return a
    if isinstance(x, tuple) and len(x) == 2 and not callable(x[0]):
        if not _isconsistent(fs, x[1]):
            error(f"Signal expected to have frame rate of {fs} Hz.")
        return ArraySig(x[0], U.inHz(x[1]))
    if isinstance(x, Quantity):
        if x.unit == "dB":  # src/numbers.jl:48-49
            return NumberSig(U.gain_ratio(x), fs, dB=True,
                             dtype=F32 if isinstance(x.value, np.floating) and x.value.dtype == F32 else F64)
        error(f"Don't know how create a signal from {x}.")
    if isinstance(x, (bool, int, float, np.integer, np.floating)):
        return NumberSig(x, fs)
    if isinstance(x, (list, range)) or isinstance(x, np.ndarray) or _is_torch(x):
        return ArraySig(x, fs)
    if callable(x) or (isinstance(x, str) and x in (SIN, COS, IDENTITY, RANDN)):
        code = None if isinstance(x, Elementwise) else _fn_code(x)
        pyfn = None
        if isinstance(x, Elementwise):
            # traced into a device program over the time argument (include/sigops.h SO_MAP_EXPR over a FUNC identity)
            x.program([F64])  # (traced here: what cannot be traced fails at construction, not at sink time)
            code, pyfn = EXPR, x
        elif code is None:
            # what the engine cannot lower is materialised on the host and passed
            # as an array leaf (here: the closure is evaluated with NumPy at sink time, lowering.py)
            code, pyfn = OPAQUE, x
        if code == RANDN:  # src/functions.jl:109-110
            return FuncSig(RANDN, fs, None, 0.0, rng=rng)
        if frequency is not None and ω is None:
            pass  # keyword `frequency` is accepted but ignored (src/functions.jl:90,92)
        w = U.inHz(ω)
        ph = phase if phase is not None else ϕ
        if w is None:
            if isinstance(ph, Quantity) and ph.unit not in ("s", "ms"):
                error("phase in radians needs a frequency (reference src/functions.jl:93)")
            p = U.inseconds(ph) if isinstance(ph, Quantity) else float(ph)
        else:
            p = U.inradians(ph, w) / (2 * math.pi)
        return FuncSig(code, fs, w, p, pyfn=pyfn)
    error(f"Don't know how create a signal from {x!r}.")


# --------------------------------------------------------------------------
# cutting: src/cutting.jl:46-57,77-78,105-106
def _curry2(ctor):
    def f(*args, **kw):
        if len(args) == 1:
            a = args[0]
            return Curried(lambda x: ctor(x, a, **kw))
        return ctor(*args, **kw)

    f.__name__ = ctor.__name__
    return f


def _Until(x, time):
    return CutApply(_assignal(x), time, "until")


def _After(x, time):
    return CutApply(_assignal(x), time, "after")


Until = _curry2(_Until)
After = _curry2(_After)


def Window(x=None, *, at=None, width=None, from_=None, to=None):
    if x is None:
        return Curried(lambda y: Window(y, at=at, width=width, from_=from_, to=to))
    if (at is None) != (width is None) or (from_ is None) != (to is None) or \
            (at is None) == (from_ is None):
        error("`Window` must either use the two keywords `at` and `width` OR"
              "the two keywords `from` and `to`.")
    # the reference's `at/width` form is broken by tuple precedence (SURVEY C-10)
    if from_ is None:
        error("Window(at=,width=) is broken in the reference (src/cutting.jl:55)")
    return _Until(_After(x, from_), to - from_)


# padding: src/padding.jl:76-101
def _Pad(x, p):
    x = _assignal(x)
    return x if isknowninf(nframes(x)) else PaddedSignal(x, p)


def _Extend(x, p):
    x = _assignal(x)
    return x if isknowninf(nframes(x)) else PaddedSignal(x, p, True)


Pad = _curry2(_Pad)
Extend = _curry2(_Extend)


# --------------------------------------------------------------------------
# reformatting: src/reformatting.jl
default_blocksize = 2 ** 12


def _maybe_rationalize(r):  # src/reformatting.jl:103-111
    for num, den in ((1, 1), (2, 1), (3, 1), (1, 2), (1, 3), (3, 2), (2, 3)):
        v = num / den
        if abs(v - r) <= np.spacing(r):
            return (num, den)
    return float(r)


def _resample(x, fs, blocksize):  # __ToFramerate__ :113-122
    ratio = _maybe_rationalize(fs / x.fs)
    if ratio == (1, 1):
        return x
    return FilteredSignal(x, ResamplerFn(ratio, fs), blocksize, fs)


def _stretchtime(t, scale):  # src/cutting.jl:140-141
    if U.is_frames(t) and scale is not None:
        return Quantity(int(math.floor(t.value * scale)), "frames")
    return t


def ToFramerate(x, fs=None, blocksize=default_blocksize):
    if fs is None and not isinstance(x, (AbstractSignal, np.ndarray, tuple, list)) and not _is_torch(x):
        rate = x  # curried form ToFramerate(fs)
        return Curried(lambda y: ToFramerate(y, rate, blocksize))
    x = _assignal(x)
    fs = U.inHz(fs)
    if fs is None:  # :67,85-86
        return x
    if x.fs is not None and fs == x.fs:
        return x
    known = x.fs is not None
    bs = blocksize
    if isinstance(x, ArraySig):  # src/arrays.jl:47-50
        return _resample(x, fs, bs) if known else ArraySig(x.data, fs)
    if isinstance(x, FuncSig):  # src/functions.jl:62-63
        return FuncSig(x.fn, fs, x.omega, x.phi, rng=x.rng, pyfn=x.pyfn)
    if isinstance(x, NumberSig):  # src/numbers.jl:56-57
        return NumberSig(x.val, fs, dB=x.dB, dtype=x.dtype)
    if isinstance(x, MapSignal):  # src/mapsignal.jl:46-64
        if known and not fs < x.fs:
            return _resample(x, fs, bs)
        kids = [ToFramerate(c, fs, bs) for c in x.signals]
        return _OperateOn(x.fn, kids, padding=x.padding, bychannel=x.bychannel, extra=x.extra)
    if isinstance(x, FilteredSignal):  # src/filters.jl:143-157
        if known and x.fs != x.signal.fs:
            return _resample(x.signal, fs, bs)
        return FilteredSignal(ToFramerate(x.signal, fs, bs), x.fn, x.blocksize, fs)
    if isinstance(x, StageSignal):
        # a result that has a rate is resampled like any computed signal; a missing rate goes to the children that take one
        if known:
            return _resample(x, fs, bs)
        return x.rebuild(lambda c: ToFramerate(c, fs, bs))
    computed = x.evaltrait == "computed"
    if known and not computed:  # generic DataSignal method :88-90
        return _resample(x, fs, bs)
    if isinstance(x, CutApply):  # src/cutting.jl:142-152
        scale = fs / x.fs if known else None
        return CutApply(ToFramerate(x.signal, fs, bs), _stretchtime(x.time, scale), x.kind)
    if isinstance(x, PaddedSignal):  # src/padding.jl:16-19
        return PaddedSignal(ToFramerate(x.signal, fs, bs), x.pad)
    if isinstance(x, AppendSignals):  # src/appending.jl:77-80
        return _Append([ToFramerate(c, fs, bs) for c in x.signals])
    if isinstance(x, RampSignal):  # src/ramps.jl:28-43
        return RampSignal(x.direction, ToFramerate(x.signal, fs, bs), x.time, x.fn)
    if isinstance(x, NormedSignal):  # src/filters.jl:276-285
        return NormedSignal(ToFramerate(x.signal, fs, bs))
    error(f"Value is not a signal: {x!r}")


def ToChannels(x, ch=None):  # src/reformatting.jl:132-170
    if ch is None:
        n = x
        return Curried(lambda y: ToChannels(y, n))
    x = _assignal(x)
    if ch == x.nch:
        return x
    if ch == 1:
        return _OperateOn(AS1CHANNEL, [x], bychannel=False)
    if x.nch == 1:
        return _OperateOn(ASNCHANNELS, [x], bychannel=False, extra=ch)
    error(f"No rule to convert signal with {x.nch} channels to a signal with {ch} channels.")


def ToEltype(x, T=None):  # src/reformatting.jl:183-184
    if T is None:
        t = x
        return Curried(lambda y: ToEltype(y, t))
    return _OperateOn(TOELTYPE, [_assignal(x)], extra=np.dtype(T))


def Format(x, fs, ch=None):  # src/reformatting.jl:207-213
    x = _assignal(x)
    if ch is None:
        ch = x.nch
    if ch > 1 and x.nch == 1:
        return ToChannels(ToFramerate(x, fs), ch)
    return ToFramerate(ToChannels(x, ch), fs)


def Uniform(xs, channels=False):  # src/reformatting.jl:241-254
    xs = [_assignal(x) for x in xs]
    rates = [x.fs for x in xs if x.fs is not None]
    fs = max(rates) if rates else None
    if not channels:
        return [Format(x, fs) for x in xs]
    ch = max(x.nch for x in xs)
    return [Format(x, fs, ch) for x in xs]


# --------------------------------------------------------------------------
# mapping: src/mapsignal.jl:131-145
def _OperateOn(fn, xs, padding=None, bychannel=True, extra=0, blocksize=default_blocksize):
    if padding is None:
        padding = default_pad(fn)
    xs = Uniform(xs, channels=bychannel)
    return MapSignal(fn, xs, xs[0].fs, padding, bychannel, extra, blocksize)


def OperateOn(fn, *xs, padding=None, bychannel=True):
    code = _map_code(fn)
    if code == REVERSECH:
        bychannel = False
    if fn is operator.neg and len(xs) != 1:
        error("negation takes one signal")
    return _OperateOn(code, list(xs), padding=padding, bychannel=bychannel)


def Operate(fn, *xs, **kw):
    return Curried(lambda x: OperateOn(fn, x, *xs, **kw))


def _nary(code):
    def f(*xs):
        if len(xs) == 1:
            y = xs[0]
            return Curried(lambda x: _OperateOn(code, [x, y]))
        return _OperateOn(code, list(xs))

    return f


Mix = _nary(ADD)  # src/mapsignal.jl:307-308
Amplify = _nary(MUL)  # src/mapsignal.jl:332-333


def AddChannel(*xs):  # src/mapsignal.jl:359-360
    if len(xs) == 1:
        y = xs[0]
        return Curried(lambda x: _OperateOn(TUPLECAT, [x, y], bychannel=False))
    return _OperateOn(TUPLECAT, list(xs), bychannel=False)


def SelectChannel(x, n=None):  # src/mapsignal.jl:388-391
    if n is None:
        k = x
        return Curried(lambda y: SelectChannel(y, k))
    x = _assignal(x)
    return _OperateOn(GETCHAN, [x], bychannel=False, extra=int(n))


# --------------------------------------------------------------------------
# SampleAt / Delay: a signal read at computed positions (no reference counterpart)
def _real_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


SAMPLEAT_INTERP = ("linear", "cubic", "sinc")  # the node's i1
SAMPLEAT_PHASES = 512


def sampleat_beta(taps):
    """the Kaiser window's shape for `taps` taps (DESIGN.md "SampleAt"): 96 dB of stop-band attenuation from 16 taps on,
    5.0 (about 54 dB) for the short kernels, whose main lobe would otherwise swallow the pass band"""
    return 0.1102 * (96 - 8.7) if taps >= 16 else 5.0


def sampleat_taps(taps, cutoff):
    """the tap tables of `SampleAt(..., interp="sinc")`: `h`, 513 rows (phase 0 .. 512 of 512) of `taps` Float64, and
    `dh[ph] = h[ph + 1] - h[ph]`, 512 rows.  Row ph, tap k lies d = ph/512 - (k - taps/2 + 1) frames from the position:
    h = cutoff sinc(cutoff d) kaiser(d / (taps/2)), each row divided by its sum; with cutoff == 1 rows 0 and 512 are the
    exact unit impulses.  (tests/sampleat_interp_ref.py restates this; the device receives the bytes.)"""
    K, P = int(taps), SAMPLEAT_PHASES
    c = np.float64(cutoff)
    d = np.arange(P + 1, dtype=np.float64)[:, None] / np.float64(P) - (np.arange(K, dtype=np.float64)[None, :] - np.float64(K // 2 - 1))
    w = d / np.float64(K // 2)
    beta = np.float64(sampleat_beta(K))
    h = c * np.sinc(c * d) * (np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - w * w))) / np.i0(beta))
    h = h / h.sum(axis=1)[:, None]
    if c == 1.0:
        h[0] = 0.0
        h[0, K // 2 - 1] = 1.0
        h[P] = 0.0
        h[P, K // 2] = 1.0
    return np.ascontiguousarray(h), np.ascontiguousarray(h[1:] - h[:-1])


def _sampleat_kind(what, interp, taps, cutoff):
    """(interp, taps, cutoff) checked: `taps` and `cutoff` belong to "sinc" alone (None: not given)"""
    if interp not in SAMPLEAT_INTERP:
        error(f'{what}: interp must be "linear", "cubic" or "sinc", not {interp!r}')
    if interp != "sinc":
        for name, v in (("taps", taps), ("cutoff", cutoff)):
            if v is not None:
                error(f'{what}: {name} is an argument of interp="sinc" only (interp={interp!r} given)')
        return interp, 0, 0.0
    taps = 16 if taps is None else taps
    cutoff = 1.0 if cutoff is None else cutoff
    if isinstance(taps, (bool, np.bool_)) or not isinstance(taps, (int, np.integer)) or taps < 4 or taps > 64 or taps % 2:
        error(f"{what}: taps must be an even integer from 4 to 64, not {taps!r}")
    if not _real_number(cutoff) or not (0.0 < cutoff <= 1.0):
        error(f"{what}: cutoff must be a number in (0, 1], a fraction of the table's Nyquist, not {cutoff!r}")
    return interp, int(taps), float(cutoff)


def _SampleAt(x, pos, left=0.0, right=0.0, relative=False, wrap=False, interp="linear", taps=None, cutoff=None, what="SampleAt"):
    interp, taps, cutoff = _sampleat_kind(what, interp, taps, cutoff)
    x = _assignal(x)
    n = nframes(x)
    if n is None or isknowninf(n):
        error("SampleAt: the table x must have a known, finite length (use `Until`)")
    if n < 1:
        error("SampleAt: the table x must have at least one frame")
    if x.dtype not in (F32, F64):
        error("SampleAt: the table x must be Float32 or Float64 (use `ToEltype`)")
    for name, v in (("left", left), ("right", right)):
        if not _real_number(v):
            error(f"SampleAt: {name} must be a number, not {v!r}")
    if _real_number(pos):
        pos = NumberSig(float(pos))
    pos = _assignal(pos)
    if pos.dtype not in (F32, F64):
        error("SampleAt: the positions must be Float32 or Float64 (use `ToEltype`)")
    if pos.nch not in (1, x.nch):
        error(f"SampleAt: the positions have {pos.nch} channels; 1 or the table's {x.nch} expected")
    return SampleAtSignal(x, pos, left, right, relative, wrap, interp, taps, cutoff)


_NOT_GIVEN = object()


def SampleAt(*args, left=0.0, right=0.0, relative=False, wrap=False, interp="linear", taps=_NOT_GIVEN, cutoff=_NOT_GIVEN):
    """`SampleAt(x, pos)`, curried `x | SampleAt(pos)`: frame n, channel c of the result is
    `np.interp(p, arange(N), x[:, c], left, right)` -- `np.interp(p, arange(N), x[:, c], period=N)` with `wrap` -- at
    `p = pos[n, c]` (`n + pos[n, c]` with `relative`): positions count the frames of `x` from 0.  `interp="cubic"` reads
    through a Catmull-Rom polynomial, `interp="sinc"` through `taps` (16; even, 4 .. 64) taps of a Kaiser-windowed sinc
    whose pass band ends at `cutoff` (1.0; in (0, 1]) of the table's Nyquist -- `1 / v` for a read at speed v > 1."""
    kw = dict(left=left, right=right, relative=relative, wrap=wrap, interp=interp,
              taps=None if taps is _NOT_GIVEN else taps, cutoff=None if cutoff is _NOT_GIVEN else cutoff)
    if len(args) == 1:
        pos = args[0]
        return Curried(lambda x: _SampleAt(x, pos, **kw))
    if len(args) != 2:
        error("SampleAt(x, pos) expected")
    return _SampleAt(args[0], args[1], **kw)


def _Delay(x, d, interp="linear", taps=None, cutoff=None):
    from .units import frames

    _sampleat_kind("Delay", interp, taps, cutoff)

    x = _assignal(x)
    n = nframes(x)
    if n is None or isknowninf(n):
        error("Delay: SampleAt needs a signal x of known, finite length (use `Until`)")
    if isinstance(d, Quantity):
        if U.is_time(d):
            if x.fs is None:
                error("Delay: a delay given as a time needs the frame rate of x")
            d = U.inseconds_raw(d) * x.fs
        elif U.is_frames(d):
            d = d.value
        else:
            error(f"Delay: {d} is neither a time nor a number of frames")
    if _real_number(d):
        pos = NumberSig(-float(d), x.fs)
    else:
        d = _assignal(d)
        if x.fs is not None:
            d = ToFramerate(d, x.fs)
        pos = _OperateOn(SUB, [d])
    y = _SampleAt(x, pos, relative=True, interp=interp, taps=taps, cutoff=cutoff, what="Delay")
    return _Until(_Pad(y, zero), n * frames)


def Delay(*args, interp="linear", taps=_NOT_GIVEN, cutoff=_NOT_GIVEN):
    """`Delay(x, d)`, curried `x | Delay(d)`: `x` delayed by `d` frames (a number or a signal; a time quantity is
    converted with the rate of `x`), zeros before its first frame: `SampleAt(x, -d, relative=True)` over the frames of `x`,
    with `SampleAt`'s `interp`, `taps` and `cutoff`."""
    kw = dict(interp=interp, taps=None if taps is _NOT_GIVEN else taps, cutoff=None if cutoff is _NOT_GIVEN else cutoff)
    if len(args) == 1:
        d = args[0]
        return Curried(lambda x: _Delay(x, d, **kw))
    if len(args) != 2:
        error("Delay(x, d) expected")
    return _Delay(args[0], args[1], **kw)


# --------------------------------------------------------------------------
# Comb / Allpass: feedback delay lines (no reference counterpart)
def _comb_delay(what, x, d):
    """the delay in frames: a number of frames, a `frames` quantity, or a time converted with the rate of x"""
    if isinstance(d, Quantity):
        if U.is_time(d):
            if x.fs is None:
                error(f"{what}: a delay given as a time needs the frame rate of x")
            return U.inframes_int(d, x.fs)
        if not U.is_frames(d):
            error(f"{what}: the delay {d} is neither a time nor a number of frames")
        d = d.value
    if not _real_number(d) or not math.isfinite(d) or d != math.floor(d):
        error(f"{what}: the delay must be a whole number of frames, not {d!r} (`Delay` interpolates; a delay line does not)")
    return int(d)


def _Comb(what, x, d, b0, bD, a):
    """`what` names the construct in a refusal: "Comb", or "Allpass (Comb)" for the wrapper"""
    x = _assignal(x)
    n = nframes(x)
    if n is None or isknowninf(n):
        error(f"{what}: the signal x must have a known, finite length (use `Until`): the recurrence starts at frame 0")
    if x.dtype not in (F32, F64):
        error(f"{what}: the signal x must be Float32 or Float64 (use `ToEltype`)")
    for name, v in (("g", a), ("feedforward", bD), ("direct", b0)):
        if not _real_number(v) or not math.isfinite(v):
            error(f"{what}: {name} must be a finite number, not {v!r}")
    D = _comb_delay(what, x, d)
    if D < 1:
        error(f"{what}: the delay must be at least one frame ({D} given)")
    return CombSignal(x, D, b0, bD, a)


def Comb(*args, feedforward=0.0, direct=1.0):
    """`Comb(x, d, g)`, curried `x | Comb(d, g)`: a comb filter, `y[n] = (direct x[n] + feedforward x[n - D]) + g y[n - D]`
    per channel, frames before the first taken as +0.0, every product and sum rounded on its own in Float64 and a term
    whose coefficient is exactly 0 left out.  The default is the feedback comb `y[n] = x[n] + g y[n - D]`, an echo with
    repeats.  `d` is a whole number of frames (a number or a `frames` quantity) or a time, converted with the rate of `x`.
    The result has the length of `x`; an echo's tail is the caller's to ask for: `x | Pad(zero) | Until(t) | Comb(d, g)`.
    `x` must have a known, finite length.  `stream` over the node works, but the recurrence starts at frame 0, so
    every block recomputes the frames before it (quadratic in the length, as `stream` over `Normpower` re-reads its
    input).  Blocks and windows agree with the whole sink bit for bit where `x` gives the same bits whatever number of
    frames is asked of it (arrays, formulas, maps, `SampleAt`, nested `Comb`s); a `Filt` below the node rounds by how it
    chunks its input, and the comb carries that: agreement within the Float64 contract.  A `BlockStream` carries the delay line from push to push and gives the whole sink's bits; multi-GPU
    shards refuse the node."""
    if len(args) == 2:
        d, g = args
        return Curried(lambda x: _Comb("Comb", x, d, direct, feedforward, g))
    if len(args) != 3:
        error("Comb(x, d, g) expected")
    return _Comb("Comb", args[0], args[1], direct, feedforward, args[2])


def Allpass(*args):
    """`Allpass(x, d, g)`, curried `x | Allpass(d, g)`: Schroeder's allpass, `y[n] = (-g x[n] + x[n - D]) + g y[n - D]`:
    `Comb(x, d, g, feedforward=1, direct=-g)`."""
    if len(args) == 2:
        d, g = args
        return Curried(lambda x: _Comb("Allpass (Comb)", x, d, -g if _real_number(g) else g, 1.0, g))
    if len(args) != 3:
        error("Allpass(x, d, g) expected: Comb with direct = -g, feedforward = 1")
    g = args[2]
    return _Comb("Allpass (Comb)", args[0], args[1], -g if _real_number(g) else g, 1.0, g)


# --------------------------------------------------------------------------
# Cumsum / Integrate: running sums (no reference counterpart)
def _Cumsum(x, what="Cumsum"):
    """`what` names the construct in a refusal: "Cumsum", or "Integrate (Cumsum)" for the wrapper"""
    x = _assignal(x)
    n = nframes(x)
    if n is None or isknowninf(n):
        error(f"{what}: the signal x must have a known, finite length (use `Until`): the sum starts at frame 0")
    if x.dtype not in (F32, F64):
        error(f"{what}: the signal x must be Float32 or Float64 (use `ToEltype`)")
    return CumsumSignal(x)


Cumsum = Curried(_Cumsum)
Cumsum.__doc__ = """`Cumsum(x)`, piped `x | Cumsum`: the running sum, frame n of a channel is `x[0] + ... + x[n]` in Float64 -- the phase
of an oscillator whose frequency `x` gives, brown noise from white.  A parallel sum rounds differently from a loop, so
the node fixes ONE summation tree that depends on the frame index only (runs of 16 frames left to right, a Kogge-Stone
scan over the 64 runs of a tile, sequential carries over the 16 tiles of a chunk and over the chunks; DESIGN.md
"Cumsum", tests/cumsum_ref.py): a window, a `stream` block and the whole sink give the same bits, and the error of
frame n stays within about (40 + chunks) * 2**-53 * sum(|x[:n + 1]|).  `x` must have a known, finite length.  `stream` over
the node recomputes the frames before every block (quadratic in the length, as over `Comb`): stream what follows the
node.  A `BlockStream` carries the running total that enters a chunk and gives the whole sink's bits; multi-GPU shards refuse the node."""


def _Integrate(x):
    x = _assignal(x)
    if x.fs is None:
        error("Integrate (Cumsum): the signal x needs a frame rate: the integral is the running sum times 1 / framerate (use `Cumsum`, or `ToFramerate`)")
    return _OperateOn(MUL, [_Cumsum(x, "Integrate (Cumsum)"), NumberSig(1.0 / x.fs)])


Integrate = Curried(_Integrate)
Integrate.__doc__ = """`Integrate(x)`, piped `x | Integrate`: the integral of `x` over time, `Cumsum(x)` times the Float64 constant
`1.0 / framerate(x)` (one more rounding a sample, through the map path)."""


# --------------------------------------------------------------------------
# Recur / OnePole / Smooth / PeakDecay: first-order scans (no reference counterpart)
def _Recur(what, op, a, b):
    """`what` names the construct in a refusal: "Recur", or "OnePole (Recur)" and so on for the wrappers"""
    b = _assignal(b)
    n = nframes(b)
    if n is None or isknowninf(n):
        error(f"{what}: the signal b must have a known, finite length (use `Until`): the recurrence starts at frame 0")
    if b.dtype not in (F32, F64):
        error(f"{what}: the signal b must be Float32 or Float64 (use `ToEltype`)")
    if _real_number(a):
        if not math.isfinite(a):
            error(f"{what}: the coefficient a must be a finite number or a signal, not {a!r}")
        return RecurSignal(float(a), b, op)
    if isinstance(a, (bool, np.bool_, Quantity, str)) or a is None:
        error(f"{what}: the coefficient a must be a number or a signal, not {a!r}")
    a = _assignal(a)
    if a.dtype not in (F32, F64):
        error(f"{what}: the coefficient signal a must be Float32 or Float64 (use `ToEltype`)")
    if a.nch not in (1, b.nch):
        error(f"{what}: the coefficient signal a has {a.nch} channels; 1 or b's {b.nch} expected")
    if a.fs is not None and b.fs is not None and a.fs != b.fs:
        error(f"{what}: the coefficient signal a has a frame rate of {a.fs} Hz and b one of {b.fs} Hz (use `ToFramerate`)")
    if a.fs is None and b.fs is not None:
        a = ToFramerate(a, b.fs)
    elif b.fs is None and a.fs is not None:
        b = ToFramerate(b, a.fs)
    na = nframes(a)
    if na is None or (not isknowninf(na) and na < n):
        error(f"{what}: the coefficient signal a ({'an unknown number of' if na is None else na} frames) must be infinite or at least as long as b ({n} frames)")
    return RecurSignal(a, b, op)


def Recur(*args):
    """`Recur(a, b)`, curried `b | Recur(a)`: the first-order linear recurrence `y[n] = a[n] y[n-1] + b[n]`, `y[0] = b[0]`
    per channel in Float64 -- a smoother whose time constant is a signal, a leaky integrator, a decay envelope with a
    controlled rate.  `a` is a real number, or a Float32 / Float64 signal of one channel (every channel of `b` reads it) or of
    `b`'s channel count, infinite or at least as long as `b`.  A parallel scan rounds differently from a loop, so the node
    fixes ONE tree that depends on the frame index only (Cumsum's: runs of 16 frames, a Kogge-Stone scan over the 64 runs of
    a tile, sequential carries over the tiles of a chunk and over the chunks, on pairs (product of a, value); DESIGN.md
    "Recur", tests/recur_ref.py), product and sum rounded on their own: a window, a `stream` block and the whole sink give
    the same bits, and `Recur(1.0, x)` equals `Cumsum(x)` bit for bit.  A term `b[k]` reaches frame n through at most
    `(n - k) + 2 (40 + chunks)` rounded operations, against the loop's `2 (n - k)`: the error is of the order of the loop's
    own, relative to `S[n] = |a[n]| S[n-1] + |b[n]|`.  The node is meant for `|a| <= 1`: where
    `|a| > 1` over hundreds of frames a product of the a can overflow and `Inf * 0` gives NaN where a loop would stay
    finite.  There is no initial state: `y[-1]` is absent, not 0.  `b` must have a known, finite length.  `stream` over the
    node recomputes the frames before every block (as over `Cumsum`); a `BlockStream` carries the scan's state from chunk to chunk and gives the whole sink's bits; multi-GPU shards refuse the node."""
    if len(args) == 1:
        a = args[0]
        return Curried(lambda b: _Recur("Recur", 0, a, b))
    if len(args) != 2:
        error("Recur(a, b) expected")
    return _Recur("Recur", 0, args[0], args[1])


def _rate_for(what, x, name):
    if x.fs is None:
        error(f"{what}: {name} needs the frame rate of x (use `ToFramerate`, or `Recur` with a coefficient per frame)")
    return float(x.fs)


def _coef_signal(what, name, x, v, fn):
    """the coefficient sub-tree of a wrapper: the signal `v` at the rate of x, through the traced map `fn`"""
    fs = _rate_for(what, x, f"{name} given as a signal")
    v = _assignal(v)
    if v.dtype not in (F32, F64):
        error(f"{what}: the signal {name} must be Float32 or Float64 (use `ToEltype`)")
    if v.fs is not None and v.fs != fs:
        error(f"{what}: the signal {name} has a frame rate of {v.fs} Hz and x one of {fs} Hz (use `ToFramerate`)")
    return _OperateOn(_map_code(Elementwise(fn)), [ToFramerate(v, fs)])


def _lowpass(what, x, a):
    """`y[n] = a y[n-1] + (1 - a) x[n]`: unit gain at DC.  A signal `a` scales x through a traced map, as Integrate builds its product"""
    from .units import frames

    if not isinstance(a, AbstractSignal):
        return _Recur(what, 0, a, _OperateOn(MUL, [x, NumberSig(1.0 - a)]))
    n = nframes(x)
    if n is None or isknowninf(n):
        error(f"{what}: the signal x must have a known, finite length (use `Until`): the recurrence starts at frame 0")
    b = _OperateOn(_map_code(Elementwise(lambda c, v: (1.0 - c) * v)), [a, x])
    return _Recur(what, 0, a, _Until(b, n * frames))


def _OnePole(x, fc):
    what = "OnePole (Recur)"
    x = _assignal(x)
    if x.dtype not in (F32, F64):
        error(f"{what}: the signal x must be Float32 or Float64 (use `ToEltype`)")
    if isinstance(fc, Quantity) or _real_number(fc):
        try:
            hz = U.inHz(fc)
        except ValueError:
            error(f"{what}: the cutoff {fc} is not a frequency")
        if not math.isfinite(hz) or hz < 0:
            error(f"{what}: the cutoff must be a finite frequency >= 0, not {fc!r}")
        return _lowpass(what, x, math.exp(-2.0 * math.pi * hz / _rate_for(what, x, "a cutoff in Hz")))
    k = -2.0 * math.pi / _rate_for(what, x, "a cutoff in Hz")
    return _lowpass(what, x, _coef_signal(what, "fc", x, fc, lambda f: np.exp(f * k)))


def OnePole(*args):
    """`OnePole(x, fc)`, curried `x | OnePole(fc)`: a one-pole low-pass with unit gain at DC,
    `y[n] = a y[n-1] + (1 - a) x[n]`, `a = exp(-2 pi fc / framerate)`: `Recur(a, (1 - a) x)`.  `fc` is a frequency (a number
    of Hz or a quantity; `math.exp` on the host) or a signal of Hz at the rate of `x` (`a` and `(1 - a) x` are then traced
    maps on the device), of one channel or of `x`'s."""
    if len(args) == 1:
        fc = args[0]
        return Curried(lambda x: _OnePole(x, fc))
    if len(args) != 2:
        error("OnePole(x, fc) expected")
    return _OnePole(args[0], args[1])


def _decay(what, name, x, t):
    """`exp(-1 / (t framerate))` from the time `t` (a number of seconds or a time quantity); a time of 0 gives 0"""
    if isinstance(t, Quantity) and not U.is_time(t):
        error(f"{what}: {name} {t} is not a time")
    sec = U.inseconds_raw(t) if isinstance(t, Quantity) else float(t)
    if not math.isfinite(sec) or sec < 0:
        error(f"{what}: {name} must be a finite time >= 0, not {t!r}")
    fs = _rate_for(what, x, f"{name} given as a time")
    return 0.0 if sec == 0 else math.exp(-1.0 / (sec * fs))


def _Smooth(x, tau):
    what = "Smooth (Recur)"
    x = _assignal(x)
    if x.dtype not in (F32, F64):
        error(f"{what}: the signal x must be Float32 or Float64 (use `ToEltype`)")
    if isinstance(tau, Quantity) or _real_number(tau):
        return _lowpass(what, x, _decay(what, "tau", x, tau))
    k = -1.0 / _rate_for(what, x, "tau")
    return _lowpass(what, x, _coef_signal(what, "tau", x, tau, lambda t: np.exp(k / t)))


def Smooth(*args):
    """`Smooth(x, tau)`, curried `x | Smooth(tau)`: `OnePole` by its time constant, `a = exp(-1 / (tau framerate))`: the step
    response reaches `1 - 1/e` after `tau`.  `tau` is a time (a number of seconds or a quantity) or a signal of seconds at
    the rate of `x`; `tau == 0` gives `a = 0`, `x` itself."""
    if len(args) == 1:
        tau = args[0]
        return Curried(lambda x: _Smooth(x, tau))
    if len(args) != 2:
        error("Smooth(x, tau) expected")
    return _Smooth(args[0], args[1])


def _PeakDecay(x, release, r):
    what = "PeakDecay (Recur)"
    x = _assignal(x)
    if (release is None) == (r is None):
        error(f"{what}: give the release time or `r=`, the factor a frame, one of them")
    if r is None:
        if not (isinstance(release, Quantity) or _real_number(release)):
            error(f"{what}: the release must be a time, not {release!r} (a factor per frame that is a signal goes to `r=`)")
        r = _decay(what, "the release", x, release)
    elif _real_number(r) and not 0.0 <= r <= 1.0:
        error(f"{what}: a constant r must lie in [0, 1], not {r!r}")
    return _Recur(what, 1, r, x)


def PeakDecay(*args, r=None):
    """`PeakDecay(x, release)`, curried `x | PeakDecay(release)`: the peak follower with instant attack and exponential
    release, `y[n] = max(x[n], r y[n-1])`, `y[0] = x[0]` -- the companion of `MovingMax` in a limiter's side-chain.
    `r = exp(-1 / (release framerate))` from the release time, or `r=` directly: a number in [0, 1] or a signal (`Recur`'s
    rules for `a`).  The product is rounded once; a NaN in `x` or `r` makes the frames after it NaN; over the same tree as
    `Recur`, so windows, `stream` blocks and the whole sink agree bit for bit."""
    if len(args) == 0 and r is not None:
        return Curried(lambda x: _PeakDecay(x, None, r))
    if len(args) == 1 and r is None:
        release = args[0]
        return Curried(lambda x: _PeakDecay(x, release, None))
    if len(args) == 1:
        return _PeakDecay(args[0], None, r)
    if len(args) != 2:
        error("PeakDecay(x, release) or PeakDecay(x, r=...) expected")
    return _PeakDecay(args[0], args[1], r)


# --------------------------------------------------------------------------
# Recur2 / Resonator / Sweep: second-order scans (no reference counterpart)
def _Recur2(what, a1, a2, b):
    """`what` names the construct in a refusal: "Recur2", or "Resonator (Recur2)" and "Sweep (Recur2)" for the wrappers"""
    b = _assignal(b)
    n = nframes(b)
    if n is None or isknowninf(n):
        error(f"{what}: the signal b must have a known, finite length (use `Until`): the recurrence starts at frame 0")
    if b.dtype not in (F32, F64):
        error(f"{what}: the signal b must be Float32 or Float64 (use `ToEltype`)")
    coefs = []
    for name, a in (("a1", a1), ("a2", a2)):
        if _real_number(a):
            if not math.isfinite(a):
                error(f"{what}: the coefficient {name} must be a finite number or a signal, not {a!r}")
            coefs.append(float(a))
            continue
        if isinstance(a, (bool, np.bool_, Quantity, str)) or a is None:
            error(f"{what}: the coefficient {name} must be a number or a signal, not {a!r}")
        a = _assignal(a)
        if a.dtype not in (F32, F64):
            error(f"{what}: the coefficient signal {name} must be Float32 or Float64 (use `ToEltype`)")
        if a.nch not in (1, b.nch):
            error(f"{what}: the coefficient signal {name} has {a.nch} channels; 1 or b's {b.nch} expected")
        coefs.append(a)
    if not any(isinstance(a, AbstractSignal) for a in coefs):
        return Recur2Signal(coefs[0], coefs[1], b)
    # one rate for the three: every known rate must be the same one, a missing one is taken from the others
    fs = b.fs
    for name, a in zip(("a1", "a2"), coefs):
        if isinstance(a, AbstractSignal) and a.fs is not None:
            if fs is not None and a.fs != fs:
                error(f"{what}: the coefficient signal {name} has a frame rate of {a.fs} Hz and {'b' if b.fs is not None else 'the other coefficient'} one of {fs} Hz (use `ToFramerate`)")
            fs = a.fs
    if fs is not None and b.fs is None:
        b = ToFramerate(b, fs)
    for k, name in enumerate(("a1", "a2")):
        a = coefs[k]
        if not isinstance(a, AbstractSignal):
            a = NumberSig(a, fs)  # a constant next to a signal: a row of it, written once by a pointwise step
        elif a.fs is None and fs is not None:
            a = ToFramerate(a, fs)
        na = nframes(a)
        if na is None or (not isknowninf(na) and na < n):
            error(f"{what}: the coefficient signal {name} ({'an unknown number of' if na is None else na} frames) must be infinite or at least as long as b ({n} frames)")
        coefs[k] = a
    return Recur2Signal(coefs[0], coefs[1], b)


def Recur2(*args):
    """`Recur2(a1, a2, b)`, curried `b | Recur2(a1, a2)`: the second-order linear recurrence
    `y[n] = (a1[n] y[n-1] + a2[n] y[n-2]) + b[n]`, `y[0] = b[0]`, `y[1] = (a1[1] y[0] + a2[1] 0) + b[1]` per channel in
    Float64 -- the recursive half of a filter whose cutoff or resonance moves over time.  Each coefficient is a finite real
    number, or a Float32 / Float64 signal of one channel (every channel of `b` reads it) or of `b`'s channel count, infinite
    or at least as long as `b`; a number next to a signal becomes a row of it.  A parallel scan rounds differently from a
    loop, so the node fixes ONE tree that depends on the frame index only (Cumsum's: runs of 16 frames, a Kogge-Stone scan
    over the 64 runs of a tile, sequential carries over the tiles of a chunk and over the chunks, on the affine maps
    `s -> M s + v` of the state `(y[n], y[n-1])`; DESIGN.md "Recur2", tests/recur2_ref.py), every product and sum rounded on
    its own: a window, a `stream` block and the whole sink give the same bits, and inside a run of 16 frames the outputs are
    the loop's own operations on the state that entered the run; the composites are joined in double-double arithmetic,
    which keeps poles close to `z = 1` or `z = -1` within 1e-8 of an extended-precision loop (DESIGN.md gives the figures).
    The node is meant for stable coefficients: unstable stretches overflow the composites, and an `Inf` that meets a zero
    of a composite gives NaN.  There is no initial state.  `b` must have a
    known, finite length.  `stream` over the node recomputes the frames before every block (as over `Cumsum`);
    a `BlockStream` carries the scan's state from chunk to chunk and gives the whole sink's bits; multi-GPU shards refuse the node."""
    if len(args) == 2:
        a1, a2 = args
        return Curried(lambda b: _Recur2("Recur2", a1, a2, b))
    if len(args) != 3:
        error("Recur2(a1, a2, b) expected")
    return _Recur2("Recur2", args[0], args[1], args[2])


def _hz_param(what, name, x, v, lowest=0.0, strict=False):
    """a parameter of a wrapper: a number (for a frequency a quantity too) checked and returned as a float, or a signal at
    the rate of x returned as a Float64 signal"""
    if isinstance(v, Quantity) or _real_number(v):
        if name == "q":
            if isinstance(v, Quantity):
                error(f"{what}: q is a plain number, not {v}")
            hz = float(v)
        else:
            try:
                hz = U.inHz(v)
            except ValueError:
                error(f"{what}: {name} = {v} is not a frequency")
        if not math.isfinite(hz) or hz < lowest or (strict and hz <= lowest):
            error(f"{what}: {name} must be a finite {'number' if name == 'q' else 'frequency'} {'>' if strict else '>='} {lowest:g}, not {v!r}")
        return hz
    if isinstance(v, (bool, np.bool_, str)) or v is None:
        error(f"{what}: {name} must be a number or a signal, not {v!r}")
    fs = _rate_for(what, x, f"{name} given as a signal")
    v = _assignal(v)
    if v.dtype not in (F32, F64):
        error(f"{what}: the signal {name} must be Float32 or Float64 (use `ToEltype`)")
    if v.nch not in (1, x.nch):
        error(f"{what}: the signal {name} has {v.nch} channels; 1 or x's {x.nch} expected")
    if v.fs is not None and v.fs != fs:
        error(f"{what}: the signal {name} has a frame rate of {v.fs} Hz and x one of {fs} Hz (use `ToFramerate`)")
    v = ToFramerate(v, fs)
    return v if v.dtype == F64 else ToEltype(v, F64)


def _formulas(what, x, params, fns, taps):
    """`Recur2` from formulas: `params` are numbers or signals; `fns(*params) -> (a1, a2, c0, ..)` gives the two coefficients
    and one gain per tap, `taps` being x and its delayed copies; b is the sum of the gains times the taps, left to right.
    All numbers: `fns` runs on the host with `math`.  A signal among them: one traced map per coefficient and one for b."""
    from .units import frames

    n = nframes(x)
    sig = [i for i, v in enumerate(params) if isinstance(v, AbstractSignal)]

    def mix(gains, ts):
        acc = gains[0] * ts[0]
        for g, t in zip(gains[1:], ts[1:]):
            acc = acc + g * t
        return acc

    if not sig:
        a1, a2, *gains = fns(math, *params)
        gains = [np.float64(g) for g in gains]  # (strong Float64: a Float32 x widens before it is multiplied)
        if len(taps) == 1:
            b = _OperateOn(MUL, [taps[0], NumberSig(gains[0])])
        else:
            b = _OperateOn(_map_code(Elementwise(lambda *ts: mix(gains, ts))), list(taps))
        return _Recur2(what, a1, a2, b)

    def full(args):
        vals = list(params)
        for k, i in enumerate(sig):
            vals[i] = args[k]
        return vals

    ps = [params[i] for i in sig]
    coef = [_OperateOn(_map_code(Elementwise(lambda *s, k=k: fns(np, *full(s))[k])), ps) for k in (0, 1)]
    b = _OperateOn(_map_code(Elementwise(lambda *s: mix(fns(np, *full(s[: len(sig)]))[2:], s[len(sig):]))), ps + list(taps))
    return _Recur2(what, coef[0], coef[1], _Until(b, n * frames))


def _wrapper_input(what, x):
    x = _assignal(x)
    if x.dtype not in (F32, F64):
        error(f"{what}: the signal x must be Float32 or Float64 (use `ToEltype`)")
    n = nframes(x)
    if n is None or isknowninf(n):
        error(f"{what}: the signal x must have a known, finite length (use `Until`): the recurrence starts at frame 0")
    return x


def _Resonator(x, fc, bw):
    what = "Resonator (Recur2)"
    x = _wrapper_input(what, x)
    fs = _rate_for(what, x, "a frequency in Hz")
    fc, bw = _hz_param(what, "fc", x, fc), _hz_param(what, "bw", x, bw)

    def fns(m, fc, bw):
        r = m.exp(-math.pi * bw / fs)
        th = 2.0 * math.pi * fc / fs
        return 2.0 * r * m.cos(th), -(r * r), (1.0 - r * r) * m.sin(th)

    return _formulas(what, x, [fc, bw], fns, [x])


def Resonator(*args):
    """`Resonator(x, fc, bw)`, curried `x | Resonator(fc, bw)`: the two-pole resonator at the centre frequency `fc` with the
    bandwidth `bw`: `Recur2(2 r cos(theta), -r^2, (1 - r^2) sin(theta) x)` with `r = exp(-pi bw / framerate)` and
    `theta = 2 pi fc / framerate`; its gain at `fc` is about one for narrow bandwidths.  `fc` and `bw` are each a frequency
    (a number of Hz or a quantity; `math` on the host) or a signal of Hz at the rate of `x`, of one channel or of `x`'s
    (the coefficients are then traced maps on the device): a resonator whose pitch follows `Cumsum`'s oscillator, a
    formant glide."""
    if len(args) == 2:
        fc, bw = args
        return Curried(lambda x: _Resonator(x, fc, bw))
    if len(args) != 3:
        error("Resonator(x, fc, bw) expected")
    return _Resonator(args[0], args[1], args[2])


def _shifted(x, k):
    """`x` delayed by the whole number of frames `k`, as Float64: `k` frames of +0.0, then bit copies of `x`, cut to the length
    of `x` -- the frames `Delay(x, k)` gives, bit for bit, without `SampleAt`'s table: frame n needs no frame of `x` but
    n - k, so a `BlockStream`, which keeps only a tail of its input, can compute it."""
    from .units import frames

    y = _Until(_Append([ArraySig(np.zeros((k, x.nch), dtype=x.dtype), x.fs), x]), nframes(x) * frames)
    return y if y.dtype == F64 else ToEltype(y, F64)


def _Sweep(x, kind, fc, q):
    what = "Sweep (Recur2)"
    kind = kind if isinstance(kind, type) else type(kind)
    if kind not in (Lowpass, Highpass, Bandpass):
        error(f"{what}: the response must be Lowpass, Highpass or Bandpass, not {kind!r}")
    x = _wrapper_input(what, x)
    fs = _rate_for(what, x, "a frequency in Hz")
    fc, q = _hz_param(what, "fc", x, fc), _hz_param(what, "q", x, q, strict=True)

    def fns(m, fc, q):
        w = 2.0 * math.pi * fc / fs
        cw = m.cos(w)
        alpha = m.sin(w) / (2.0 * q)
        a0 = 1.0 + alpha
        if kind is Lowpass:
            b0, b1 = (1.0 - cw) / 2.0, 1.0 - cw
            b2 = b0
        elif kind is Highpass:
            b0, b1 = (1.0 + cw) / 2.0, -(1.0 + cw)
            b2 = b0
        else:
            b0, b1, b2 = alpha, 0.0 * alpha, -alpha
        return 2.0 * cw / a0, -(1.0 - alpha) / a0, b0 / a0, b1 / a0, b2 / a0

    return _formulas(what, x, [fc, q], fns, [x, _shifted(x, 1), _shifted(x, 2)])


def Sweep(*args, q=math.sqrt(0.5)):
    """`Sweep(x, Lowpass | Highpass | Bandpass, fc, q=sqrt(1/2))`, curried `x | Sweep(Lowpass, fc)`: the audio-EQ-cookbook
    biquad with a cutoff (and a resonance) that may move -- a swept low-pass, a wah, an auto-filter driven by an envelope.
    With `w = 2 pi fc / framerate`, `alpha = sin(w) / (2 q)` and `a0 = 1 + alpha` it runs as a direct form I with the
    coefficients of frame n on all taps: `Recur2(2 cos(w) / a0, -(1 - alpha) / a0, (b0 x[n] + b1 x[n-1] + b2 x[n-2]) / a0)`,
    the taps `x[n-1]` and `x[n-2]` being the frames of `Delay(x, 1)` and `Delay(x, 2)` (bit copies with zeros in front), built
    as `x` appended to one and two frames of zeros so that they need no table.  `fc` is a
    frequency or a signal of Hz at the rate of `x`, `q > 0` a number or a signal.  `Bandpass` has a peak gain of 0 dB."""
    if len(args) == 2:
        kind, fc = args
        return Curried(lambda x: _Sweep(x, kind, fc, q))
    if len(args) == 4:
        return _Sweep(args[0], args[1], args[2], args[3])
    if len(args) != 3:
        error("Sweep(x, response, fc, q=...) expected")
    return _Sweep(args[0], args[1], args[2], q)


# --------------------------------------------------------------------------
# MovingMax / MovingMin: sliding-window extrema (no reference counterpart)
def _moving_frames(what, name, x, v):
    """`_comb_delay`'s rules: a whole number of frames, a `frames` quantity, or a time converted with the rate of x"""
    if isinstance(v, Quantity):
        if U.is_time(v):
            if x.fs is None:
                error(f"{what}: {name} given as a time needs the frame rate of x")
            return U.inframes_int(v, x.fs)
        if not U.is_frames(v):
            error(f"{what}: {name} {v} is neither a time nor a number of frames")
        v = v.value
    if not _real_number(v) or not math.isfinite(v) or v != math.floor(v):
        error(f"{what}: {name} must be a whole number of frames, not {v!r}")
    return int(v)


def _Moving(what, is_min, x, w, ahead, center):
    x = _assignal(x)
    if x.dtype not in (F32, F64):
        error(f"{what}: the signal x must be Float32 or Float64 (use `ToEltype`)")
    W = _moving_frames(what, "the window w", x, w)
    if W < 1:
        error(f"{what}: the window must be at least one frame ({W} given)")
    if center:
        if ahead is not None:
            error(f"{what}: give `center=True` or `ahead`, not both")
        A = (W - 1) // 2
    else:
        A = 0 if ahead is None else _moving_frames(what, "`ahead`", x, ahead)
    if A < 0 or A > W - 1:
        error(f"{what}: `ahead` must lie in [0, w - 1] = [0, {W - 1}] frames ({A} given): it is the part of the window after frame n")
    return MovingSignal(x, W - 1 - A, A, is_min)


def _moving_ctor(what, is_min):
    def ctor(*args, ahead=None, center=False):
        if len(args) == 1:
            w = args[0]
            return Curried(lambda x: _Moving(what, is_min, x, w, ahead, center))
        if len(args) != 2:
            error(f"{what}(x, w) expected")
        return _Moving(what, is_min, args[0], args[1], ahead, center)

    ctor.__name__ = ctor.__qualname__ = what
    return ctor


MovingMax = _moving_ctor("MovingMax", False)
MovingMax.__doc__ = """`MovingMax(x, w, *, ahead=0, center=False)`, curried `x | MovingMax(w, ahead=...)`: the sliding-window maximum.  With
`back = w - 1 - ahead`, frame n of a channel is the greatest of `x[k]` over `max(0, n - back) <= k <= min(N - 1, n + ahead)`:
the window is clipped to the signal, never padded, and the result has the length, rate, channels and sample type of `x`
(Float32 stays Float32: nothing is rounded).  `w` is the window length, at least one frame: a whole number of frames (a
number or a `frames` quantity) or a time, converted with the rate of `x`; `ahead`, in the same units, is how much of the
window lies after frame n (`0 <= ahead <= w - 1`); `center=True` is `ahead = (w - 1) // 2`.  The default is the causal
window `[n - w + 1, n]`.  The samples are ordered `-Inf < ... < -0.0 < +0.0 < ... < +Inf`, so `+0.0` beats `-0.0` and a
window of only `-0.0` gives `-0.0`; the result is a bit copy of the greatest sample.  A NaN anywhere in the window makes
the frame NaN (its payload is unspecified).  Maximum and minimum round nothing and are associative, so every way of
splitting the work gives the same bits: windows, `stream` blocks and the whole sink agree bit for bit where `x` does.
The dependence is local: a window or a `stream` block computes its own frames from its own range of `x` plus `back`
frames before and `ahead` after, so `stream` over the node is linear and an `x` of infinite length is accepted.
A `BlockStream` computes each push from the tail of the input it keeps (`back` frames of history; `ahead` frames of output wait
for their input) and gives the whole sink's bits; multi-GPU shards refuse the node."""
MovingMin = _moving_ctor("MovingMin", True)
MovingMin.__doc__ = """`MovingMin(x, w, *, ahead=0, center=False)`, curried `x | MovingMin(w, ahead=...)`: the sliding-window minimum, the
mirror image of `MovingMax`: the least sample of the clipped window under the same order, so `-0.0` beats `+0.0`, NaN
propagates, and the result equals `-MovingMax(-x)` bit for bit.  Window, units, result type, `stream`, `BlockStream` and
shards as for `MovingMax`."""


# --------------------------------------------------------------------------
# MovingSum / MovingMean / MovingRMS: sliding sums (no reference counterpart)
def _MovingSum(what, op, x, w, ahead, center):
    m = _Moving(what, False, x, w, ahead, center)  # (the window's rules and refusals, under this construct's name)
    return MovingSumSignal(m.signal, m.back, m.ahead, op)


def _moving_sum_ctor(what, op):
    def ctor(*args, ahead=None, center=False):
        if len(args) == 1:
            w = args[0]
            return Curried(lambda x: _MovingSum(what, op, x, w, ahead, center))
        if len(args) != 2:
            error(f"{what}(x, w) expected")
        return _MovingSum(what, op, args[0], args[1], ahead, center)

    ctor.__name__ = ctor.__qualname__ = what
    return ctor


MovingSum = _moving_sum_ctor("MovingSum", 0)
MovingSum.__doc__ = """`MovingSum(x, w, *, ahead=0, center=False)`, curried `x | MovingSum(w, ahead=...)`: the sliding-window sum.  With
`back = w - 1 - ahead`, frame n of a channel is the sum of `x[k]` over `max(0, n - back) <= k <= min(N - 1, n + ahead)`: the
window is clipped to the signal, and the result has the length, rate and channels of `x` and is Float64 (a Float32 `x`
widens exactly).  `w`, `ahead` and `center` as for `MovingMax`: whole frames, a `frames` quantity or a time converted with
the rate of `x`; `0 <= ahead <= w - 1`; `center=True` is `ahead = (w - 1) // 2`; the default is the causal window.
Floating-point addition does not associate, so the sum is taken over ONE tree that the absolute frame numbers, `back` and
`ahead` fix (tests/movingsum_ref.py; DESIGN.md "Moving sums"): runs of 16 frames, a Kogge-Stone scan over the runs of a
segment of up to 1024 frames, a suffix, whole segments and a prefix joined -- no partial sum is ever subtracted, so nothing
cancels, and windows, `stream` blocks and the whole sink agree bit for bit where `x` does.  What lies outside the signal
counts as `-0.0`, the additive identity: a window of only `-0.0` sums to `-0.0`.  The dependence is local: a window or a
`stream` block computes its own frames from its own range of `x` plus `back` frames before and `ahead` after, and an `x`
of infinite length is accepted.  A `BlockStream` streams the node like `MovingMax`, bit for bit; multi-GPU shards refuse it."""
MovingMean = _moving_sum_ctor("MovingMean", 1)
MovingMean.__doc__ = """`MovingMean(x, w, *, ahead=0, center=False)`, curried `x | MovingMean(w, ...)`: `MovingSum` divided by the number of
frames of the window that lie inside the signal (one IEEE division by that count as a Float64), so an edge frame is the
mean of what is there.  Window, units, result type, `stream`, `BlockStream` and shards as for `MovingSum`."""
MovingRMS = _moving_sum_ctor("MovingRMS", 2)
MovingRMS.__doc__ = """`MovingRMS(x, w, *, ahead=0, center=False)`, curried `x | MovingRMS(w, ...)`: the root of the mean square over the
window: the `MovingSum` tree over `x[k] * x[k]` (the product formed in Float64, exact for a Float32 `x`), divided by the
frames of the clipped window, and the square root of that, each rounded once.  Window, units, result type, `stream`,
`BlockStream` and shards as for `MovingSum`."""


# --------------------------------------------------------------------------
# MovingMedian / MovingQuantile: sliding rank filters (no reference counterpart)
MOVING_RANK_HALO = 1024  # csrc/kernels.h kRankHalo: the one form that is built takes a window of at most this many frames + 1


def _MovingRank(what, x, w, q, ahead, center):
    m = _Moving(what, False, x, w, ahead, center)  # (the window's rules and refusals, under this construct's name)
    if not _real_number(q) or not math.isfinite(q) or not 0.0 <= q <= 1.0:
        error(f"{what}: the quantile q must be a finite real number in [0, 1], not {q!r}")
    n = m.signal.nframes_helper()
    back, ahead = m.back, m.ahead
    if isinstance(n, (int, np.integer)):  # a known, finite length: a window longer than the signal is the signal
        back, ahead = min(back, int(n)), min(ahead, int(n))
    if back + ahead > MOVING_RANK_HALO:
        error(f"{what}: a window of {m.back + m.ahead + 1} frames is longer than the {MOVING_RANK_HALO + 1} frames that are built "
              "(one form: a tile and its halo in the device's local memory); a longer one is refused, not computed on the host")
    return MovingRankSignal(m.signal, m.back, m.ahead, q)


def MovingQuantile(*args, ahead=None, center=False):
    """`MovingQuantile(x, w, q, *, ahead=0, center=False)`, curried `x | MovingQuantile(w, q, ahead=...)`: the sliding-window
    quantile, a rank filter.  With `back = w - 1 - ahead`, frame n of a channel looks at the `m` samples `x[k]`,
    `max(0, n - back) <= k <= min(N - 1, n + ahead)` -- the window is clipped to the signal, never padded -- ordered
    `-Inf < ... < -0.0 < +0.0 < ... < +Inf` (the two zeros are distinct), and is a bit copy of the one of rank
    `floor(q * (m - 1))`, counted from 0: always a sample of the window, never an interpolation or an average.  The product is
    one Float64 multiplication and the floor is exact.  `q` is a finite number in [0, 1]: `q = 0` is `MovingMin` and `q = 1`
    is `MovingMax`, bit for bit; a window of one frame is `x` itself.  The result has the length, rate, channels and sample
    type of `x` (Float32 stays Float32: nothing is rounded).  A NaN anywhere in the clipped window makes the frame NaN (its
    payload is unspecified).  `w`, `ahead` and `center` as for `MovingMax`: whole frames, a `frames` quantity or a time
    converted with the rate of `x`; `0 <= ahead <= w - 1`; `center=True` is `ahead = (w - 1) // 2`; the default is the
    causal window `[n - w + 1, n]`.  A selection rounds nothing, so windows, `stream` blocks and the whole sink agree bit for
    bit where `x` does.  The dependence is local: a window or a `stream` block computes its own frames from its own range
    of `x` plus `back` frames before and `ahead` after, and an `x` of infinite length is accepted.  One form is built, a
    window of at most 1025 frames (counted after `back` and `ahead` are clipped to the length of `x`): a longer one is
    refused here and by the planner, never computed on the host.  A `BlockStream` streams the node like `MovingMax`, bit for bit; multi-GPU shards refuse it."""
    what = "MovingQuantile"
    if len(args) == 2:
        w, q = args
        return Curried(lambda x: _MovingRank(what, x, w, q, ahead, center))
    if len(args) != 3:
        error(f"{what}(x, w, q) expected")
    return _MovingRank(what, args[0], args[1], args[2], ahead, center)


def MovingMedian(*args, ahead=None, center=False):
    """`MovingMedian(x, w, *, ahead=0, center=False)`, curried `x | MovingMedian(w, center=True)`: the sliding-window median,
    `MovingQuantile` with `q = 0.5`: of the `m` samples of the clipped window the one of rank `(m - 1) // 2` -- the middle
    sample of an odd count and the LOWER of the two middle samples of an even count.  It is always a sample of the window,
    never an average: where `m` is even it differs from `np.median`, which averages the two.  With an odd `w` that happens
    only at the edges of the signal, where the window is clipped to an even count.  A declicker is
    `x - MovingMedian(x, 5, center=True)` and a threshold; the Hampel identifier takes
    `MovingMedian(|x - MovingMedian(x, w)|, w)`.  Order, zeros, NaN, window, units, result type, the limit of 1025 frames,
    `stream`, `BlockStream` and shards as for `MovingQuantile`."""
    what = "MovingMedian"
    if len(args) == 1:
        w = args[0]
        return Curried(lambda x: _MovingRank(what, x, w, 0.5, ahead, center))
    if len(args) != 2:
        error(f"{what}(x, w) expected")
    return _MovingRank(what, args[0], args[1], 0.5, ahead, center)


# --------------------------------------------------------------------------
# appending: src/appending.jl:59-76
def _Append(xs):
    xs = Uniform(xs, channels=True)
    if any(isknowninf(nframes(x)) for x in xs[:-1]):
        error("Cannot Append to the end of an infinite signal")
    El = xs[0].dtype
    for x in xs[1:]:
        El = promote_type(El, x.dtype)
    xs = [x if x.dtype == El else ToEltype(x, El) for x in xs]
    lens = [nframes(x) for x in xs]
    if any(isknowninf(n) for n in lens):
        ln = inflen
    elif any(n is None for n in lens):
        ln = None
    else:
        ln = sum(lens)
    return AppendSignals(xs, ln, El)


def Append(*xs):
    if len(xs) == 1:
        y = xs[0]
        return Curried(lambda x: _Append([x, y]))
    return _Append(list(xs))


def Prepend(*xs):  # src/appending.jl:30-31
    if len(xs) == 1:
        x0 = xs[0]
        return Curried(lambda y: _Append([x0, y]))
    return _Append(list(reversed(xs)))


# --------------------------------------------------------------------------
# ramps: src/ramps.jl:156-161,191-196,227-231,263-273
def _ramp_args(args):
    ln, fn = 10 * U.ms, "sinramp"
    for a in args:
        if callable(a) or isinstance(a, str):
            fn = a
        else:
            ln = a
    if isinstance(fn, np.ufunc):  # (a bare ufunc in the ramp position counts as marked: it is elementwise by definition)
        fn = Elementwise(fn)
    if isinstance(fn, Elementwise):  # any shape, as a device program of the ramp position (SO_RAMP_EXPR)
        fn.program([F64])
        return ln, fn
    if fn is sinramp:
        fn = "sinramp"
    elif fn is identity or getattr(fn, "__name__", "") == "identity":
        fn = "identity"
    if fn not in ("sinramp", "identity"):
        error("ramp function is an opaque closure for the HIP engine (sinramp, identity supported)")
    return ln, fn


def _is_sigarg(a):
    return isinstance(a, (AbstractSignal, np.ndarray, tuple, list)) or _is_torch(a)


def _mkramp(direction):
    def R(*args):
        if not args or not _is_sigarg(args[0]):
            return Curried(lambda x: R(x, *args))
        x = _assignal(args[0])
        ln, fn = _ramp_args(args[1:])
        return _OperateOn(MUL, [x, RampSignal(direction, x, ln, fn)])

    return R


RampOn = _mkramp("on")
RampOff = _mkramp("off")


def Ramp(*args):
    if not args or not _is_sigarg(args[0]):
        return Curried(lambda x: Ramp(x, *args))
    x = _assignal(args[0])
    return RampOff(RampOn(x, *args[1:]), *args[1:])


def FadeTo(*args):
    if len(args) < 2 or not _is_sigarg(args[1]):
        y, rest = args[0], args[1:]
        return Curried(lambda x: FadeTo(x, y, *rest))
    x, y = args[0], args[1]
    ln, fn = _ramp_args(args[2:])
    x, y = Uniform((x, y))
    if x.fs is None:
        error("Unknown frame rate is not supported by `FadeTo`.")
    n = U.inframes_int(U.maybeseconds(ln), x.fs)
    silence = _Until(NumberSig(0, None, dtype=y.dtype) if y.dtype != I64 else NumberSig(0),
                     (nframes(x) - n) * U.frames)
    return Mix(RampOff(x, ln, fn), Prepend(RampOn(y, ln, fn), silence))


# --------------------------------------------------------------------------
# filters: src/filters.jl:14-20,54-66,96-97,323-326
class _Response:
    """DSP.jl response types.  The CLASS is the tag of `Filt(Lowpass, 4kHz)`; an INSTANCE,
    `Highpass(8, fs=100)`, is DSP.jl's response object for `digitalfilter` (test/runtests.jl:365-367)."""

    def __init__(self, *bounds, fs=None):
        self.bounds = tuple(U.inHz(b) for b in bounds)
        self.fs = None if fs is None else float(U.inHz(fs))


class Lowpass(_Response): pass  # noqa: E701
class Highpass(_Response): pass  # noqa: E701
class Bandpass(_Response): pass  # noqa: E701
class Bandstop(_Response): pass  # noqa: E701


class ZeroPoleGain:
    """DSP.jl ZeroPoleGain (what `digitalfilter` returns)"""

    def __init__(self, z, p, k):
        self.z = np.asarray(z, dtype=np.complex128).ravel()
        self.p = np.asarray(p, dtype=np.complex128).ravel()
        self.k = float(k)


class SecondOrderSections:
    """DSP.jl SecondOrderSections: rows [b0 b1 b2 1 a1 a2] + gain"""

    def __init__(self, sos, gain=1.0):
        self.sos = np.asarray(sos, dtype=np.float64).reshape(-1, 6)
        self.gain = float(gain)


class Biquad:
    def __init__(self, b0, b1, b2, a1, a2):
        self.row = [float(b0), float(b1), float(b2), 1.0, float(a1), float(a2)]


# largest relative l2 distance between the impulse responses of a PolynomialRatio's direct form and of its factored
# cascade the engine accepts (so_tf_to_sos's residual; the suite holds Float64 results to 1e-8)
TF_RESIDUAL_MAX = 1e-9


class PolynomialRatio:
    """DSP.jl PolynomialRatio(b, a): FIR for a == [a0], one section for orders <= 2, otherwise factored into
    second-order sections by the library (so_tf_to_sos)"""

    def __init__(self, b, a):
        self.b = np.asarray(b, dtype=np.float64).ravel()
        self.a = np.asarray(a, dtype=np.float64).ravel()


def digitalfilter(response, method):
    """digitalfilter(Highpass(8, fs=fs), Chebyshev1(5, 1)) -> ZeroPoleGain, through the library's
    design entry point (the same code the named form `Filt(Highpass, 8Hz, ...)` uses)"""
    from . import _capi as K
    import ctypes as C

    if not isinstance(response, _Response) or response.fs is None:
        error("digitalfilter needs a response object with a frame rate, e.g. Highpass(8, fs=100)")
    order = method[1]
    ripple = method[2] if len(method) > 2 else 0.0
    cap = 2 * order + 2
    z = (C.c_double * (2 * cap))()
    p = (C.c_double * (2 * cap))()
    nz, npl, k = C.c_int32(0), C.c_int32(0), C.c_double(0)
    b = response.bounds
    st = K.lib().so_design_iir_zpk(K.FILT[_DESIGNS[type(response)]], b[0], b[1] if len(b) > 1 else 0.0, response.fs,
                                   K.METHOD[method[0]], order, ripple, z, C.byref(nz), p, C.byref(npl), cap, C.byref(k))
    if st != 0:
        error(K.last_error())
    zz = np.array(z[: 2 * nz.value]).view(np.complex128)
    pp = np.array(p[: 2 * npl.value]).view(np.complex128)
    return ZeroPoleGain(zz, pp, k.value)


def tf_to_sos(b, a):
    """(sos rows, gain, residual) of so_tf_to_sos: the direct-form coefficients factored into second-order sections"""
    from . import _capi as K
    import ctypes as C

    b = np.ascontiguousarray(np.atleast_1d(b), dtype=np.float64)
    a = np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64)
    cap = 6 * (max(len(a), len(b)) // 2 + 2)
    sos = (C.c_double * cap)()
    nsec, gain, resid = C.c_int32(0), C.c_double(0), C.c_double(0)
    dp = C.POINTER(C.c_double)
    st = K.lib().so_tf_to_sos(b.ctypes.data_as(dp), len(b), a.ctypes.data_as(dp), len(a), sos, cap, C.byref(nsec),
                              C.byref(gain), C.byref(resid))
    if st != 0:
        error(K.last_error())
    return np.array(sos[: 6 * nsec.value]).reshape(-1, 6), gain.value, resid.value


def tf_zero_input(b, a, si, nmax):
    """zero-input response of the direct form from state `si` (so_tf_zero_input), cut where it has decayed"""
    from . import _capi as K
    import ctypes as C

    b = np.ascontiguousarray(np.atleast_1d(b), dtype=np.float64)
    a = np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64)
    si = np.ascontiguousarray(si, dtype=np.float64).ravel()
    out = np.empty(max(int(nmax), 0), dtype=np.float64)
    used = C.c_int64(0)
    dp = C.POINTER(C.c_double)
    st = K.lib().so_tf_zero_input(b.ctypes.data_as(dp), len(b), a.ctypes.data_as(dp), len(a), si.ctypes.data_as(dp),
                                  len(si), out.ctypes.data_as(dp), len(out), C.byref(used))
    if st != 0:
        error(K.last_error())
    return out[: used.value]


def _raw_filter(h):
    """RawFilterFn(h) (reference src/filters.jl:89-97): a DSP.jl filter object -> what the engine
    lowers: SOS rows + gain (IIR; resolve_filter = DF2TFilter(h)) or FIR coefficients"""
    from . import _capi as K
    import ctypes as C

    if isinstance(h, (RawFilterFn, RawFirFn)):
        return h
    if isinstance(h, SecondOrderSections):
        return RawFilterFn(h.sos, h.gain)
    if isinstance(h, Biquad):
        return RawFilterFn([h.row], 1.0)
    if isinstance(h, ZeroPoleGain):
        z = np.ascontiguousarray(h.z).view(np.float64)
        p = np.ascontiguousarray(h.p).view(np.float64)
        cap = 6 * (len(h.p) + 2)
        sos = (C.c_double * cap)()
        nsec, gain = C.c_int32(0), C.c_double(0)
        st = K.lib().so_zpk_to_sos(z.ctypes.data_as(C.POINTER(C.c_double)), len(h.z),
                                   p.ctypes.data_as(C.POINTER(C.c_double)), len(h.p), h.k, sos, cap,
                                   C.byref(nsec), C.byref(gain))
        if st != 0:
            error(K.last_error())
        return RawFilterFn(np.array(sos[: 6 * nsec.value]).reshape(-1, 6), gain.value)
    if isinstance(h, PolynomialRatio):
        a0 = h.a[0]
        b, a = h.b / a0, h.a / a0
        if len(a) == 1:
            return RawFirFn(b)
        if len(a) <= 3 and len(b) <= 3:
            b = np.concatenate([b, np.zeros(3 - len(b))])
            a = np.concatenate([a, np.zeros(3 - len(a))])
            return RawFilterFn([[b[0], b[1], b[2], 1.0, a[1], a[2]]], 1.0)
        sos, gain, resid = tf_to_sos(b, a)
        if not resid <= TF_RESIDUAL_MAX:
            error("PolynomialRatio: the polynomials of this filter are too ill-conditioned to be factored into "
                  f"second-order sections (impulse responses differ by {resid:.1e}): pass SecondOrderSections or "
                  "ZeroPoleGain")
        return RawFilterFn(sos, gain)
    arr = np.asarray(h, dtype=np.float64)
    if arr.ndim == 1 and arr.size >= 1:  # FIR coefficient vector
        return RawFirFn(arr)
    error(f"Filt: unsupported filter object {h!r}")


def Butterworth(order):
    return ("butterworth", int(order))


def Chebyshev1(order, ripple):
    return ("chebyshev1", int(order), float(ripple))


def _nyquist_check(x, hz):
    if x.fs is not None and U.inHz(hz) >= 0.5 * x.fs:
        error(f"The frequency {hz} cannot be represented at a sampling rate of {x.fs} Hz. "
              "Increase the frame rate or lower the frequency.")


_DESIGNS = {Lowpass: "lowpass", Highpass: "highpass", Bandpass: "bandpass", Bandstop: "bandstop"}


def _is_signal_like(v):
    if isinstance(v, (ZeroPoleGain, SecondOrderSections, Biquad, PolynomialRatio, RawFilterFn, RawFirFn, FilterFn)):
        return False
    if isinstance(v, AbstractSignal) or _is_torch(v):
        return True
    if isinstance(v, tuple):
        return True
    if isinstance(v, np.ndarray):
        return v.ndim == 2  # a 1-D vector on its own is a coefficient vector: Filt(h)
    return False


def Filt(*args, blocksize=default_blocksize, order=5, method=None, sos=None, gain=1.0):
    if args and isinstance(args[0], type) and args[0] in _DESIGNS:  # curried Filt(Type,bounds...)
        a = args
        return Curried(lambda x: Filt(x, *a, blocksize=blocksize, order=order, method=method))
    if not args and sos is not None:
        return Curried(lambda x: Filt(x, blocksize=blocksize, sos=sos, gain=gain))
    if len(args) == 1 and not _is_signal_like(args[0]):  # curried Filt(h)
        h = args[0]
        return Curried(lambda x: Filt(x, h, blocksize=blocksize))
    x = _assignal(args[0])
    if sos is not None:  # Filt(x,h): raw DSP.jl filter object -> SOS rows
        return FilteredSignal(x, RawFilterFn(sos, gain), blocksize, x.fs)
    if len(args) == 2 and isinstance(args[1], FilterFn):
        return FilteredSignal(x, args[1], blocksize, x.fs)
    if len(args) == 2:  # Filt(x,h): RawFilterFn(h), reference src/filters.jl:96-97
        return FilteredSignal(x, _raw_filter(args[1]), blocksize, x.fs)
    if len(args) < 3 or not (isinstance(args[1], type) and args[1] in _DESIGNS):
        error("Filt(x, Type, bounds...) expected")
    if method is None:
        method = Butterworth(order)
    bounds = args[2:]
    for b in bounds:
        _nyquist_check(x, b)
    fn = FilterFn(_DESIGNS[args[1]], method, [U.inHz(b) for b in bounds])
    return FilteredSignal(x, fn, blocksize, x.fs)


def _Normpower(x):  # src/filters.jl:323-326
    x = _assignal(x)
    return NormedSignal(x)


Normpower = Curried(_Normpower)
