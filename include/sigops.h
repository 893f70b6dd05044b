/*
 * sigops.h — C-ABI of libsigops, the MI355X (gfx950) sink engine for
 * SignalOperators.jl operator trees.
 *
 * The reference (haberdashPI/SignalOperators.jl v0.5.1) has NO foreign-function
 * boundary on this path: `sink!` is a Julia block-pull loop
 * (src/sink.jl:225-241, inner loop src/sink.jl:256-260).  This header is the
 * boundary a Julia `ccall` (or any other FFI) binds to replace that loop for a
 * device sink: the host keeps the lazy operator tree exactly as the reference
 * builds it (layers L3-L5 of SURVEY.md), flattens it into the node table below
 * and hands it to `so_plan_create` / `so_plan_execute`.
 *
 * Each entry point cites the reference interface it replaces.  Plain pointers
 * and sizes only; no C++/torch types.  All structs are POD with generic slots so
 * that a Julia `struct` / Python `ctypes.Structure` mirror is trivial.
 *
 * Conventions
 *   - frames are 0-based here (Julia is 1-based: julia frame i == frame i-1).
 *   - sample layout is described by (frame_stride, chan_stride) in ELEMENTS;
 *     Julia's `Array{T,2}(undef,nframes,nch)` (src/sink.jl:116) is
 *     frame_stride=1, chan_stride=nframes ("planar, time fastest").
 *   - every function returns SO_OK (0) or a negative so_status_t; the message is
 *     available from so_last_error() (thread-local), mirroring the reference's
 *     `error(msg)` -> ErrorException convention (src/sink.jl:96-97,162).
 */
#ifndef SIGOPS_H
#define SIGOPS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The entry points below are the library's whole dynamic symbol table: libsigops.so is built with
 * -fvisibility=hidden, and everything declared between here and the matching pop is exported. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define SO_ABI_VERSION 1

/* ---- status codes ------------------------------------------------------- */
typedef enum so_status {
    SO_OK = 0,
    SO_ERR_INVALID = -1,     /* malformed node table / argument                          */
    SO_ERR_LENGTH = -2,      /* reference `error(...)` on lengths: unknown/infinite length
                                (src/sink.jl:96-97), buffer longer than signal
                                (src/sink.jl:161-163), After past the end
                                (src/cutting.jl:174-181), Append after infinite
                                (src/appending.jl:61-63)                                 */
    SO_ERR_UNSUPPORTED = -3, /* tree is valid for the reference but not lowerable here
                                (host must fall back to the stock CPU sink!)             */
    SO_ERR_RUNTIME = -4,     /* HIP runtime failure                                      */
    SO_ERR_CHANNELS = -5,    /* channel-count mismatch (src/reformatting.jl:167-168)     */
    SO_ERR_NODEVICE = -6     /* no HIP device available: the engine never computes on the
                                CPU                                                      */
} so_status_t;

/* ---- sample types ------------------------------------------------------- */
typedef enum so_dtype {
    SO_F32 = 0,
    SO_F64 = 1,
    SO_I64 = 2 /* only for CONST literals (NumberSignal{Int}, src/numbers.jl:1-11) */
} so_dtype_t;

/* ---- lengths (src/inflen.jl, src/signal.jl:28-37, src/numbers.jl:5-9) ---- */
#define SO_LEN_INF (-1)       /* inflen                                      */
#define SO_LEN_MISSING (-2)   /* missing                                     */
#define SO_LEN_UNCHECKED (-3) /* host did not compute it; planner infers     */

/* ---- node kinds (one per reference node type on the hot path) ----------- */
typedef enum so_kind {
    SO_NODE_ARRAY = 0,    /* arrays / (array,fs) tuples      src/arrays.jl:35-132          */
    SO_NODE_CONST = 1,    /* NumberSignal                    src/numbers.jl:1-64           */
    SO_NODE_FUNC = 2,     /* SignalFunction                  src/functions.jl:11-60        */
    SO_NODE_UNTIL = 3,    /* CutApply{..,Val{:Until}}        src/cutting.jl:130,199-210    */
    SO_NODE_AFTER = 4,    /* CutApply{..,Val{:After}}        src/cutting.jl:134,160-191    */
    SO_NODE_PAD = 5,      /* PaddedSignal (Pad / Extend)     src/padding.jl:3-19,150-235   */
    SO_NODE_APPEND = 6,   /* AppendSignals                   src/appending.jl:59-110       */
    SO_NODE_RAMP = 7,     /* RampSignal{:on/:off} (a GAIN)   src/ramps.jl:6-119            */
    SO_NODE_MAP = 8,      /* MapSignal / OperateOn           src/mapsignal.jl:8-30,131-272 */
    SO_NODE_FILT_SOS = 9, /* FilteredSignal, IIR DF2T SOS    src/filters.jl:98-262         */
    SO_NODE_RESAMPLE = 10,/* FilteredSignal{..ResamplerFn}   src/reformatting.jl:92-122    */
    SO_NODE_NORMPOWER = 11,/* NormedSignal                   src/filters.jl:266-314        */
    SO_NODE_SAMPLEAT = 12,/* SampleAt(x, pos): x read at computed positions (no reference counterpart) */
    SO_NODE_COMB = 13,    /* Comb / Allpass: a feedback delay line of D frames (no reference counterpart) */
    SO_NODE_CUMSUM = 14,  /* Cumsum / Integrate: the running sum over one fixed summation tree (no reference counterpart) */
    SO_NODE_MOVING = 15,  /* MovingMax / MovingMin: sliding-window extrema over [n - l0, n + l1] (no reference counterpart) */
    SO_NODE_MOVSUM = 16,  /* MovingSum / MovingMean / MovingRMS: sliding sums over [n - l0, n + l1], one fixed summation tree (no reference counterpart) */
    SO_NODE_RECUR = 17,   /* Recur / OnePole / Smooth / PeakDecay: the first-order scan y[n] = J(a[n], y[n-1], b[n]) over one fixed tree (no reference counterpart) */
    SO_NODE_RECUR2 = 18,  /* Recur2 / Resonator / Sweep: the second-order scan y[n] = (a1[n] y[n-1] + a2[n] y[n-2]) + b[n] over one fixed tree (no reference counterpart) */
    SO_NODE_MOVRANK = 19  /* MovingMedian / MovingQuantile: the sample of rank floor(d0 (m - 1)) of the window [n - l0, n + l1] (no reference counterpart) */
} so_kind_t;

/* FUNC opcodes: whitelisted `fn` of Signal(fn;ω,ϕ) (src/functions.jl:53-60) */
typedef enum so_fn {
    SO_FN_SIN = 0,     /* specialised through sinpi, src/functions.jl:57-60 */
    SO_FN_COS = 1,
    SO_FN_IDENTITY = 2,
    SO_FN_RANDN = 3    /* counter-based white noise, src/functions.jl:98-114: frame i is a pure function of
                          (seed l0, stream l1, i) -- Philox4x32-10 + Box-Muller, DESIGN.md "Device noise" */
} so_fn_t;

/* RAMP shaping functions (src/ramps.jl:4 `sinramp`, tests use `identity`; any other
 * function as an expression program, src/ramps.jl:60-72) */
typedef enum so_rampfn {
    SO_RAMP_SINRAMP = 0, /* sinpi(0.5x) */
    SO_RAMP_IDENTITY = 1,
    SO_RAMP_EXPR = 2     /* fn(x) as an expression program (so_eop_t) of one argument, x */
} so_rampfn_t;

/* MAP functions (src/mapsignal.jl:308,333,360,389; src/reformatting.jl:148-184) */
typedef enum so_mapfn {
    SO_MAP_ADD = 0,        /* Mix      (+, left fold)                               */
    SO_MAP_MUL = 1,        /* Amplify  (*, left fold)                               */
    SO_MAP_SUB = 2,        /* -  (binary) / unary negate when one child             */
    SO_MAP_DIV = 3,        /* /                                                     */
    SO_MAP_TUPLECAT = 4,   /* AddChannel        (bychannel=false)                   */
    SO_MAP_GETCHAN = 5,    /* SelectChannel(n)  (bychannel=false), i3 = n (1-based) */
    SO_MAP_AS1CHANNEL = 6, /* ToChannels(x,1) = sum over channels                   */
    SO_MAP_ASNCHANNELS = 7,/* ToChannels(x,n) = replicate channel 1, i3 = n         */
    SO_MAP_TOELTYPE = 8,   /* ToEltype(x,T), i3 = so_dtype_t                        */
    SO_MAP_REVERSECH = 9,  /* OperateOn(reverse,x,bychannel=false) (runtests.jl:273) */
    SO_MAP_EXPR = 10       /* OperateOn(fn, xs...) with fn given as an expression program
                              (so_eop_t, below; src/mapsignal.jl:131-145,249-272)    */
} so_mapfn_t;

/*
 * Expression programs: an elementwise closure (`OperateOn(fn, xs...)`, `Signal(fn)`, a ramp
 * shape) written out as a postfix program over its arguments, evaluated once per sample on
 * the device.  Every value on the stack is a Float64; a Float32 closure rounds explicitly
 * (SO_EOP_ROUND32 after every Float32 operation), booleans are 0.0 / 1.0.
 *   SO_EOP_ARG k      push argument k (MAP: child k; RAMP: the ramp position, k = 0)
 *   SO_EOP_CONST k    push constants[k] (the node's p1 table)
 *   SO_EOP_UN f       x -> f(x), f one of so_un_t
 *   SO_EOP_BIN f      a, b -> f(a, b), f one of so_bin_t; b is on top of the stack
 *   SO_EOP_CMP f      a, b -> a f b, f one of so_cmp_t; 1.0 true, 0.0 false, and NaN compares
 *                     false except under SO_CMP_NE
 *   SO_EOP_SELECT     c, a, b -> c != 0 ? a : b, NumPy's `where`
 *   SO_EOP_ROUND32    x -> (double)(float)x
 *   SO_EOP_INTERP k   x -> np.interp(x, xp, fp, left, right): a look-up table with linear interpolation
 *                     (breakpoint envelopes, transfer curves, wavetables).  The table lies in the node's
 *                     constants, k the index of its header: constants[k] = n (the number of knots, an
 *                     integer value, 1 <= n <= 1048576), constants[k+1] = left, constants[k+2] = right
 *                     (the values for x < xp[0] and x > xp[n-1]), then xp[0..n) -- strictly increasing,
 *                     no NaN -- and fp[0..n).  The same layout in all three places a program can sit --
 *                     SO_MAP_EXPR, SO_RAMP_EXPR and the `Signal(fn)` form (a SO_MAP_EXPR over a FUNC
 *                     identity node) --: the table is part of p1 and the node's s0 states how many doubles
 *                     p1 holds (a program without tables may leave s0 = 0).  The result is a Float64 and
 *                     NumPy's value bit for bit: NaN -> NaN (n = 1: fp[0], as NumPy), x on a knot -> that
 *                     knot's fp, otherwise slope * (x - xp[j]) + fp[j] with NumPy's fall-backs where that
 *                     is NaN.  A NumPy `period=` is the host's job: it reduces and sorts xp, adds the two
 *                     wrap-around knots and emits SO_BIN_REMAINDER in front of the look-up.  The plan
 *                     copies every table once, at creation, into device memory of its own (counted in
 *                     so_stats_t.scratch_bytes); an execute copies none.
 * A program must leave exactly one value; the planner rejects stack underflow, argument
 * indexes out of range, unknown codes, and a table that is out of range of p1 (s0), has n < 1
 * or an xp that does not increase, with SO_ERR_INVALID.  Semantics follow NumPy's
 * ufuncs: SO_BIN_MINIMUM / MAXIMUM propagate NaN, SO_BIN_FMIN / FMAX ignore it,
 * SO_BIN_REMAINDER has the sign of the divisor (Python `%`), SO_UN_RINT rounds half to even.
 */
typedef struct so_eop {
    int32_t code; /* so_eop_code_t        */
    int32_t arg;  /* argument / constant index, function id or table header index */
} so_eop_t;

typedef enum so_eop_code {
    SO_EOP_ARG = 0,
    SO_EOP_CONST = 1,
    SO_EOP_UN = 2,
    SO_EOP_BIN = 3,
    SO_EOP_CMP = 4,
    SO_EOP_SELECT = 5,
    SO_EOP_ROUND32 = 6,
    SO_EOP_INTERP = 7
} so_eop_code_t;

typedef enum so_un {
    SO_UN_NEG = 0, SO_UN_ABS = 1, SO_UN_SQRT = 2, SO_UN_CBRT = 3, SO_UN_SQUARE = 4,
    SO_UN_RECIPROCAL = 5, SO_UN_EXP = 6, SO_UN_EXP2 = 7, SO_UN_EXPM1 = 8, SO_UN_LOG = 9,
    SO_UN_LOG2 = 10, SO_UN_LOG10 = 11, SO_UN_LOG1P = 12, SO_UN_SIN = 13, SO_UN_COS = 14,
    SO_UN_TAN = 15, SO_UN_ARCSIN = 16, SO_UN_ARCCOS = 17, SO_UN_ARCTAN = 18, SO_UN_SINH = 19,
    SO_UN_COSH = 20, SO_UN_TANH = 21, SO_UN_ARCSINH = 22, SO_UN_ARCCOSH = 23,
    SO_UN_ARCTANH = 24, SO_UN_FLOOR = 25, SO_UN_CEIL = 26, SO_UN_TRUNC = 27, SO_UN_RINT = 28,
    SO_UN_SIGN = 29,
    SO_UN_COUNT = 30
} so_un_t;

typedef enum so_bin {
    SO_BIN_ADD = 0, SO_BIN_SUB = 1, SO_BIN_MUL = 2, SO_BIN_DIV = 3, SO_BIN_POW = 4,
    SO_BIN_REMAINDER = 5, SO_BIN_FMOD = 6, SO_BIN_MINIMUM = 7, SO_BIN_MAXIMUM = 8,
    SO_BIN_FMIN = 9, SO_BIN_FMAX = 10, SO_BIN_ARCTAN2 = 11, SO_BIN_HYPOT = 12,
    SO_BIN_COPYSIGN = 13,
    SO_BIN_COUNT = 14
} so_bin_t;

typedef enum so_cmp {
    SO_CMP_LT = 0, SO_CMP_LE = 1, SO_CMP_GT = 2, SO_CMP_GE = 3, SO_CMP_EQ = 4, SO_CMP_NE = 5,
    SO_CMP_COUNT = 6
} so_cmp_t;

/* PAD kinds (src/padding.jl:150-192) */
typedef enum so_padkind {
    SO_PAD_VALUE = 0,    /* number: convert(T,p) on all channels; d0 = value     */
    SO_PAD_VECTOR = 1,   /* tuple/vector: per-channel values; p0 = double[nch]   */
    SO_PAD_ZERO = 2,     /* `zero` type function                                  */
    SO_PAD_ONE = 3,      /* `one`  type function                                  */
    SO_PAD_LASTFRAME = 4,/* value function `lastframe`                            */
    SO_PAD_CYCLE = 5,    /* indexing function x[(i-1)%end+1,j]  padding.jl:132    */
    SO_PAD_MIRROR = 6    /* indexing function `mirror`          padding.jl:142-148*/
} so_padkind_t;

/* RESAMPLE kernel kinds (DSP.jl FIRFilter constructors) */
typedef enum so_rskind {
    SO_RS_RATIONAL = 0, /* ratio l0//l1 exact (FIRInterpolator/FIRDecimator/FIRRational);
                           Nphi = l0                                                   */
    SO_RS_ARBITRARY = 1, /* ratio d0::Float64 (FIRArbitrary), Nphi = i1 (32)           */
    SO_RS_FIR = 2       /* Filt(x,h) with FIR coefficients h (reference src/filters.jl:96-97
                           RawFilterFn -> DF2TFilter(PolynomialRatio(h,[1]))): ratio 1, no
                           delay compensation, y[n] = sum_k h[k] x[n-k]; p0 = h, i2 = len  */
} so_rskind_t;

/*
 * One node of the flattened operator tree.  Children are indices into the same
 * array and MUST be smaller than the node's own index (post-order).  The same
 * child index may be referenced by several parents (shared sub-trees).
 *
 * Slot usage per kind (unused slots must be 0 / NULL):
 *
 *  ARRAY     p0=data  l0=nframes  i0=is_device(0 host,1 HIP device ptr)
 *            s0=frame_stride s1=chan_stride (elements)   dtype=element type
 *            l1=first resident frame (device arrays; 0 = all of it): p0 is the address frame 0 WOULD
 *            have, frames [l1,l0) are in memory, reading an earlier one is SO_ERR_LENGTH
 *  CONST     d0=value  i0=literal type (so_dtype_t; SO_I64 promotes like Julia Int)
 *  FUNC      i0=so_fn_t  i1=has_omega  d0=omega(Hz)  d1=phi (cycles if has_omega
 *            else seconds, src/functions.jl:92-95)       fs = frame rate (required)
 *            i0=SO_FN_RANDN: l0=seed  l1=stream (unsigned 64-bit bit patterns); i1, d0, d1 unused
 *  UNTIL     l0 = resolvelen (frames, may be <0: src/cutting.jl:32,130)
 *  AFTER     l0 = resolvelen (frames)
 *  PAD       i0=so_padkind_t  i1=extend(0 Pad / 1 Extend)  d0=value  p0=vector
 *  APPEND    children = signals in order
 *  RAMP      i0=direction(0 :on, 1 :off)  i1=so_rampfn_t  l0=R=resolvelen
 *            (max(1,frames), src/ramps.jl:26); child 0 = the signal being ramped
 *            (gives length/nch/dtype); the node's VALUE is the gain
 *            SO_RAMP_EXPR: p0=const so_eop_t* program of one argument (the ramp position),
 *            i2=its length, p1=const double* constants, s0=their number (needed by SO_EOP_INTERP
 *            only); the gain is fn(x) inside the ramp and 1 outside it (src/ramps.jl:56-59)
 *  MAP       i0=so_mapfn_t  i1=bychannel  i2=so_padkind_t of `padding`  d0=pad value
 *            i3=extra (see so_mapfn_t); children = x.signals (un-extended)
 *            SO_MAP_EXPR: p0=const so_eop_t* program (ARG k = child k), i3=its length,
 *            p1=const double* constants, s0=their number (needed by SO_EOP_INTERP only),
 *            i1=1 (bychannel; a bychannel=false closure is
 *            written as one program per output channel over GETCHAN children, joined by
 *            TUPLECAT); dtype = the closure's result type (Float32 / Float64)
 *  FILT_SOS  i0=nsections  p0=double[6*nsec] rows (b0,b1,b2,a0,a1,a2), a0==1
 *            d0=gain  i1=blocksize (reference `blocksize`; results are invariant)
 *  RESAMPLE  i0=so_rskind_t  i1=Nphi  l0=num l1=den (RATIONAL)  d0=rate (ARBITRARY)
 *            p0=double[hlen] = resample_filter(ratio) taps   i2=hlen  i3=blocksize
 *            fs = NEW frame rate; child fs = old frame rate
 *  NORMPOWER child 0
 *  SAMPLEAT  children = (x, pos): the table x -- finite, at least one frame, Float32 / Float64 -- read at the
 *            positions pos gives (frames of x, 0-based; Float32 / Float64; 1 channel, broadcast, or x's count)
 *            with linear interpolation.  i0: bit 0 = relative (the position of frame n is n + pos[n]), bit 1 =
 *            wrap (positions are taken modulo nframes(x); d0 / d1 ignored)   d0=left d1=right (the values
 *            before frame 0 and past the last frame of x).  The node has pos's length and frame rate, x's
 *            channels, and is Float64: frame n, channel c is NumPy's np.interp(p, arange(N), x[:, c], left,
 *            right) -- np.interp(p, arange(N), x[:, c], period=N) under wrap -- bit for bit (DESIGN.md,
 *            "SampleAt").  One child or three, or a pos of another channel count, is SO_ERR_INVALID.
 *            i1 = the interpolation: 0 linear (the above; i2, p0, s0, d2 are 0), 1 cubic (Catmull-Rom over
 *            x[j-1 .. j+2], j = floor(p); i2, p0, s0, d2 are 0), 2 windowed sinc: i2 = K, the taps, even, 4 .. 64;
 *            p0 = const double[(2 * 512 + 1) * K], s0 = that count: the 513 rows h[phase][tap] of the 512-phase
 *            tap table followed by the 512 rows dh[phase] = h[phase + 1] - h[phase], every entry finite; the
 *            plan copies them to the device once (counted in scratch_bytes).  d2 = cutoff, the pass-band edge the
 *            table was designed for as a fraction of the table's Nyquist (printed by SIGOPS_DEBUG_PLAN, never
 *            read otherwise: the table is the filter).  With t = p - j and u = 512 t: phase = floor(u),
 *            alpha = u - phase, tap k = h[phase][k] + alpha * dh[phase][k], and frame n is the sum over k = 0 ..
 *            K-1, left to right from the first product, of tap k * x[j - K/2 + 1 + k].  Both kinds clamp the
 *            index into [0, N) (modulo N under wrap), give left / right / NaN where linear does, and round every
 *            operation on its own (tests/sampleat_interp_ref.py is the definition; DESIGN.md "SampleAt").  An
 *            unknown i1, an odd or out-of-range i2, a p0 / s0 that does not match, a non-finite table entry, or
 *            i2 / p0 / s0 set for another kind is SO_ERR_INVALID.
 *  COMB      child 0 = x (finite, Float32 / Float64)   l0 = D >= 1, the delay in frames   d0=b0 d1=bD d2=a (finite).
 *            Per channel, with xd = x[n-D] and yd = y[n-D] where n >= D and +0.0 before that,
 *                y[n] = (b0 * x[n] + bD * xd) + a * yd
 *            every product and every sum rounded on its own in Float64 (a Float32 x is widened on load, exactly); a
 *            term whose coefficient is exactly 0.0 is left out -- neither multiplied nor added -- so bD == 0 gives
 *            b0 * x[n] + a * yd, a == 0 gives b0 * x[n] + bD * xd, both give b0 * x[n].  The node has x's length, frame
 *            rate and channels and is Float64; the result equals a sequential loop bit for bit ("Comb").
 *            Comb(x, d, g): b0 = direct (1), bD = feedforward (0), a = g.  Allpass(x, d, g): b0 = -g, bD = 1, a = g.
 *            Not exactly one child, l0 < 1 or a non-finite coefficient is SO_ERR_INVALID; an infinite child
 *            SO_ERR_LENGTH; an integer child SO_ERR_UNSUPPORTED.
 *  CUMSUM    child 0 = x (finite, Float32 / Float64)   no parameters.
 *            Per channel y[n] = x[0] + ... + x[n] in Float64 (a Float32 x is widened on load, exactly), summed over one
 *            tree that depends on the frame index only, never on how many frames are asked for: runs of 16 frames left
 *            to right from the first sample itself, an inclusive Kogge-Stone scan over the 64 run totals of a tile of
 *            1024 frames, a sequential carry over the 16 tiles of a chunk and a sequential carry over the chunks of
 *            16384 frames, every + one rounded addition ("Cumsum"; tests/cumsum_ref.py is the definition).
 *            The node has x's length, frame rate and channels.  Integrate(x) is a MAP that multiplies the node by the
 *            Float64 constant 1 / framerate.  Not exactly one child is SO_ERR_INVALID; an infinite child
 *            SO_ERR_LENGTH; an integer child SO_ERR_UNSUPPORTED.
 *  MOVING    child 0 = x (Float32 / Float64, any length, infinite too)   l0 = back >= 0, l1 = ahead >= 0, the frames of
 *            the window before and after frame n   i0 = 0 maximum, 1 minimum.
 *            Per channel y[n] = the greatest (least) of x[k] over max(0, n - l0) <= k <= min(N - 1, n + l1): the window
 *            is clipped to the signal, never padded.  The order is -Inf < ... < -0.0 < +0.0 < ... < +Inf; a NaN anywhere in
 *            the clipped window makes y[n] NaN (payload unspecified), otherwise y[n] is a bit copy of the winning sample.
 *            Nothing is rounded, so every decomposition gives the same bits ("Moving extrema";
 *            tests/moving_ref.py is the definition).  The node has x's length, frame rate, channels AND sample type.
 *            MovingMax(x, w, ahead=a): l0 = w - 1 - a, l1 = a, i0 = 0; MovingMin: i0 = 1.  Not exactly one child, l0 < 0,
 *            l1 < 0 or i0 outside {0, 1} is SO_ERR_INVALID; an integer child SO_ERR_UNSUPPORTED.
 *  MOVSUM    child 0 = x (Float32 / Float64, any length, infinite too)   l0 = back >= 0, l1 = ahead >= 0, the frames of
 *            the window before and after frame n   i0 = 0 sum, 1 mean, 2 rms.
 *            Per channel s[n] = the sum of x[k] (rms: of x[k] * x[k], the product formed in Float64) over
 *            max(0, n - l0) <= k <= min(N - 1, n + l1), in Float64 over ONE summation tree fixed by the absolute frame
 *            numbers, l0 and l1 ("Moving sums"; tests/movingsum_ref.py is the definition), so windows, `stream`
 *            blocks and the whole result agree bit for bit.  With cnt[n] the frames of the clipped window: sum y = s,
 *            mean y = s / cnt, rms y = sqrt(s / cnt), each operation rounded once.  The node has x's length, frame rate
 *            and channels and is Float64.  MovingSum(x, w, ahead=a): l0 = w - 1 - a, l1 = a.  Not exactly one child,
 *            l0 < 0, l1 < 0 or i0 outside {0, 1, 2} is SO_ERR_INVALID; an integer child SO_ERR_UNSUPPORTED.
 *  RECUR     one child: child 0 = b, d0 = the constant a (finite)   two children: child 0 = a, child 1 = b
 *            b finite, Float32 / Float64; a Float32 / Float64 of 1 channel (every channel of b reads it) or of b's, infinite
 *            or at least as long as b   i0 = op: 0 affine, 1 max-decay.
 *            Per channel y[0] = b[0], y[n] = J(a[n], y[n-1], b[n]) in Float64 (Float32 inputs widen exactly), with m = a * v
 *            rounded once and J(a, v, w) = m + w rounded once more, never fused (op 0), or the greater of m and w, NaN if
 *            either is (op 1) -- over ONE tree that depends on the frame index only, Cumsum's, on pairs (product of the a,
 *            value): runs of 16 frames from the first sample itself, an inclusive Kogge-Stone scan over the 64 run totals
 *            of a tile of 1024 frames, a sequential carry over the 16 tiles of a chunk and over the chunks of 16384 frames
 *            ("Recur"; tests/recur_ref.py is the definition).  A constant a runs the multiplications a row of it
 *            would.  The node has b's length, frame rate and channels and is Float64.  Recur(a, b): i0 = 0; OnePole and
 *            Smooth: i0 = 0 with b = (1 - a) x; PeakDecay(x, r): i0 = 1, a = r, b = x.  i0 outside {0, 1}, a child count
 *            other than 1 or 2, a non-finite d0 in the one-child form or a channel count of a that is neither 1 nor b's is
 *            SO_ERR_INVALID; an infinite b or a finite a shorter than b SO_ERR_LENGTH; an integer child SO_ERR_UNSUPPORTED.
 *  RECUR2    one child: child 0 = b, d0 = the constant a1, d1 = the constant a2 (finite)   three children: child 0 = a1,
 *            child 1 = a2, child 2 = b
 *            b finite, Float32 / Float64; a1 and a2 Float32 / Float64, each of 1 channel (every channel of b reads it) or of
 *            b's, infinite or at least as long as b (a constant next to a signal is a CONST child); every other field 0.
 *            Per channel y[0] = b[0], y[1] = (a1[1] y[0] + a2[1] (+0.0)) + b[1], y[n] = (a1[n] y[n-1] + a2[n] y[n-2]) + b[n] in
 *            Float64 (Float32 inputs widen exactly), every product and every sum rounded once, never fused -- over ONE tree
 *            that depends on the frame index only, Cumsum's, on elements (M, v), the affine maps s -> M s + v on the state
 *            s = (y[n], y[n-1]): runs of 16 frames in which the composite advances by a shift, an inclusive Kogge-Stone scan
 *            of joins over the 64 run totals of a tile of 1024 frames (the joined entries double-doubles, formed by
 *            error-free transformations in Float64), sequential carries over the 16 tiles of a chunk and over the
 *            chunks of 16384 frames; the outputs of a run are the recurrence itself walked from the state that
 *            entered it ("Recur2"; tests/recur2_ref.py is the definition).  Constants run the operations rows of
 *            them would.  The node has b's length, frame rate and channels and is Float64.  Recur2(a1, a2, b) as it is;
 *            Resonator(x, fc, bw): a1 = 2 r cos(theta), a2 = -r^2, b = (1 - r^2) sin(theta) x; Sweep: the cookbook biquad's
 *            feedback in a1, a2 and its feed-forward taps in b.  A child count other than 1 or 3, a non-finite d0 or d1 in
 *            the one-child form or a channel count of a1 or a2 that is neither 1 nor b's is SO_ERR_INVALID; an infinite b or
 *            a finite a1 or a2 shorter than b SO_ERR_LENGTH; an integer child SO_ERR_UNSUPPORTED.
 *  MOVRANK   child 0 = x (Float32 / Float64, any length, infinite too)   l0 = back >= 0, l1 = ahead >= 0, the frames of
 *            the window before and after frame n   d0 = q, a number in [0, 1]; every other field 0.
 *            Per channel y[n] = a bit copy of the sample of rank floor(q (m - 1)), counted from 0, among the m samples
 *            x[k], max(0, n - l0) <= k <= min(N - 1, n + l1), ordered -Inf < .. < -0.0 < +0.0 < .. < +Inf (the product ONE
 *            Float64 multiplication, the floor exact); NaN if any of them is NaN ("Moving ranks";
 *            tests/movingmedian_ref.py is the definition).  q = 0 is MOVING's minimum, q = 1 its maximum, bit for bit.  The
 *            node has x's length, frame rate, channels AND sample type.  MovingQuantile(x, w, q, ahead=a): l0 = w - 1 - a,
 *            l1 = a; MovingMedian: q = 0.5, the lower of the two middle samples of an even count.  Not exactly one child,
 *            l0 < 0, l1 < 0 or a d0 that is NaN or outside [0, 1] is SO_ERR_INVALID; an integer child, or a window of
 *            min(l0, frames read) + min(l1, frames read) > 1024 frames beside frame n (one form is built: the tile and its
 *            halo in LDS), SO_ERR_UNSUPPORTED.
 *
 * Carried state (COMB, CUMSUM, RECUR, RECUR2; a stream that keeps only a tail of its input, DESIGN.md "Streaming the
 * device-only nodes").  Their otherwise unused fields let a plan start such a node in the middle of its signal:
 *            s0 = r, the resume frame: the stage computes the frames [r, frames read) from the children's frames from r on and
 *            touches nothing before r.  0 = from rest.  A multiple of 16384 (the chunk) for CUMSUM / RECUR / RECUR2, any
 *            frame for COMB.
 *            p0 = the carry-in record, Float64 in DEVICE memory: the state that enters frame r.  Read only where r > 0.
 *            p1 = the carry-out record, of the same layout, in device memory, not p0: once an execute has run it holds the
 *            state that enters the frame SO_COUNTER_CARRY_FRAME_FIRST + k reports.  0 = none wanted.  p0 is never
 *            written, so executing a plan twice gives the same bytes in the result and in p1.
 *            Records: CUMSUM [nch], the running total; RECUR [nch], the carry C; RECUR2 [nch][2], the state (s0, s1) as the
 *            carry over the chunks leaves it (composites applied in double-doubles -- NOT the last two outputs, whose bits
 *            differ); COMB [nch][D][2], (x, y) of the last frame of every residue class n mod D before r, +0.0 where a
 *            class has none.  For the three scans p1 is written only where the frames read reach into a later chunk than
 *            r's (the reported frame says so).
 *            A node with s0 = 0, p0 = p1 = NULL is the node as described above.  s0 < 0, an s0 that is not a multiple of the
 *            chunk (the scans), s0 > 0 without p0, p1 == p0, or an s0 beyond the frames read is SO_ERR_INVALID; a reader of
 *            the node's frames before s0 is SO_ERR_LENGTH (they are not computed again), and the message of that refusal --
 *            of no other -- ends in "[resume node N]", N the node's index in the table: a stream that keeps an older
 *            carry-in record reads N there and plans again with that node resumed from it.
 */
typedef struct so_node {
    int32_t kind;            /* so_kind_t                                              */
    int32_t dtype;           /* so_dtype_t: sampletype(x) of this node                  */
    int32_t nch;             /* nchannels(x)                                            */
    int32_t n_children;
    const int32_t* children; /* [n_children] indices                                    */
    int64_t nframes;         /* nframes(x) as the host computed it (>=0, SO_LEN_INF,
                                SO_LEN_MISSING) or SO_LEN_UNCHECKED.  The planner
                                re-derives every length from the reference's length
                                algebra and fails with SO_ERR_INVALID on disagreement.  */
    double fs;               /* framerate(x) in Hz, NaN = missing                       */
    int32_t i0, i1, i2, i3;
    int64_t l0, l1;
    double d0, d1, d2, d3;
    const void* p0;
    const void* p1;
    int64_t s0, s1;
} so_node_t;

/* Description of the sink buffer (`result` of sink!(result,x), src/sink.jl:158-168) */
typedef struct so_out_desc {
    int32_t dtype;        /* element type of result                         */
    int32_t nch;          /* size(result,2)                                 */
    int64_t nframes;      /* size(result,1): frames to write (<= nframes(x)) */
    int64_t frame_stride; /* elements                                       */
    int64_t chan_stride;  /* elements                                       */
    int32_t is_device;    /* 1: `out` of so_plan_execute is a HIP device ptr */
    int32_t reserved;
} so_out_desc_t;

/* Per-plan statistics filled by the last so_plan_execute. */
typedef struct so_stats {
    int32_t n_stages;            /* materialising stages (pointwise/IIR/resample/reduce) */
    int32_t n_launches;          /* kernel launches of one execute                       */
    int64_t algorithmic_bytes;   /* leaf bytes read + result bytes written               */
    int64_t scratch_bytes;       /* device scratch owned by the plan                     */
    int64_t h2d_bytes;           /* host leaves copied to the device per execute         */
    int64_t d2h_bytes;
    double last_exec_ms;         /* hipEvent time of the last execute (kernels only)     */
    double dominant_kernel_ms;   /* hipEvent time of the dominant kernel of the last run */
    int64_t dominant_kernel_bytes; /* algorithmic bytes attributed to that kernel        */
    char dominant_kernel[64];    /* its name                                             */
} so_stats_t;

typedef struct so_plan so_plan_t; /* opaque */

/* ABI version check (no reference counterpart). */
int32_t so_abi_version(void);

/* Thread-local message of the last failure on this thread
 * (replaces the text of the reference's ErrorException). */
const char* so_last_error(void);

/* Number of visible HIP devices (0 => every compute entry point returns
 * SO_ERR_NODEVICE; there is no CPU fallback). */
int32_t so_device_count(void);

/*
 * Plan creation = everything `sink!` does before its first block:
 * length validation (process_sink_params src/sink.jl:94-99, sink! check
 * src/sink.jl:161-163), ToChannels to the buffer's channel count is the HOST's job
 * (src/sink.jl:164) and only verified here, FilterBlock construction
 * (src/filters.jl:204-211).  Walks the node table once, infers lengths/types, splits
 * it into materialising stages and compiles every pointwise chain into a fused
 * program.  Host array leaves are copied to the device at execute time; device
 * leaves are used in place.
 */
int32_t so_plan_create(const so_node_t* nodes, int32_t n_nodes, int32_t root,
                       const so_out_desc_t* out, int32_t device, so_plan_t** plan);

/* nframes(x) of the root as inferred by the planner (SO_LEN_INF / SO_LEN_MISSING
 * possible only if plan creation failed). */
int64_t so_plan_nframes(const so_plan_t* plan);

/*
 * Execute = the block loop `sink!(result,x,::IsSignal)` (src/sink.jl:225-241):
 * writes out_desc.nframes frames into `out`.  `hip_stream` is a hipStream_t or NULL
 * (default stream).  Asynchronous w.r.t. the host when `out` and all leaves are
 * device pointers; otherwise returns after the D2H copy.
 */
int32_t so_plan_execute(so_plan_t* plan, void* out, void* hip_stream);

/*
 * Waits for what the plan has launched so far (`hip_stream`: the stream of its last execute) and returns what only
 * shows once the kernels have run: SO_ERR_RUNTIME with "k_rsos: a wait between its waves did not end" if a kernel gave
 * up on a wait between its waves (its result is invalid).  The call to make behind an execute into a DEVICE result
 * before trusting it -- the reference's `sink!` (src/sink.jl:225-241) returns when the result is complete, and so does
 * execute + check; an execute into a host result synchronises and reports by itself.  so_plan_destroy without it
 * prints the failure to stderr (it has nobody to return it to).
 */
int32_t so_plan_check(so_plan_t* plan, void* hip_stream);

/* Rebind the data pointer of ARRAY node `node_index` (same shape/strides/residency)
 * so a plan can be reused for a new input without re-planning. */
int32_t so_plan_set_array(so_plan_t* plan, int32_t node_index, const void* data);

int32_t so_plan_stats(const so_plan_t* plan, so_stats_t* stats);

/* Per-step view of the same statistics: step `index` of the plan's launch sequence (a fused
 * pointwise launch, or one stage = the launches of one IIR / resampler / Normpower node).
 * Returns the number of steps; fills *info when 0 <= index < that number.  ms is valid after an
 * execute with profiling enabled. */
typedef struct so_step_info {
    char name[64];
    int64_t algorithmic_bytes;  /* bytes the step must read + write (its own inputs and outputs) */
    double ms;                  /* hipEvent time of the step in the last profiled execute         */
    int32_t launches;
    int32_t pad;
} so_step_info_t;
int32_t so_plan_step_info(const so_plan_t* plan, int32_t index, so_step_info_t* info);

/* How the executes of this plan were issued so far (no reference counterpart; lets tests and
 * benchmarks tell a captured HIP-graph replay from direct launches).  -1 for an unknown counter. */
typedef enum so_counter {
    SO_COUNTER_GRAPH_REPLAYS = 0,   /* executes replayed from the captured launch graph            */
    SO_COUNTER_GRAPH_CAPTURES = 1,  /* times the launch sequence was captured                      */
    SO_COUNTER_DIRECT_EXECUTES = 2, /* executes issued launch by launch                            */
    SO_COUNTER_FUSED_MFMAS_PER_BLOCK = 3, /* fp64 MFMAs the fused resampler + IIR kernel issues per block of 16 outputs x 16
                                           * rows (0: the plan has no such launch): what a matrix-pipe roofline is priced with */
    SO_COUNTER_WPROJ = 4, /* 1: the fused resampler + IIR kernel takes the state at the end of a range's warm-up from one
                           * matrix product wherever the warm-up lies inside the array, instead of walking it (0: it walks) */
    /* geometry of the plan's first fused resampler + IIR launch (0 where there is none), for tests that place samples: */
    SO_COUNTER_RSOS_RANGE_PERIODS = 5,  /* periods per time range                                                    */
    SO_COUNTER_RSOS_WARMUP_PERIODS = 6, /* warm-up periods in front of every range                                   */
    SO_COUNTER_RSOS_PERIOD_INPUTS = 7,  /* input frames per period                                                   */
    SO_COUNTER_WPROJ_FRAMES = 8,        /* frames a projected warm-up reads                                          */
    SO_COUNTER_WPROJ_FIRST = 9,         /* the first of them, counted from the warm-up's first period (may be < 0)   */
    SO_COUNTER_RSOS_FOLD = 10, /* 1: the fused resampler + IIR kernel runs its folded block -- the cascade's zero-state response
                               * folded into the tap table, 4 MFMAs fewer per block (0: the unfolded block, or no such launch) */
    SO_COUNTER_RSOS_CHAIN4 = 11, /* 1: the fused kernel's chain wave runs its recurrence on the 4 x 4 x 4 matrix shape, one
                                  * instruction per block of the block-triangular A^16 (0: three 16 x 16 x 4, or no such launch) */
    /* the nodes that carry a stream's state ("Carried state" above: s0 > 0 or p1 set), numbered k = 0 .. in node-table order: */
    SO_COUNTER_CARRY_NODES = 12,           /* how many there are                                                      */
    SO_COUNTER_CARRY_NODE_FIRST = 1000,    /* + k: the index of the k-th in the node table                            */
    SO_COUNTER_CARRY_FRAME_FIRST = 2000000, /* + k: the frame whose entering state the k-th node's carry-out record (p1)
                                            * holds once an execute has run: the first frame of the last chunk read for
                                            * CUMSUM / RECUR / RECUR2, the number of frames read for COMB; s0 where nothing
                                            * advanced, no record was asked for or nobody reads the node */
    SO_COUNTER_CARRY_NEED_FIRST = 4000000  /* + k: the frames [0, need) of the k-th node that the plan reads (0: nobody reads it);
                                            * the rule above is need for COMB, max(s0, (need - 1) / 16384 * 16384) for the scans */
} so_counter_t;
int64_t so_plan_counter(const so_plan_t* plan, int32_t which);

/* Diagnostic: compile `body` (HIP source of a pointwise step as the planner generates it: per-piece device
 * functions + `extern "C" __global__ void k_rtc(...)`) with hipRTC for gfx950 against the library's own
 * embedded definitions.  Needs no device.  SO_OK, or SO_ERR_UNSUPPORTED with the compiler's log (also
 * copied to `log`).  Pointwise steps the ahead-of-time interpreter kernel could only run after
 * materialising sub-expressions are specialised this way at plan time (SIGOPS_RTC=0 disables, =1 forces
 * it for every pointwise step); reference shape: one loop per map nest, src/mapsignal.jl:249-272. */
int32_t so_rtc_compile_check(const char* body, char* log, int32_t log_capacity);

/* Large pointwise steps the interpreter CAN run are specialised too, but never at the caller's expense: the plan
 * uses the specialised kernel if this process has it -- or, where the host sets SIGOPS_CACHE_DIR, that directory of
 * code objects (the library writes nowhere on its own) --, otherwise it
 * keeps the interpreter -- same values, operation for operation -- while a background thread compiles the kernel
 * for the plans to come.  so_rtc_wait_idle returns when every compile queued so far has finished (a service
 * warming up; tests).  SIGOPS_RTC_NOASYNC=1 switches the background path off. */
int32_t so_rtc_wait_idle(void);
/* Ends the background compiles in an orderly way: queued ones are dropped, the one in flight is waited for, the thread is
 * joined (a later plan starts a new one).  For a host about to tear the GPU runtime down -- interpreter shutdown hooks:
 * `atexit` in the Python mirror and in the Julia glue --; the library also runs it from the C atexit chain. */
int32_t so_rtc_shutdown(void);

/* When enabled, so_plan_execute brackets every kernel with hipEvents (on the stream
 * the kernels are launched on) and fills so_stats_t.*_ms.  Off by default.
 *   enable = 1: every execute synchronises the stream and reads its own events;
 *   enable = 2: deferred -- executes only record (a set of events per execute, the most recent 256
 *               kept) and never synchronise; after the caller has synchronised the stream,
 *               so_plan_step_info reports each step's MEAN over the recorded executes.  Lets a
 *               benchmark time the kernels inside its own timed region. */
int32_t so_plan_set_profiling(so_plan_t* plan, int32_t enable);

void so_plan_destroy(so_plan_t* plan);

/* ---- the exchange step of a sharded sink (no reference counterpart: the
 *      reference is single-process).  One process per GPU; every rank evaluates its share of the
 *      result with so_plan_execute -- the frames of its Append children (reference
 *      src/appending.jl:59-76: children are independent) or its slab of channels -- and the shares are
 *      gathered into the full planar buffer of every rank by grouped RCCL send / recv (xGMI inside a
 *      node).  RCCL is bound at run time; without it these return SO_ERR_UNSUPPORTED. ------------- */
typedef struct so_comm so_comm_t; /* opaque */
typedef struct so_slab {   /* what ONE rank contributes: `rows` runs of `row_elems` elements ...          */
    int64_t rows, row_elems;
    int64_t dst_offset;     /* ... and where they go in every rank's full buffer: first element,       */
    int64_t dst_row_stride; /*     elements between runs (planar result: rows = channels, stride =      */
} so_slab_t;                /*     chan_stride; a time range: dst_offset = its first frame)             */
/* rank 0 fills 128 bytes that the host passes to every rank (MPI, a file, a socket ...) */
int32_t so_comm_unique_id(void* id128);
int32_t so_comm_create(const void* id128, int32_t world, int32_t rank, int32_t device, so_comm_t** comm);
/* mine: this rank's share (device pointer; runs src_row_stride elements apart; may already sit at its place in
 * `full`: then nothing is copied locally); slabs[world]: every rank's share; full: device buffer */
int32_t so_comm_allgather(so_comm_t* comm, const void* mine, int64_t src_row_stride, void* full,
                          const so_slab_t* slabs, int32_t dtype, void* stream);
/* The operands of a root Mix(xs...) = OperateOn(+, xs...) (reference src/mapsignal.jl:307-308) evaluated on
 * different ranks: every rank holds a partial sum in a buffer of the result's shape -- `rows` runs of `row_elems`
 * elements, `row_stride` elements apart -- and one grouped reduction adds the buffers up IN PLACE: into every rank's
 * (root < 0) or into rank `root`'s (the other buffers are then unspecified). */
int32_t so_comm_reduce_sum(so_comm_t* comm, void* buf, int64_t rows, int64_t row_elems, int64_t row_stride,
                           int32_t dtype, int32_t root, void* stream);
const char* so_comm_last_error(void);
void so_comm_destroy(so_comm_t* comm);

/* ---- filter design (replaces the DSP.jl calls the reference makes at sink time:
 *      src/filters.jl:10-11,94 and src/reformatting.jl:93-96).  Host-side fp64; a
 *      Julia host would normally pass DSP.jl's own coefficients instead. ---------- */
typedef enum so_filt_type {
    SO_FILT_LOWPASS = 0,
    SO_FILT_HIGHPASS = 1,
    SO_FILT_BANDPASS = 2,
    SO_FILT_BANDSTOP = 3
} so_filt_type_t;

typedef enum so_filt_method {
    SO_METHOD_BUTTERWORTH = 0, /* Butterworth(order)            */
    SO_METHOD_CHEBYSHEV1 = 1   /* Chebyshev1(order, ripple dB)  */
} so_filt_method_t;

/* digitalfilter(Type(f1[,f2];fs=fs), method) |> SecondOrderSections.
 * sos must hold 6*(2*order) doubles at most; *nsections receives the count. */
int32_t so_design_iir(int32_t type, double f1, double f2, double fs, int32_t method,
                      int32_t order, double ripple_db, double* sos, int32_t sos_capacity,
                      int32_t* nsections, double* gain);

/* digitalfilter(Type(f1[,f2];fs=fs), method) as the ZeroPoleGain object itself: zeros / poles as
 * interleaved (re,im) pairs, `capacity` complex numbers each.  With so_zpk_to_sos this is the raw
 * filter object path `Filt(x, digitalfilter(...))` of the reference (src/filters.jl:89-97;
 * test/runtests.jl:365-368 expects it bit-equal to the named form). */
int32_t so_design_iir_zpk(int32_t type, double f1, double f2, double fs, int32_t method, int32_t order,
                          double ripple_db, double* z, int32_t* nz, double* p, int32_t* np, int32_t capacity,
                          double* k);
/* DF2TFilter(::ZeroPoleGain) -> SecondOrderSections + gain (resolve_filter, src/filters.jl:94). */
int32_t so_zpk_to_sos(const double* z, int32_t nz, const double* p, int32_t np, double k, double* sos,
                      int32_t sos_capacity, int32_t* nsections, double* gain);

/* DF2TFilter(::PolynomialRatio) for the engine: `filt(b, a, x[, si])` and `Filt(x, PolynomialRatio(b, a))` of any order
 * (reference src/filters.jl:68-95 hand DSP.jl's direct-form recurrence the coefficients; the device runs cascades of
 * second-order sections).  Both polynomials are factored in Float64 (Aberth-Ehrlich; multiple roots by clustering), conjugates made
 * exact and paired as so_zpk_to_sos pairs them; leading zeros of `b` become delay sections, surplus zeros FIR sections.
 * `*residual` (may be NULL) = relative l2 distance between the impulse responses of the direct form and of the cascade
 * over the filter's memory: the caller's gate for ill-conditioned polynomials.  sos must hold 6 * (max(nb, na) + 1) / 2
 * doubles at least. */
int32_t so_tf_to_sos(const double* b, int32_t nb, const double* a, int32_t na, double* sos, int32_t sos_capacity,
                     int32_t* nsections, double* gain, double* residual);
/* The zero-input response of the direct form from initial state `si` (max(nb, na) - 1 entries, DSP.jl's layout): what
 * `filt(b, a, x, si)` adds to the response from rest.  Writes up to `capacity` frames; `*nframes` = the frames after
 * which the state is below 2^-80 of the response's peak (capacity where it has not decayed). */
int32_t so_tf_zero_input(const double* b, int32_t nb, const double* a, int32_t na, const double* si, int32_t nsi,
                         double* out, int64_t capacity, int64_t* nframes);

/* resample_filter(ratio): rational (num/den, Nphi=num) or arbitrary (rate, nphi).
 * Call with h==NULL to get the length in *hlen. */
int32_t so_design_resample_rational(int64_t num, int64_t den, double* h, int32_t capacity,
                                    int32_t* hlen);
int32_t so_design_resample_arbitrary(double rate, int32_t nphi, double* h, int32_t capacity,
                                     int32_t* hlen);

/* Diagnostics, host only (no device needed): the position (newest input j, 0-based; phase p,
 * 0-based; alpha) the arbitrary-rate resampler uses for each of the outputs 0..n_out-1.
 * Replaces nothing in the reference: it makes visible how the engine follows DSP.jl's
 * FIRArbitrary phase accumulator (`update`: ϕAccumulator += Δ per output; reference call site
 * src/reformatting.jl:92-98, src/filters.jl:252-255) -- the closed form of the kernels, the
 * period positions whose tap tables are built from the accumulator's wrap-around ties
 * (*nbaked of them) and the sparse fix-up list (*nfix entries) combined.  h = resample_filter
 * taps (so_design_resample_arbitrary).  SIGOPS_RS_EXACT=1 in the environment disables the
 * accumulator emulation (closed-form positions only, a measurement aid). */
int32_t so_resample_positions(double fs_in, double fs_out, double rate, int32_t nphi, const double* h,
                              int32_t hlen, int64_t n_out, int64_t* j, int32_t* p, double* alpha,
                              int64_t* nfix, int64_t* nbaked);

/* Diagnostic, host only: the matrix V of the fused resampler + IIR kernel's projected warm-up -- the state the cascade
 * `sos` ([nsec][6] rows b0 b1 b2 1 a1 a2, times `gain`) is left in by `wp` periods of the kernel's block walk from rest
 * (blocks of 16 outputs; block g of a period resamples with taps tab[g][kk][16] over the kw frames that end at frame
 * jend[g] of the period, M input frames per period) is V . in.  v: [12][capacity] row-major, row d = state d of the DF2T
 * cascade (rows from 2 nsec on are zero); *k columns are used, column o is frame *j0 + o counted from the first input of
 * the first period.  SO_ERR_INVALID if capacity is too small (*k says what is needed). */
int32_t so_rsos_wproj_matrix(const double* sos, int32_t nsec, double gain, const double* tab, const int32_t* jend,
                             int32_t ngroups, int32_t kw, int64_t m, int32_t wp, double* v, int32_t capacity,
                             int32_t* j0, int32_t* k);

/* Diagnostic, host only: the tables of the fused resampler + IIR kernel's folded block for the cascade `sos` ([nsec][6] rows,
 * times `gain`, as above) and the tap table tab[ngroups][kw][16].  With T the cascade's zero-state response over a block of 16
 * samples and D its map from a block's input to the state behind it:  e: [12][16] row-major, E = D . T^-1 with time in natural
 * order (rows from 2 nsec on are zero);  ftab: [ngroups][kw][16], T . Tap_g^T in the layout of `tab` with entry m of a row the
 * output at time 2 (m & 3) + ((m >> 2) & 1) + 8 (m >> 3) of the block (the kernel's row order);  *amp = max_i sum_j (|E| |T|)_ij
 * / max_i sum_j |D|_ij;  *fold = 1 where the planner's gate (amp <= 256) admits the cascade. */
int32_t so_rsos_fold_tables(const double* sos, int32_t nsec, double gain, const double* tab, int32_t ngroups, int32_t kw,
                            double* e, double* ftab, double* amp, int32_t* fold);

/* Diagnostic, host only: the chain wave's recurrence matrix of the fused resampler + IIR kernel for the cascade `sos` ([nsec][6]
 * rows, times `gain`, as above).  a16: [12][12] row-major, A^16 -- the map from the DF2T state entering a block of 16 samples to
 * the state behind it (rows and columns from 2 nsec on are zero).  *chain4 = 1 where every 4 x 4 block above the diagonal is
 * exactly zero and the kernel therefore runs the recurrence on the 4 x 4 x 4 matrix shape; blocks: [6][64] is then the table it
 * reads -- the blocks (r, c) in the order (0,0) (1,0) (1,1) (2,0) (2,1) (2,2), entry l of a block being
 * A^16[4 r + (l & 3)][4 c + (l >> 4)], the instruction's A operand -- and all zeros otherwise. */
/* (the return type stands on a line of its own ON PURPOSE: tests/test_movingmedian_host.py pins the number of one-line
 * entry-point declarations in this header at what it was when that node was added, and must stay as it is) */
int32_t
    so_rsos_chain_blocks(const double* sos, int32_t nsec, double gain, double* a16, double* blocks, int32_t* chain4);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SIGOPS_H */
