"""A NumPy evaluator for composite trees of the device-only nodes (`SampleAt` with linear, cubic and windowed-sinc
interpolation, `Comb` / `Allpass`, `Cumsum`, `MovingMax` / `MovingMin`, `MovingSum` / `MovingMean` / `MovingRMS`, `Recur` /
`PeakDecay`, `Recur2`, `MovingMedian` / `MovingQuantile`) under the structural operators, and the generator of random trees
of that grammar.  `evaluate(tree)` walks the Python signal objects and never calls the engine: the structural operators are
slices and concatenations, `Mix` and `Amplify` are single IEEE additions and multiplications, and every device-only node
is evaluated by its own definition (tests/*_ref.py), so every tree of the grammar has ONE expected value, bit for bit.
tests/test_tree_ref_host.py holds the structural part to the CPU oracle bit for bit and every node's branch to a direct
call of its definition; tests/test_gpu_node_trees.py holds the device to `evaluate`.

The grammar (every signal at one frame rate, FS = 10 kHz):

    leaves      Float64 arrays of 1 or nch channels; Float32 arrays where no arithmetic touches them before a device-only
                node or the root: under `Until` / `After` / `Pad` / `Append` among Float32 only, and under a node
    structure   `Until`, `After`, `Pad(zero | one | number | lastframe | cycle | mirror) | Until`, `Append`,
                `ToChannels` (mono -> n), `Mix(x, y)`, `Mix(x, number)`, `Amplify(x, y)`, `Amplify(x, number)`: unequal
                lengths (the shorter operand is extended with 0.0 under `Mix` and 1.0 under `Amplify`, and the operation
                is carried out there too: -0.0 + 0.0 is +0.0) and mono against n channels
    nodes       nine families (`FAMILIES`), their parameters as their own test files map them: the six of `SIX`, and
                "Recur2" (constants or two coefficient rows: three inputs), "MovingRank" (it keeps the sample type, as the
                extrema do: a Float32 one stands where a Float32 extremum may) and "SampleAtFir", a `SampleAt` whose
                `interp` is "cubic" or "sinc" ("SampleAt" is the linear one)

The random trees come in two sets.  `SEEDS` draw from `SIX`, the families the generator began with, and their trees are
pinned by digest (tests/golden/tree_seeds.json): a change to the generator must not move them.  `SEEDS_ALL` draw from all
nine.

Outside the grammar, deliberately: generators (`sin` on the device is not NumPy's `sin` bit for bit), `Ramp`, `FadeTo`,
`Filt`, `ToFramerate`, `Normpower`, Float32 arithmetic, `OnePole` / `Smooth` / `Integrate` (a scaling map over the node) and
`Resonator` / `Sweep` (their coefficient maps use the device's `cos` and `exp`, which are not NumPy's bit for bit: with
constants they are `Recur2` over a scaled input, and tests/test_gpu_recur2.py holds them).

Refused by design, and therefore not generated: `Pad(x, cycle)` and `Pad(x, mirror)` over anything but an array leaf
(the engine and the oracle raise the reference's "indexing pad function" error: the pad indexes its child, and only an
array can be indexed); signals of no frames (`After` never takes a whole signal, `Until` at least one frame); a moving
rank whose window is longer than the 1025 frames that are built."""
import hashlib
import math

import numpy as np

import sigops_amd as so
from sigops_amd import signals as S

from comb_ref import DELAYS, comb_ref
from cumsum_ref import CH, L, T, cumsum_ref
from moving_ref import moving_ref
from movingmedian_ref import movrank_ref
from movingsum_ref import B, TILE, movingsum_ref
from recur2_ref import recur2_ref
from recur_ref import recur_ref
from sampleat_interp_ref import sampleat_interp
from sampleat_ref import sampleat_np

FS = 10 * so.kHz
NODE_TYPES = (S.SampleAtSignal, S.CombSignal, S.CumsumSignal, S.MovingSignal, S.MovingSumSignal, S.RecurSignal, S.Recur2Signal,
              S.MovingRankSignal)
SIX = ("SampleAt", "Comb", "Cumsum", "Moving", "MovingSum", "Recur")  # what the generator began with: the trees of `SEEDS`
FAMILIES = SIX + ("Recur2", "MovingRank", "SampleAtFir")


# ---- the evaluator -----------------------------------------------------------------------------------------------------
def _finite_len(x):
    n = S.nframes(x)
    return None if n is None or S.isknowninf(n) else int(n)


def _pad_value(pad):
    if pad is S.zero:
        return 0.0
    if pad is S.one:
        return 1.0
    assert isinstance(pad, (int, float)) and not isinstance(pad, bool), pad
    return float(pad)


def _extend(base, n, pad, child):
    """the first n >= len(base) frames of `Pad(child, pad)`; base holds all of child"""
    N = base.shape[0]
    if n <= N:
        return base[:n]
    if pad is S.lastframe:
        tail = np.repeat(base[N - 1:N], n - N, axis=0)
    elif pad is S.cycle or pad is S.mirror:
        assert isinstance(child, S.ArraySig), "an indexing pad reads an array leaf"
        f = np.arange(N, n)
        k, rem = f // N, f % N
        tail = base[rem if pad is S.cycle else np.where(k % 2 == 0, rem, N - 1 - rem)]
    else:
        tail = np.full((n - N, base.shape[1]), _pad_value(pad), dtype=base.dtype)
    return np.concatenate([base, tail], axis=0)


def _ev(x, n, memo):
    """the first n frames of x (all of a finite x for n None), frames x channels in x's sample type"""
    if n is not None and isinstance(x, NODE_TYPES) and _finite_len(x) is not None:
        assert n <= _finite_len(x)
        return _ev(x, None, memo)[:n]  # (a node's first n frames are the first n of all of them: one call of its definition)
    key = (id(x), n)
    if key not in memo:
        memo[key] = _ev1(x, n, memo)
    return memo[key]


def _ev1(x, n, memo):
    N = _finite_len(x)
    if n is None:
        assert N is not None, "an infinite signal needs a frame count"
        n = N
    assert N is None or n <= N
    if isinstance(x, S.ArraySig):
        d = np.asarray(x.data)
        return d.reshape(d.shape[0], -1)[:n]
    if isinstance(x, S.NumberSig):
        return np.full((n, 1), x.val, dtype=x.dtype)
    if isinstance(x, S.CutApply):
        k = x.resolvelen()
        return _ev(x.signal, n, memo) if x.kind == "until" else _ev(x.signal, k + n, memo)[k:]
    if isinstance(x, S.PaddedSignal):
        return _extend(_ev(x.signal, None, memo), n, x.pad, x.signal)
    if isinstance(x, S.AppendSignals):
        parts, rem = [], n
        for c in x.signals:
            m = _finite_len(c)
            m = rem if m is None else min(m, rem)
            if m > 0:
                parts.append(_ev(c, m, memo))
            rem -= m
        assert rem == 0
        return np.concatenate(parts, axis=0)
    if isinstance(x, S.MapSignal):
        if x.fn == S.ASNCHANNELS:
            return np.repeat(_ev(x.signals[0], n, memo), int(x.extra), axis=1)
        if x.fn == S.TOELTYPE:
            return _ev(x.signals[0], n, memo).astype(np.dtype(x.extra))
        assert x.fn in (S.ADD, S.MUL) and x.bychannel, x.fn
        acc = None
        for c in x.signals:
            m = _finite_len(c)
            v = _ev(c, n, memo) if m is None else _extend(_ev(c, min(m, n), memo), n, x.padding, c)
            with np.errstate(all="ignore"):
                acc = v if acc is None else (np.add(acc, v) if x.fn == S.ADD else np.multiply(acc, v))
        assert acc.dtype == x.dtype
        return acc
    if isinstance(x, S.SampleAtSignal):
        table, pos = _ev(x.signal, None, memo), _ev(x.pos, n, memo)
        if x.interp == "linear":
            return sampleat_np(table, pos, x.left, x.right, x.relative, x.wrap)
        return sampleat_interp(table, pos, x.interp, x.left, x.right, x.relative, x.wrap, taps=x.taps, cutoff=x.cutoff)
    if isinstance(x, S.CombSignal):
        return comb_ref(_ev(x.signal, None, memo), x.delay, x.b0, x.bD, x.a)[:n]
    if isinstance(x, S.CumsumSignal):
        return cumsum_ref(_ev(x.signal, None, memo))[:n]
    if isinstance(x, (S.MovingSignal, S.MovingSumSignal, S.MovingRankSignal)):
        # (an infinite child: the window is clipped at the front only, and `ahead` more frames are all frame n - 1 reaches)
        child = _ev(x.signal, None if _finite_len(x.signal) is not None else n + x.ahead, memo)
        if isinstance(x, S.MovingSignal):
            return moving_ref(child, x.back, x.ahead, x.is_min)[:n]
        if isinstance(x, S.MovingRankSignal):
            return movrank_ref(child, x.back, x.ahead, x.q)[:n]
        return movingsum_ref(child, x.back, x.ahead, x.op)[:n]
    if isinstance(x, S.RecurSignal):
        b = _ev(x.signal, None, memo)
        a = x.a if x.coef is None else _ev(x.coef, b.shape[0], memo)
        return recur_ref(a, b, x.op)[:n]
    if isinstance(x, S.Recur2Signal):
        b = _ev(x.signal, None, memo)
        # (a coefficient row may have one channel against b's, and more frames than b: the first of them are read)
        a1, a2 = (x.a1, x.a2) if x.coefs is None else (_ev(c, b.shape[0], memo) for c in x.coefs)
        return recur2_ref(a1, a2, b)[:n]
    raise AssertionError(f"outside the grammar: {type(x).__name__}")


def evaluate(tree):
    """the whole of a finite tree -> frames x channels, planar (Fortran order), in the tree's sample type"""
    tree = S._assignal(tree)
    out = _ev(tree, None, {})
    assert out.dtype == tree.dtype and out.shape[1] == tree.nch
    return np.asfortranarray(out)


# ---- what a tree holds -------------------------------------------------------------------------------------------------
def family(x):
    if not isinstance(x, NODE_TYPES):
        return None
    if isinstance(x, S.SampleAtSignal) and x.interp != "linear":
        return "SampleAtFir"
    return (SIX + ("Recur2", "MovingRank"))[NODE_TYPES.index(type(x))]


def digest(a):
    """sha256 over the sample type, the shape and the bytes (planar) of an array"""
    a = np.asfortranarray(a)
    h = hashlib.sha256()
    h.update(f"{a.dtype.str} {a.shape}".encode())
    h.update(a.tobytes(order="F"))
    return h.hexdigest()


def _through_cuts(x):
    while isinstance(x, S.CutApply):
        x = x.signal
    return x


def walk(tree):
    """every signal object of the tree once, with the number of parents that read it"""
    seen, order = {}, []
    stack = [S._assignal(tree)]
    while stack:
        x = stack.pop()
        if id(x) in seen:
            seen[id(x)] += 1
            continue
        seen[id(x)] = 1
        order.append(x)
        stack.extend(x.children)
    return [(x, seen[id(x)]) for x in order]


def census(tree):
    """-> (the families that occur, the placements that occur): `under_root_append` a node that is a child of a root
    `Append`; `over_append_or_pad` a node whose input is an `Append` or a `Pad` (through `Until` / `After`);
    `pad_behind_node` a `Pad` whose child is a node (through `Until` / `After`); `two_readers` a node two parents read"""
    tree = S._assignal(tree)
    fams, places = set(), set()
    if isinstance(tree, S.AppendSignals) and any(isinstance(c, NODE_TYPES) for c in tree.signals):
        places.add("under_root_append")
    for x, readers in walk(tree):
        if isinstance(x, NODE_TYPES):
            fams.add(family(x))
            if readers >= 2:
                places.add("two_readers")
            if any(isinstance(_through_cuts(c), (S.AppendSignals, S.PaddedSignal)) for c in x.children):
                places.add("over_append_or_pad")
        if isinstance(x, S.PaddedSignal) and isinstance(_through_cuts(x.signal), NODE_TYPES):
            places.add("pad_behind_node")
    return fams, places


def placed(tree):
    """-> the set of (family, placement) of the tree's nodes, the placements as `census` has them, each told of the node
    itself: the child of the root `Append`, the node over an `Append` or a `Pad`, the node behind the `Pad`, the node read twice"""
    tree = S._assignal(tree)
    out = set()
    if isinstance(tree, S.AppendSignals):
        out.update((family(c), "under_root_append") for c in tree.signals if isinstance(c, NODE_TYPES))
    for x, readers in walk(tree):
        if isinstance(x, NODE_TYPES):
            if readers >= 2:
                out.add((family(x), "two_readers"))
            if any(isinstance(_through_cuts(c), (S.AppendSignals, S.PaddedSignal)) for c in x.children):
                out.add((family(x), "over_append_or_pad"))
        if isinstance(x, S.PaddedSignal) and isinstance(_through_cuts(x.signal), NODE_TYPES):
            out.add((family(_through_cuts(x.signal)), "pad_behind_node"))
    return out


# ---- the generator -----------------------------------------------------------------------------------------------------
SEEDS = (11, 12, 13, 14, 15)       # the seeds of test_random_node_trees: trees of `SIX`
SEEDS_ALL = (21, 22, 23, 24, 25)   # and these: trees of all of `FAMILIES`
TREES_PER_SEED = 20
SHORT = [1, 2, L - 1, L, L + 1, 255, T - 1, T, T + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 77]
LONG = [CH - 1, CH, CH + 1, CH + T + 77]
MARKS = [1, L - 1, L, L + 1, T - 1, T, T + 1, TILE - 1, TILE, TILE + 1, CH - 1, CH, CH + 1]
WINDOWS = [1, 2, 3, 16, 17, 33, 480, B, B + 1, B + 2, TILE + 1, TILE + 2, 2 * TILE + 1]
NUMBERS = [0.5, -1.25, 2.5, 1.0, 0.0, -0.0]
RANK_WINDOWS = [1, 2, 3, 5, 16, 17, 33, 65, 257, 1024, 1025]  # 1025: the longest window that is built
RANK_Q = [0.0, 0.1, 0.5, 0.9, 1.0]
RANK_LONG = 4 * T   # over more frames than this, a window above 257 is kept one time in six (the definition sorts every window)
STABLE_PAIRS = [(1.8, -0.9), (1.2, -0.5), (0.0, 0.25), (-0.5, 0.0), (0.0, 0.0)]  # `Recur2`'s constants: poles inside the circle
FIR_KINDS = [dict(interp="cubic"), dict(interp="sinc"), dict(interp="sinc", taps=4), dict(interp="sinc", taps=64),
             dict(interp="sinc", taps=10, cutoff=0.5)]


def _length(rng):
    return int(rng.choice(LONG if rng.random() < 0.2 else SHORT))


def _data(rng, n, nch, dtype=np.float64):
    """normal samples with a few zeros of both signs"""
    x = rng.standard_normal((n, nch)).astype(dtype)
    for v in (0.0, -0.0):
        x[rng.integers(0, n, 1 + n // 500), rng.integers(0, nch)] = v
    return np.asfortranarray(x)


def _leaf(rng, nch, dtype=np.float64, n=None):
    return so.Signal(_data(rng, n or _length(rng), nch, dtype), FS)


def _beside(rng, n, lo=0):
    """a frame count in [lo, n) on or beside a boundary of the kernels where n allows, else anywhere"""
    c = [m for m in MARKS if lo <= m < n]
    return int(rng.choice(c)) if c and rng.random() < 0.8 else int(rng.integers(lo, n))


def _cut(rng, x):
    """`After` and / or `Until` that leave at least one frame"""
    n = S.nframes(x)
    how = rng.integers(0, 3) if n > 1 else 1
    if how != 1:
        k = _beside(rng, n, 1)
        x, n = x | so.After(k * so.frames), n - k
    if how != 0:
        x = x | so.Until(_beside(rng, n + 1, 1) * so.frames)
    return x


def _pad(rng, x, indexing=False):
    n = S.nframes(x)
    kinds = [so.zero, so.one, so.lastframe, float(rng.choice(NUMBERS))] + ([so.cycle, so.mirror] if indexing else [])
    p = kinds[rng.integers(0, len(kinds))]
    k = int(rng.choice([1, 3, L + 1, n + 3, 2 * n + 1]))
    return so.Pad(x, p) | so.Until((n + min(k, 3 * T)) * so.frames)


class _Gen:
    def __init__(self, rng, nodes=True, families=SIX):
        """with the default families every draw is what it was when there were six: the trees of `SEEDS` stay"""
        self.rng = rng
        self.nodes = nodes
        self.families = tuple(families)

    # -- Float32: nothing but structure, the extrema and the moving ranks, which keep the type
    def f32(self, nch, depth):
        rng = self.rng
        kinds = 4 + (1 + ("MovingRank" in self.families) if self.nodes else 0)
        how = rng.integers(0, kinds) if depth > 0 else 0
        if how == 0:
            return _leaf(rng, nch, np.float32)
        if how == 1:
            return _cut(rng, self.f32(nch, depth - 1))
        if how == 2:
            x = self.f32(nch, depth - 1)
            return _pad(rng, x, isinstance(x, S.ArraySig))
        if how == 3:
            return so.Append(*[self.f32(nch, depth - 1) for _ in range(rng.integers(2, 4))])
        return (self.moving if how == 4 else self.rank)(self.f32(nch, depth - 1))

    # -- the nodes
    def moving(self, x):
        rng = self.rng
        w = int(rng.choice(WINDOWS))
        return (so.MovingMax, so.MovingMin)[rng.integers(0, 2)](x, w, ahead=int(rng.choice([0, (w - 1) // 2, w - 1])))

    def rank(self, x):
        rng = self.rng
        w = int(rng.choice(RANK_WINDOWS))
        if w > 257 and S.nframes(x) > RANK_LONG and rng.random() >= 1 / 6:
            w = int(rng.choice([v for v in RANK_WINDOWS if v <= 257]))
        q, ahead = float(rng.choice(RANK_Q)), int(rng.choice([0, (w - 1) // 2, w - 1]))
        return so.MovingMedian(x, w, ahead=ahead) if q == 0.5 and rng.random() < 0.5 else so.MovingQuantile(x, w, q, ahead=ahead)

    def coefficients2(self, n, nch):
        """`Recur2`'s a1 and a2 for a b of n frames: two numbers, or two rows (resonator pairs, or U[-1, 1] and U[-0.5, 0.5],
        as tests/recur2_ref.py `coef`) of one channel or nch each, at times an `Append` of two rows or longer than b"""
        rng = self.rng
        if rng.random() < 0.3:
            return STABLE_PAIRS[rng.integers(0, len(STABLE_PAIRS))]
        m = n + 7
        shape = (m, 1 if rng.random() < 0.5 else nch)
        if rng.random() < 0.5:
            r, th = rng.uniform(0.5, 0.9995, shape), rng.uniform(0.0, math.pi, shape)
            a1, a2 = 2.0 * r * np.cos(th), -(r * r)
        else:
            a1, a2 = rng.uniform(-1.0, 1.0, shape), rng.uniform(-0.5, 0.5, shape)
        if shape[1] > 1 and rng.random() < 0.4:  # (one of the two mono, the other of nch channels)
            a2 = a2[:, :1]
        row = lambda a, lo, hi: so.Signal(np.asfortranarray(a[lo:hi]), FS)  # noqa: E731
        out = []
        for a in (a1, a2):
            if n > 2 and rng.random() < 0.4:
                k = _beside(rng, n, 1)
                out.append(so.Append(row(a, 0, k), row(a, k, n + int(rng.choice([0, 5])))))
            else:
                out.append(row(a, 0, n + int(rng.choice([0, 0, 7]))))
        return tuple(out)

    def operand(self, nch, depth):
        """a node's input: Float64, or (one time in five) a Float32 structure"""
        return self.f32(nch, min(depth, 2)) if self.rng.random() < 0.2 else self.f64(nch, depth)

    def coefficients(self, n, nch, lo, hi):
        """`Recur`'s a for a b of n frames: a number, or a row of one channel or nch, at times an `Append` of two rows or
        longer than b"""
        rng = self.rng
        if rng.random() < 0.3:
            return float(rng.choice([0.999, 0.5, 0.0, 1.0, -0.75 if lo < 0 else 0.25]))
        c = 1 if rng.random() < 0.5 else nch
        row = lambda m: so.Signal(np.asfortranarray(rng.uniform(lo, hi, (m, c))), FS)  # noqa: E731
        if n > 2 and rng.random() < 0.4:
            k = _beside(rng, n, 1)
            return so.Append(row(k), row(n - k + int(rng.choice([0, 5]))))
        return row(n + int(rng.choice([0, 0, 7])))

    def positions(self, ntable, nch):
        """positions inside and slightly outside a table of ntable frames, of one channel or nch"""
        rng = self.rng
        n, c = _length(rng), 1 if rng.random() < 0.5 else nch
        p = rng.uniform(-2.0, ntable + 1.0, (n, c))
        p[rng.integers(0, n, 1 + n // 100), 0] = rng.integers(0, ntable, 1 + n // 100)  # (knots themselves)
        pos = so.Signal(np.asfortranarray(p), FS)
        if rng.random() < 0.3:  # a ramp plus a small signal: arithmetic on the positions
            pos = so.Mix(so.Signal(np.asfortranarray(np.linspace(0.0, ntable - 1.0, n).reshape(-1, 1)), FS),
                         so.Signal(np.asfortranarray(rng.uniform(-3.0, 3.0, (max(1, n - 5), c))), FS))
        return pos

    def node(self, nch, depth):
        rng = self.rng
        fam = self.families[rng.integers(0, len(self.families))]
        # (an extremum or a rank keeps Float32, and arithmetic may follow this node: a Float32 one comes from `f32` alone)
        x = self.f64(nch, depth - 1) if fam in ("Moving", "MovingRank") else self.operand(nch, depth - 1)
        n = S.nframes(x)
        if fam in ("SampleAt", "SampleAtFir"):
            kind = FIR_KINDS[rng.integers(0, len(FIR_KINDS))] if fam == "SampleAtFir" else {}
            return so.SampleAt(x, self.positions(n, nch), left=float(rng.choice([0.0, -1.5])), right=float(rng.choice([0.0, 2.0])),
                               wrap=bool(rng.random() < 0.25), **kind)
        if fam == "Recur2":
            return so.Recur2(*self.coefficients2(n, nch), x)
        if fam == "MovingRank":
            return self.rank(x)
        if fam == "Comb":
            D, g = int(rng.choice(DELAYS)), float(rng.choice([0.7, -0.8, 0.5, 0.6]))
            return so.Allpass(x, D, g) if rng.random() < 0.4 else so.Comb(x, D, g, feedforward=float(rng.choice([0.0, -0.35])))
        if fam == "Cumsum":
            return so.Cumsum(x)
        if fam == "Moving":
            return self.moving(x)
        if fam == "MovingSum":
            w = int(rng.choice(WINDOWS))
            ctor = (so.MovingSum, so.MovingMean, so.MovingRMS)[rng.integers(0, 3)]
            return ctor(x, w, ahead=int(rng.choice([0, (w - 1) // 2, w - 1])))
        if rng.random() < 0.5:
            return so.Recur(self.coefficients(n, nch, -1.0, 1.0), x)
        return so.PeakDecay(x, r=self.coefficients(n, nch, 0.0, 1.0))

    def shared(self, nch, depth):
        """one node read by two parents"""
        rng = self.rng
        n = self.node(nch, depth)
        if S.nframes(n) < 3:
            return so.Append(n, n)
        N = S.nframes(n)
        k, j = _beside(rng, N, 1), _beside(rng, N + 1, 1)
        how = rng.integers(0, 3)
        if how == 0:
            return so.Append(n | so.After(k * so.frames), n | so.Until(j * so.frames))
        if how == 1:
            return so.Mix(n, n | so.After(k * so.frames))
        return so.Amplify(n, n | so.Until(j * so.frames))

    # -- Float64
    def f64(self, nch, depth):
        rng = self.rng
        if depth <= 0:
            return _leaf(rng, nch)
        how = rng.integers(0, 12)
        if how >= 8 and self.nodes:
            if how == 11:
                return self.shared(nch, depth)
            n = self.node(nch, depth)
            return _pad(rng, n) if rng.random() < 0.2 else n
        how %= 8
        if how == 0:
            return _leaf(rng, nch)
        if how == 1:
            return _cut(rng, self.f64(nch, depth - 1))
        if how == 2:
            x = self.f64(nch, depth - 1)
            return _pad(rng, x, isinstance(x, S.ArraySig))
        if how == 3:
            return so.Append(*[self.f64(nch, depth - 1) for _ in range(rng.integers(2, 4))])
        if how == 4 and nch > 1:
            return so.ToChannels(self.f64(1, depth - 1), nch)
        op = so.Mix if rng.random() < 0.5 else so.Amplify
        if how == 5:
            return op(self.f64(nch, depth - 1), float(rng.choice(NUMBERS)))
        kids = [self.f64(1 if nch > 1 and rng.random() < 0.3 else nch, depth - 1), self.f64(nch, depth - 1)]
        return op(*(kids if rng.random() < 0.5 else kids[::-1]))

    def tree(self, nch, depth):
        if self.nodes and self.rng.random() < 0.3:  # a root `Append` of nodes: what window aliasing takes
            return so.Append(*[self.node(nch, depth - 1) for _ in range(self.rng.integers(2, 4))])
        return self.f32(nch, depth) if self.rng.random() < 0.1 else self.f64(nch, depth)


def random_tree(rng, nch, depth, nodes=True, families=SIX):
    """a finite tree of the grammar with nch channels, at most `depth` operators deep (depth <= 4), with at least one
    device-only node of `families` -- or, with `nodes=False`, of the structural operators alone, which the oracle can evaluate"""
    assert 1 <= depth <= 4
    while True:
        t = _Gen(rng, nodes, families).tree(nch, depth)
        if not nodes or census(t)[0]:
            return t


def random_trees(seed, count=TREES_PER_SEED, nodes=True, families=None):
    """the trees of one seed: [(nch, tree)], channel counts 1, 2 and 3 and depths 2 to 4 in turn; of all of `FAMILIES` for a
    seed of `SEEDS_ALL` and of `SIX` for any other, where `families` does not say"""
    if families is None:
        families = FAMILIES if seed in SEEDS_ALL else SIX
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        nch = (1, 2, 3)[i % 3]
        out.append((nch, random_tree(rng, nch, 2 + (i % 3), nodes, families)))
    return out
