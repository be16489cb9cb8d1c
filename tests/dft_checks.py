"""The instrument of the transform tests (tests only): k_dft, every length and engine, against the float64 matrix it replaces.

The model (``transform_model``) has no neurons.  Per length d, table-driven Nodes whose row at timestep t is test vector t feed
``transform_in(d, 'A'|'B', invert)`` into Nodes of 4H slots (H = d // 2 + 1) and ``transform_out(d)`` into a Node of d, all
with ``synapse=None``; built with ``build(net, staged=False)`` these are matvecs of the f32 core with ``dft`` = 1..5.  The
reference is ``OracleSimulator`` on the same model - float64, the matrix itself -, and ``tests/test_dft.py`` pins that matrix to
``np.fft``.  Every test value is made as float32 and widened, so the device sees exactly what the reference sees.

The bar.  For a row x of a transform with matrix T the scale is ``A = max_k (|T| |x|)_k`` (``||x||_1`` for the forward kinds:
the DC row of |T| is all ones; for the inverse kind plus the float64 matrix's own error, see ``scale``), and EVERY output element of
EVERY row has to satisfy ``|device - oracle| <= c u A``, ``u = 2^-24``.
``c`` depends on the engine class only and is not chosen freely: ``C0[cls]`` is the worst ratio ``error / (u A)`` that the NumPy
float32 stand-in below (``standin``) reaches over every row of every kind of every length of the class in ``SWEEP`` and ``LONG``
(``measure_c0()`` recomputes it, ``tests/test_dft.py`` holds a subset to half a bar), and ``C = 2 C0``: the margin of 2 is for
what the stand-in does not reproduce - which products the compiler contracts into fused multiply-adds, and the summation order
inside a matrix-core instruction.

First-order worst case (``analytic_c``), which every C has to stay below - a bar above it would test nothing.  Relative to the
1-norm of what enters a pass, one output of
  * a generic radix-r pass is a chain of r complex fused multiply-adds with rounded twiddles: at most (r + 2) u;
  * an in-register radix 2 / 4 / 8 pass is log2 r levels of additions (u each), the W8 products of radix 8 (2 u) and one complex
    product with a rounded twiddle (3 u): at most log2 r + 5 (the in-place passes form twiddle powers by up to three further
    products: + 9).
A direct transform of passes r_1 .. r_P is therefore within ``P(d) = sum_i pass(r_i)`` plus 2 u for the load (s0 - s1, s2 + s3 of
the inverse) and 2 u for the store (1 / d, the add of ``inc``).  Bluestein's convolution runs two such transforms of length M
around three complex products (chirp, spectrum, chirp: 3 u each); the second transform's input is the first one's output times
the chirp spectrum, whose 1-norm can reach sqrt(d) times ||x||_1 although its result cannot, so its term carries that factor:
``(1 + sqrt d) P(M) + 13``.  The four-step engine is two dense DFTs of N1 and N2 points - chains of 2 N1 and 2 N2 real
multiply-adds - and the twiddle product: ``2 N1 + 2 N2 + 7``.  Measured, the stand-in's worst case stays a factor of 7 (direct) to 160
(four-step Bluestein) below these at the length where it occurs: rounding errors do not align.

``plan`` restates the planner (``smooth_radices``, ``dft4_split``, ``plan_stockham``, ``plan_four_step`` of csrc/ssn_fft_plan.hpp and
the bounds of ``plan_dft`` in csrc/ssn_host.hip); tests/test_fft_plan.py holds the planner to it on a CPU, the GPU tests hold it to
the planner's own listing under SSN_DEBUG_PLAN for every swept length, and the stand-in is driven by it.

Wrong devices (``MUTANTS``) that each have to fail the bar on the CPU are switches of the stand-in.
"""
import functools
import re

import numpy as np

from sspslam_amd.networks.binding import transform_in, transform_out

U = 2.0 ** -24
DT = 0.001
SWEEP = tuple(range(8, 257))
# (length, needs SSN_PLAN_BLUESTEIN_FFT, SSN_DFT_NO_INPLACE, kinds)
LONG = ((512, False, False, (1, 2, 3, 4, 5)), (961, False, False, (1, 2, 3, 4, 5)), (1015, False, False, (1, 2, 3, 4, 5)),
        (1024, False, False, (1, 2, 3, 4, 5)), (1089, False, False, (1, 2, 3, 4, 5)), (2048, False, False, (1, 2, 3, 4, 5)),
        (2187, False, False, (1, 2, 3, 4, 5)), (2197, False, False, (1, 2, 3, 4, 5)), (3125, False, False, (1, 2, 3, 4, 5)),
        (1801, True, False, (1, 2, 3, 4, 5)), (1801, True, True, (1, 2, 3, 4, 5)), (2049, True, False, (1, 2, 3, 4, 5)),
        (3199, True, False, (1, 5)))
KIND_OF = {1: ("A", False), 2: ("B", False), 3: ("A", True), 4: ("B", True)}
CLASSES = ("direct", "inplace", "outofplace", "fourstep", "fourstep-bluestein")
# measure_c0(): the stand-in's worst error / (u A) per engine class over SWEEP, rounded up.  Worst cases: direct d = 225 kind 5
# (3.875), in place d = 226 kind 1 (13.464), out of place d = 237 kind 1 under SSN_DFT_NO_INPLACE (7.635), four-step d = 113 kind 5
# (one dense DFT, 11.110), four-step Bluestein d = 239 kind 1 (10.180)
C0 = {"direct": 3.9, "inplace": 13.5, "outofplace": 7.7, "fourstep": 11.2, "fourstep-bluestein": 10.2}
# measure_long(): the same for each entry of LONG on its own, key (length, SSN_DFT_NO_INPLACE)
C0_LONG = {(512, False): 3.2, (961, False): 3.6, (1015, False): 3.6, (1024, False): 2.6, (1089, False): 2.6, (2048, False): 3.8,
           (2187, False): 3.3, (2197, False): 3.1, (3125, False): 4.0, (1801, False): 15.9, (1801, True): 7.0, (2049, False): 6.6,
           (3199, False): 7.8}
C = {k: 2.0 * v for k, v in C0.items()}


# ---------------------------------------------------------------------------------------------------------------------------
# the planner, restated
class Plan:
    __slots__ = ("kind", "N", "M", "inplace", "N1", "N2", "radices")

    def __init__(self, kind, N, M=0, inplace=0, N1=0, N2=0, radices=()):
        self.kind, self.N, self.M, self.inplace, self.N1, self.N2, self.radices = kind, N, M, inplace, N1, N2, tuple(radices)

    def key(self):
        return (self.kind, self.N, self.M, self.inplace, self.N1, self.N2, self.radices)

    @property
    def cls(self):
        if self.N1:
            return "fourstep-bluestein" if self.M else "fourstep"
        return ("inplace" if self.inplace else "outofplace") if self.M else "direct"

    def __repr__(self):
        return "Plan(kind %d N %d M %d inplace %d split %dx%d radices %s)" % self.key()


@functools.lru_cache(maxsize=None)
def smooth_radices(L):
    primes, rest, twos = [], L, 0
    while rest % 2 == 0:
        twos += 1
        rest //= 2
    for p in range(3, 33):
        while rest > 1 and rest % p == 0:
            primes.append(p)
            rest //= p
    if rest != 1:
        return ()
    rad = []
    while twos >= 3 and twos != 4:
        rad.append(8)
        twos -= 3
    while twos >= 2:
        rad.append(4)
        twos -= 2
    if twos:
        rad.append(2)
    i = 0
    while i < len(primes):
        r = primes[i]
        i += 1
        while i < len(primes) and r * primes[i] <= 16:
            r *= primes[i]
            i += 1
        rad.append(r)
    return tuple(sorted(rad, reverse=True))


def stockham_cost(L):
    rad = smooth_radices(L)
    if not rad or len(rad) > 12:
        return -1.0
    return sum(1.0 if r in (2, 4, 8) else 0.25 * r + 0.5 for r in rad) * L


def dft4_cost(N1, N2, complex_in):
    P1, C1, N1p, N2p = (N1 + 15) // 16, (N2 + 15) // 16, (N1 + 3) // 4 * 4, (N2 + 3) // 4 * 4
    return P1 * C1 * ((2 if complex_in else 1) * N1p // 4) * 2 + P1 * C1 * (2 * N2p // 4) * 2


@functools.lru_cache(maxsize=None)
def dft4_split(L, complex_in):
    best, bc = (0, 0), -1
    for n1 in range(1, L + 1):
        if L % n1:
            continue
        n2 = L // n1
        if n2 > 192 or n1 > 192:
            continue
        c = dft4_cost(n1, n2, complex_in)
        if bc < 0 or c < bc:
            bc, best = c, (n1, n2)
    return best


@functools.lru_cache(maxsize=None)
def plan(d, kind=1, four_step=False, no_inplace=False):
    """What ``plan_dft`` plans for a transform of length d, or None (the matrix is kept).  The caller's rule that a Bluestein
    length M >= 2048 needs SSN_PLAN_BLUESTEIN_FFT is ``needs_flag``."""
    if d < 8 or d > 6400:
        return None
    if four_step:
        sp, M = dft4_split(d, kind == 5), 0
        if not sp[0]:
            bc = -1
            for c in range(2 * d - 1, min(6400, (2 * d - 1) + (2 * d - 1) // 8) + 1):
                s2 = dft4_split(c, True)
                if not s2[0]:
                    continue
                cost = dft4_cost(s2[0], s2[1], True)
                if bc < 0 or cost < bc:
                    bc, M, sp = cost, c, s2
        if sp[0]:
            return Plan(kind, d, M, 0, sp[0], sp[1], ())
    rad, M = smooth_radices(d), 0
    if not rad:
        best = -1.0
        for c in range(2 * d - 1, min(6400, 2 * (2 * d - 1)) + 1):
            cost = stockham_cost(c)
            if cost > 0.0 and (best < 0.0 or cost < best):
                best, M = cost, c
        if best < 0.0:
            return None
        rad = smooth_radices(M)
    if not rad or len(rad) > 12:
        return None
    inplace = int(M > 0 and not no_inplace and all(r in (2, 4, 8) for r in rad))
    return Plan(kind, d, M, inplace, 0, 0, rad)


def needs_flag(p):
    return p is not None and p.M >= 2048


def parse_listing(err):
    """The ``[ssn] dft`` lines of an SSN_DEBUG_PLAN listing -> a list of ``Plan.key()`` tuples."""
    out = []
    for m in re.finditer(r"^\[ssn\] dft kind (\d+) N (\d+) M (\d+) inplace (\d+) split (\d+)x(\d+) radices((?: \d+)*)$", err, re.M):
        g = [int(v) for v in m.groups()[:6]]
        out.append((g[0], g[1], g[2], g[3], g[4], g[5], tuple(int(v) for v in m.group(7).split())))
    return out

def assert_coverage():
    """What the sweep reaches, from the restated planner (the GPU tests hold it to the planner's listing for every length): the
    fifteen radices, both Bluestein orders, an even Bluestein length, a dense-prime four-step and a four-step Bluestein."""
    plans = [plan(d, 1) for d in SWEEP]
    assert {r for p in plans for r in p.radices} == {2, 3, 4, 5, 7, 8, 9, 11, 13, 15, 17, 19, 23, 29, 31}
    assert sum(1 for p in plans if p.cls == "direct") == 161
    assert sum(1 for p in plans if p.cls == "inplace") == 60 and {p.M for p in plans if p.cls == "inplace"} == {128, 256, 512}
    assert sum(1 for p in plans if p.cls == "outofplace") == 28
    assert {p.M for p in plans if p.cls == "outofplace"} == {80, 96, 160, 192, 320}
    assert any(p.M and p.N % 2 == 0 for p in plans) and plan(74, 1).M == 160
    assert (4, 4) == plan(16, 1).radices and 2 in plan(10, 1).radices
    assert max(len(p.radices) for p in plans) <= 6
    four = [plan(d, k, four_step=True) for d in SWEEP for k in (1, 5)]
    # (a prime length is ONE dense DFT: 1 x d for the complex input of the inverse kind, d x 1 for real input)
    assert any(p.N1 == 1 and not p.M for p in four) and any(p.N2 == 1 and not p.M for p in four) and any(p.M for p in four)
    assert plan(3199, 1).M == 6400 and plan(3200, 1).M == 0 and plan(6401, 1) is None


def pass_term(r, inplace=False):
    if r in (2, 4, 8):
        return {2: 1, 4: 2, 8: 3}[r] + 5 + (9 if inplace else 0)
    return r + 2


def analytic_c(p):
    """First-order worst case of ``error / (u A)`` for a plan (module docstring)."""
    if p.N1:
        one = 2 * p.N1 + 2 * p.N2 + 7
        return one + 4 if not p.M else (1 + np.sqrt(p.N)) * one + 13
    P = sum(pass_term(r, bool(p.inplace)) for r in p.radices)
    return P + 4 if not p.M else (1 + np.sqrt(p.N)) * P + 13


# ---------------------------------------------------------------------------------------------------------------------------
# test rows
def _f32(a):
    return np.asarray(a, dtype=np.float32)


def _impulse(n, i):
    e = np.zeros(n)
    e[i] = 1.0
    return e


@functools.lru_cache(maxsize=None)
def forward_rows(d):
    """Test vectors of a forward transform, float32 values widened to float64, read-only; the last row is zero."""
    rng = np.random.RandomState(1000 + d)
    fixed = [0, 1, 2, d // 2, d - 1]
    pos = list(range(d)) if d <= 64 else sorted(fixed + rng.choice(np.setdiff1d(np.arange(d), fixed), 4, replace=False).tolist())
    rows = [_impulse(d, n) for n in pos]
    n = np.arange(d)
    rows.append(np.ones(d))
    rows.append((-1.0) ** n)
    for b in (1, d // 2, int(rng.randint(2, max(3, d // 2)))):
        rows.append(np.cos(2 * np.pi * b * n / d))
    rows.extend(rng.randn(4, d))
    sparse = np.zeros(d)
    sparse[rng.choice(d, max(2, d // 16), replace=False)] = rng.randn(max(2, d // 16))
    rows.append(sparse)
    rows.append(rng.choice([-1.0, 1.0], d) * 2.0 ** rng.uniform(-20, 0, d))
    rows.append(np.zeros(d))
    X = _f32(np.stack(rows)).astype(np.float64)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def inverse_rows(d):
    """Test vectors of the inverse kind (4H slots), float32 values widened; the last row is zero."""
    H = d // 2 + 1
    n4 = 4 * H
    rng = np.random.RandomState(2000 + d)
    fixed = [0, 1, 2, 3, 4, n4 // 2, n4 - 4, n4 - 3, n4 - 2, n4 - 1]
    pos = list(range(n4)) if d <= 64 else sorted(fixed + rng.choice(np.setdiff1d(np.arange(n4), fixed), 4, replace=False).tolist())
    rows = [_impulse(n4, n) for n in pos]
    rows.append(np.ones(n4))
    rows.append((-1.0) ** np.arange(n4))
    for x in forward_rows(d)[-8:-1]:                  # the forward transform of real vectors, as the network's product would hold it
        rows.append(matrix(d, 1) @ x)
    rows.extend(rng.randn(4, n4))
    junk = rng.randn(3, n4)                           # junk in the imaginary slots of the purely real bins
    for j in junk:
        j[2:4] *= 1e3
        if d % 2 == 0:
            j[4 * (H - 1) + 2:4 * (H - 1) + 4] *= 1e3
    rows.extend(junk)
    only = np.zeros(n4)                               # ... and nothing but junk there
    only[2], only[3] = 3.0, -5.0
    if d % 2 == 0:
        only[4 * (H - 1) + 2], only[4 * (H - 1) + 3] = 7.0, 2.0
    rows.append(only)
    rows.append(rng.choice([-1.0, 1.0], n4) * 2.0 ** rng.uniform(-20, 0, n4))
    rows.append(np.zeros(n4))
    X = _f32(np.stack(rows)).astype(np.float64)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=64)
def matrix(d, kind):
    return transform_out(d) if kind == 5 else transform_in(d, *KIND_OF[kind])


def rows_of(d, kind):
    return inverse_rows(d) if kind == 5 else forward_rows(d)


def scale(d, kind, X):
    """A = max_k (|T| |x|)_k per row of X."""
    X = np.atleast_2d(X)
    if kind != 5:
        return np.abs(X).sum(axis=1)
    # (the reference's own error: the matrix holds sin(pi n) and its like where the exact weight is 0 - angles up to pi d^2 rounded
    #  to float64, entries scaled 2 / d: at most 2 pi d 2^-53 per entry, i.e. 2 pi d 2^-29 u ||x||_1 per output.  Without it a row
    #  with nothing but junk in the imaginary slots of the purely real bins, which the kernels clear, has a scale of 1e-16.)
    return (np.abs(X) @ np.abs(matrix(d, 5)).T).max(axis=1) + 2.0 * np.pi * d * 2.0 ** -29 * np.abs(X).sum(axis=1)


def ratios(out, ref, A):
    """Per row, the worst ``|out - ref| / (u A)`` over its elements; a row of scale 0 has to be exact (inf otherwise)."""
    err = np.abs(np.asarray(out, dtype=np.float64) - ref).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(A > 0, err / (U * A), np.where(err > 0, np.inf, 0.0))
    return r


# ---------------------------------------------------------------------------------------------------------------------------
# the model
def _table(X):
    n = len(X)
    return lambda t, X=X, n=n: X[min(max(int(round(t / DT)) - 1, 0), n - 1)]


def deal(lengths, n_models):
    """Lengths dealt round-robin: neighbours - direct, in-place and out-of-place plans alternate along the sweep - meet in one model."""
    lengths = list(lengths)
    return [tuple(lengths[i::n_models]) for i in range(n_models)]


class Case:
    """One probed transform target: the rows that arrive there, how it has to be judged."""

    def __init__(self, d, kinds, mode, p_out, index):
        self.d, self.kinds, self.mode, self.p_out, self.index = d, kinds, mode, p_out, index

    def __repr__(self):
        return "d %d kinds %s %s" % (self.d, self.kinds, self.mode)


def transform_model(lengths, kinds=(1, 2, 3, 4, 5), extras=(), tau=0.005):
    """-> (network, cases, steps).  ``extras``: lengths that also get, per direction, a target reached by TWO transforms (the second
    adds onto a non-zero destination) and one reached through a synapse (``mode='set'`` into the filter)."""
    import sspslam_amd.frontend as nengo
    cases, probes, steps = [], [], 0

    def probe(target):
        probes.append(nengo.Probe(target))
        return probes[-1], len(probes) - 1

    with nengo.Network(seed=1) as net:
        for d in lengths:
            H = d // 2 + 1
            fwd = [k for k in kinds if k != 5]
            steps = max(steps, len(forward_rows(d)) if fwd else 0, len(inverse_rows(d)) if 5 in kinds else 0)
            u = nengo.Node(_table(forward_rows(d)), size_out=d) if fwd else None
            v = nengo.Node(_table(inverse_rows(d)), size_out=4 * H) if 5 in kinds else None
            for k in fwd:
                tgt = nengo.Node(size_in=4 * H)
                nengo.Connection(u, tgt, transform=matrix(d, k), synapse=None)
                cases.append(Case(d, (k,), "plain", *probe(tgt)))
            if v is not None:
                tgt = nengo.Node(size_in=d)
                nengo.Connection(v, tgt, transform=matrix(d, 5), synapse=None)
                cases.append(Case(d, (5,), "plain", *probe(tgt)))
            if d in extras:
                u2 = nengo.Node(_table(forward_rows(d)[::-1].copy()), size_out=d)       # (the same rows, last first)
                tgt = nengo.Node(size_in=4 * H)
                nengo.Connection(u, tgt, transform=matrix(d, 1), synapse=None)
                nengo.Connection(u2, tgt, transform=matrix(d, 4), synapse=None)
                cases.append(Case(d, (1, 4), "inc", *probe(tgt)))
                tgt = nengo.Node(size_in=4 * H)
                nengo.Connection(u, tgt, transform=matrix(d, 2), synapse=tau)
                cases.append(Case(d, (2,), "filter", *probe(tgt)))
                v2 = nengo.Node(_table(inverse_rows(d)[::-1].copy()), size_out=4 * H)
                tgt = nengo.Node(size_in=d)
                nengo.Connection(v, tgt, transform=matrix(d, 5), synapse=None)
                nengo.Connection(v2, tgt, transform=matrix(d, 5), synapse=None)
                cases.append(Case(d, (5, 5), "inc", *probe(tgt)))
                tgt = nengo.Node(size_in=d)
                nengo.Connection(v, tgt, transform=matrix(d, 5), synapse=tau)
                cases.append(Case(d, (5,), "filter", *probe(tgt)))
    return net, cases, steps


def n_transforms(cases):
    return sum(len(c.kinds) for c in cases)


def case_scale(case, steps, tau=0.005):
    """The scale A of every timestep's row at a target.  Two transforms into one target: the sum of their scales (each is held to
    its own bar, and the add rounds a value no larger than that sum).  Through a synapse: the filter ``y <- a y + (1 - a) x`` is a
    convex combination, so the errors of its inputs pass through it as their scales do; its own two roundings per step are
    within 2 u of that filtered scale, which ``FILTER_EXTRA`` adds to c."""
    def padded(X):
        return np.concatenate([X, np.repeat(X[-1:], max(0, steps - len(X)), axis=0)])[:steps]
    A = np.zeros(steps)
    for i, k in enumerate(case.kinds):
        X = rows_of(case.d, k)
        if case.mode == "inc" and i == 1:
            X = X[::-1]
        A += scale(case.d, k, padded(X))
    if case.mode == "filter":
        a = np.exp(-DT / tau)
        y, out = 0.0, np.zeros(steps)
        for t in range(steps):
            y = a * y + (1 - a) * A[t]
            out[t] = y
        A = out
    return A


FILTER_EXTRA = 2.0 / (1.0 - np.exp(-DT / 0.005))     # two roundings per step, accumulated by the filter's own gain 1 / (1 - a)


def judge(cases, steps, device, oracle, c_of):
    """Every case's worst ``error / bar`` -> [(case, worst ratio of error / (u A), bar c, row of the worst)].  ``device`` and
    ``oracle`` map a case to its (steps, width) output; ``c_of(d, kind)`` gives the bar's constant."""
    out = []
    for case in cases:
        A = case_scale(case, steps)
        r = ratios(device(case), oracle(case), A)
        c = max(c_of(case.d, k) for k in case.kinds) + (FILTER_EXTRA if case.mode == "filter" else 0.0)
        out.append((case, float(r.max()), c, int(r.argmax())))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the float32 stand-in of the three engines (rows in the leading axis)
MUTANTS = ("twiddle-index", "radix8-b1-b3", "no-conj", "slot-b", "nyquist", "chirp-phase", "fb-natural", "unpadded",
           "fourstep-twiddle", "fourstep-tile", "inc-as-set", "inverse-1-over-M")


def fma(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64, the sum then rounds once more than the instruction does
    (double rounding, one case in 2^29)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def cmul(a, b):
    """cmulf of the kernels: (fma(ax, bx, -(ay by)), fma(ax, by, ay bx))."""
    return fma(a[0], b[0], -(a[1] * b[1])), fma(a[0], b[1], a[1] * b[0])


def cadd(a, b):
    return a[0] + b[0], a[1] + b[1]


def csub(a, b):
    return a[0] - b[0], a[1] - b[1]


def cmul_mi(a):
    return a[1], -a[0]


@functools.lru_cache(maxsize=32)
def twiddles(L):
    ang = -2.0 * np.pi * np.arange(L) / L
    return _f32(np.cos(ang)), _f32(np.sin(ang))


@functools.lru_cache(maxsize=32)
def chirp_tables(d, M, reduce_phase=True):
    n = np.arange(d, dtype=np.int64)
    if reduce_phase:
        ang = -np.pi * ((n * n) % (2 * d)) / d
    else:                                             # the wrong device: n^2 formed in float32, phase not reduced
        ang = (-(_f32(np.pi) / _f32(d)) * (_f32(n) * _f32(n))).astype(np.float64)
    w = np.exp(1j * ang)
    b = np.zeros(M, complex)
    b[:d] = w.conj()
    b[M - n[1:]] = w[1:].conj()
    fb = np.fft.fft(b) / M
    return (_f32(w.real), _f32(w.imag)), (_f32(fb.real), _f32(fb.imag))


def fft4(c0, c1, c2, c3):
    e0, e1, o0, o1 = cadd(c0, c2), csub(c0, c2), cadd(c1, c3), cmul_mi(csub(c1, c3))
    return cadd(e0, o0), cadd(e1, o1), csub(e0, o0), csub(e1, o1)


def fft_small(R, v, mut=()):
    if R == 2:
        return [cadd(v[0], v[1]), csub(v[0], v[1])]
    if R == 4:
        return list(fft4(*v))
    a = [cadd(v[i], v[i + 4]) for i in range(4)]
    b = [csub(v[i], v[i + 4]) for i in range(4)]
    h = np.float32(0.70710678118654752)
    b[1] = (h * (b[1][0] + b[1][1]), h * (b[1][1] - b[1][0]))
    b[2] = cmul_mi(b[2])
    b[3] = (h * (b[3][1] - b[3][0]), -h * (b[3][0] + b[3][1]))
    if "radix8-b1-b3" in mut:
        b[1], b[3] = b[3], b[1]
    a, b = fft4(*a), fft4(*b)
    return [a[0], b[0], a[1], b[1], a[2], b[2], a[3], b[3]]


def stockham(x, L, radices, mut=()):
    """dft_stockham: (re, im) arrays of shape (rows, L) -> their transform."""
    twr, twi = twiddles(L)
    xr, xi = x
    n, s = L, 1
    for st, r in enumerate(radices):
        m, fn, fr = n // r, L // n, L // r
        yr, yi = np.empty_like(xr), np.empty_like(xi)
        if r in (2, 4, 8):
            groups = L // r
            u = np.arange(groups)
            q, p = u % s, u // s
            v = fft_small(r, [(xr[:, u + k * groups], xi[:, u + k * groups]) for k in range(r)], mut)
            for j in range(r):
                out = q + s * (r * p + j)
                w = v[j] if j == 0 else cmul(v[j], (twr[p * fn * j], twi[p * fn * j]))
                yr[:, out], yi[:, out] = w
        else:
            o = np.arange(L)
            q, w = o % s, o // s
            j, p = w % r, w // r
            idx, stp, base, stride = (p * j * fn) % L, (j * fr) % L, q + s * p, s * m
            if "twiddle-index" in mut and st == 0:    # one (p, j) of the first generic pass starts one table entry late
                idx = np.where((p == min(1, m - 1)) & (j == 1), (idx + 1) % L, idx)
            ar, ai = np.zeros_like(xr), np.zeros_like(xi)
            for k in range(r):
                vr, vi, t = xr[:, base + stride * k], xi[:, base + stride * k], (idx + k * stp) % L
                ar = fma(vr, twr[t], fma(-vi, twi[t], ar))
                ai = fma(vr, twi[t], fma(vi, twr[t], ai))
            yr, yi = ar, ai
        xr, xi = yr, yi
        n, s = m, s * r
    return xr, xi


def dft_pad(a):
    return a + (a >> 3)


def pass_inplace(z, T, M, n, R, dit, padded=True):
    zr, zi = z
    sub, f = n // R, M // n
    u = np.arange(M // R)
    blk = u // sub
    i = u - blk * sub
    g = blk * n + i
    rd = [dft_pad(g + k * sub) if padded else g + k * sub for k in range(R)]
    wr = [dft_pad(g + k * sub) for k in range(R)]
    v = [(zr[:, a], zi[:, a]) for a in rd]
    w = [None, (T[0][i * f], T[1][i * f])]
    if R >= 4:
        w.append(cmul(w[1], w[1]))
        w.append(cmul(w[2], w[1]))
    if R == 8:
        w.append(cmul(w[2], w[2]))
        w.append(cmul(w[4], w[1]))
        w.append(cmul(w[3], w[3]))
        w.append(cmul(w[4], w[3]))
    if dit:
        v = [v[0]] + [cmul(v[k], w[k]) for k in range(1, R)]
    v = fft_small(R, v)
    if not dit:
        v = [v[0]] + [cmul(v[k], w[k]) for k in range(1, R)]
    zr, zi = zr.copy(), zi.copy()
    for k in range(R):
        zr[:, wr[k]], zi[:, wr[k]] = v[k]
    return zr, zi


def dif_position(k, M, rad):
    pos, ln = np.zeros_like(k), M
    for r in rad:
        ln //= r
        pos += (k % r) * ln
        k = k // r
    return pos


def load(p, X, mut=()):
    """The first loop of the bodies: rows of X -> N complex points (before the chirp)."""
    N = p.N
    H = N // 2 + 1
    X = _f32(X)
    if p.kind != 5:
        return X, np.zeros_like(X)
    i = np.arange(N)
    w = np.where(i < H, i, N - i)
    re, im = X[:, 4 * w] - X[:, 4 * w + 1], X[:, 4 * w + 2] + X[:, 4 * w + 3]
    clear = (w == 0) if "nyquist" in mut else ((w == 0) | (2 * w == N))
    im = np.where(clear, np.float32(0), im)
    return re, np.where(i < H, -im, im)


def store(p, x, dst, set_mode, mut=()):
    N = p.N
    H = N // 2 + 1
    xr, xi = x
    if p.kind != 5:
        conj, slot_b = p.kind >= 3 and "no-conj" not in mut, p.kind in (2, 4) and "slot-b" not in mut
        re, im = xr[:, :H], (-xi[:, :H] if conj else xi[:, :H])
        res = np.stack([re, im, im if slot_b else re, re if slot_b else im], axis=2).reshape(len(re), 4 * H)
    else:
        inv = np.float32(1.0) / np.float32(p.M if ("inverse-1-over-M" in mut and p.M) else N)
        res = xr[:, :N] * inv
    if set_mode or dst is None or "inc-as-set" in mut:
        return res
    return _f32(dst) + res


def dft4_fft(x, N1, N2, real_in, need_imag, n_out, mut=()):
    xr, xi = x
    rows, L = xr.shape[0], N1 * N2
    twr, twi = twiddles(L)
    xr3, xi3 = xr.reshape(rows, N1, N2), xi.reshape(rows, N1, N2)
    k1, n1 = np.arange(N1)[:, None], np.arange(N1)[None, :]
    th = 2.0 * np.pi * ((k1 * n1) % N1) / N1
    c1, s1 = _f32(np.cos(th)), _f32(np.sin(th))
    ar, ai = np.zeros((rows, N1, N2), np.float32), np.zeros((rows, N1, N2), np.float32)
    for n in range(N1):                                # K order of the MFMA chain: the real input rows, then the imaginary ones
        ar = fma(c1[None, :, n, None], xr3[:, None, n, :], ar)
        ai = fma(-s1[None, :, n, None], xr3[:, None, n, :], ai)
    if not real_in:
        for n in range(N1):
            ar = fma(s1[None, :, n, None], xi3[:, None, n, :], ar)
            ai = fma(c1[None, :, n, None], xi3[:, None, n, :], ai)
    kk1, nn2 = np.arange(N1)[:, None], np.arange(N2)[None, :]
    if "fourstep-twiddle" in mut:                      # the element's (row, column) taken as if the matrix were N2 x N1
        e = kk1 * N2 + nn2
        t = ((e // N1) * (e % N1)) % L
    else:
        t = (kk1 * nn2) % L
    br, bi = cmul((ar, ai), (twr[t][None], twi[t][None]))
    k2, n2 = np.arange(N2)[None, :], np.arange(N2)[:, None]
    ph = 2.0 * np.pi * ((k2 * n2) % N2) / N2
    c2, s2 = _f32(np.cos(ph)), _f32(np.sin(ph))         # [n2, k2]
    Xr, Xi = np.zeros((rows, N1, N2), np.float32), np.zeros((rows, N1, N2), np.float32)
    for n in range(N2):
        Xr = fma(br[:, :, n, None], c2[None, None, n, :], Xr)
        Xi = fma(br[:, :, n, None], -s2[None, None, n, :], Xi)
    for n in range(N2):
        Xr = fma(bi[:, :, n, None], s2[None, None, n, :], Xr)
        Xi = fma(bi[:, :, n, None], c2[None, None, n, :], Xi)
    Q3 = (N2 + 15) >> 4
    while Q3 > 1 and N1 * 16 * (Q3 - 1) >= n_out:
        Q3 -= 1
    if "fourstep-tile" in mut and Q3 > 1:
        Q3 -= 1
    kk = (np.arange(N1)[:, None] + N1 * np.arange(N2)[None, :])            # [k1, k2] -> output index
    keep = (kk < n_out) & (np.arange(N2)[None, :] < 16 * Q3)
    outr, outi = xr.copy(), xi.copy()                  # what is not stored keeps the input's values (the same LDS arrays)
    outr[:, kk[keep]] = Xr[:, keep]
    if need_imag:
        outi[:, kk[keep]] = Xi[:, keep]
    return outr, outi


def standin(p, X, set_mode=True, dst=None, mut=()):
    """What the kernels compute for plan ``p`` on the rows of X, in NumPy float32 -> (rows, outputs) float32."""
    N, M = p.N, p.M
    L = M or N
    xr, xi = load(p, X, mut)
    rows = xr.shape[0]
    if M:
        chirp, fb = chirp_tables(N, M, "chirp-phase" not in mut)
        ar, ai = cmul((xr, xi), chirp)
        xr, xi = np.zeros((rows, L), np.float32), np.zeros((rows, L), np.float32)
        xr[:, :N], xi[:, :N] = ar, ai
    if p.N1:
        if not M:
            fwd = p.kind != 5
            x = dft4_fft((xr, xi), p.N1, p.N2, fwd, fwd, (N // 2 + 1) if fwd else N, mut)
        else:
            vr, vi = dft4_fft((xr, xi), p.N1, p.N2, False, True, L, mut)
            yr, yi = cmul((vr, vi), fb)
            vr, vi = dft4_fft((yr, -yi), p.N1, p.N2, False, True, N, mut)
            x = cmul((vr[:, :N], -vi[:, :N]), chirp)
    elif M and p.inplace:
        tw = twiddles(M)
        zr, zi = np.zeros((rows, M + M // 8 + 1), np.float32), np.zeros((rows, M + M // 8 + 1), np.float32)
        a = dft_pad(np.arange(M))
        zr[:, a], zi[:, a] = xr, xi
        n = M
        for st, r in enumerate(p.radices):
            zr, zi = pass_inplace((zr, zi), tw, M, n, r, False, padded=not ("unpadded" in mut and st == len(p.radices) - 1))
            n //= r
        order = np.arange(M) if "fb-natural" in mut else np.argsort(dif_position(np.arange(M), M, p.radices))
        # (fb[dif_position(k)] = spectrum k: position i holds the spectrum entry whose dif_position is i)
        vr, vi = cmul((zr[:, a], zi[:, a]), (fb[0][order], fb[1][order]))
        zr[:, a], zi[:, a] = vr, -vi
        n = 1
        for r in reversed(p.radices):
            n *= r
            zr, zi = pass_inplace((zr, zi), tw, M, n, r, True)
        x = cmul((zr[:, a][:, :N], -zi[:, a][:, :N]), chirp)
    else:
        vr, vi = stockham((xr, xi), L, p.radices, mut)
        if M:
            yr, yi = cmul((vr, vi), fb)
            vr, vi = stockham((yr, -yi), L, p.radices, mut)
            x = cmul((vr[:, :N], -vi[:, :N]), chirp)
        else:
            x = (vr, vi)
    return store(p, x, dst, set_mode, mut)


def standin_ratio(p, mut=(), X=None):
    """The stand-in's worst ``error / (u A)`` over the rows of a plan's length and kind (plain store onto zero)."""
    X = rows_of(p.N, p.kind) if X is None else X
    ref = X @ matrix(p.N, p.kind).T
    return float(ratios(standin(p, X, mut=mut), ref, scale(p.N, p.kind, X)).max())


def sweep_plans(four_step=False, no_inplace=False, lengths=SWEEP, kinds=(1, 2, 3, 4, 5)):
    return [plan(d, k, four_step, no_inplace) for d in lengths for k in kinds]


def measure_c0(verbose=True):
    """The stand-in's worst ratio per engine class over SWEEP (both engines, in place and not) -> {class: (ratio, plan)}."""
    worst = {}
    for p in sweep_plans() + sweep_plans(four_step=True) + [p for p in sweep_plans(no_inplace=True) if p.M]:
        r = standin_ratio(p)
        if r > worst.get(p.cls, (0.0, None))[0]:
            worst[p.cls] = (r, p)
            if verbose:
                print("%-20s %.3f  analytic %.0f  %r" % (p.cls, r, analytic_c(p), p), flush=True)
    return worst


def measure_long():
    """The same for every entry of LONG on its own -> {(d, no_inplace): (ratio, plan)}."""
    out = {}
    for d, _, ni, kinds in LONG:
        out[(d, ni)] = max(((standin_ratio(plan(d, k, False, ni)), plan(d, k, False, ni)) for k in kinds), key=lambda v: v[0])
    return out


if __name__ == "__main__":
    for cls, (r, p) in sorted(measure_c0().items()):
        print("C0[%r] = %.3f (analytic %.0f) at %r" % (cls, r, analytic_c(p), p))
    for key, (r, p) in sorted(measure_long().items()):
        print("C0_LONG[%r] = %.3f (analytic %.0f) at %r" % (key, r, analytic_c(p), p))
