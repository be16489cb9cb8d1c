"""The instrument of the binding tests (tests only): ``SSPBinder`` / ``ssn_binder_*`` against the direct circular sum.

Reference.  ``direct(a, b)[j] = sum_i a_i b_{(j - i) mod d}`` in float64 as ``np.convolve(a, [b, b])[d:2d]`` - a plain sum, no FFT -
and ``direct(|a|, |b|)`` for the entry-wise scale.  Every test value is made as float32 and widened, so an f32 binder sees exactly
what the reference sees, from host float64, host float32 and device tensors alike.

Bars.  With ``u32 = 2^-24``, ``u64 = 2^-53``:
  * f32 (``k_bind_rows``): every entry of a row within ``c u32 |a|_2 |b|_2``.  An FFT's error is normwise: the bar has no entry-wise
    form.  A row with ``a = 0`` or ``b = 0`` has to be exactly zero.
  * f64 (``k_bind_direct``): entry j within ``(d + 8) u64 sum_i |a_i| |b_{(j - i) mod d}|`` - a chain of d fused multiply-adds.
  * normalised rows ``c / N``, ``N = max(|c|_2, floor)``: first order, ``bar_j / N + |c_j| |bar|_2 / N^2 + 4 u |c_j| / N`` (the second
    term only where ``|c|_2 >= floor``: below it N is a constant), u the binder's unit roundoff.

The constant c is not chosen freely: ``C0[route]`` is the worst ratio ``error / (u32 |a| |b|)`` that the NumPy float32 stand-in below
(``standin``: ``dft_checks.stockham`` / ``twiddles`` / ``chirp_tables`` around the kernel's packing, balancing and separation, in the
kernel's order) reaches over ``pairs(d)`` of every length in ``LENGTHS`` (``measure_c0()`` recomputes it; ``tests/test_bind.py`` holds
every length to half a bar), and ``C = 2 C0`` - the margin is for what the stand-in does not reproduce: which products the compiler
contracts, and the summation order of the float64 norms, which can move the balancing exponent by one at a boundary.

First-order worst case (``analytic_c``), which C has to stay below.  One output of a forward transform is within ``P u |z|_1`` of
exact, ``P = P(route)`` the pass sum of ``dft_checks.analytic_c`` (Bluestein: ``(1 + sqrt M') ...`` as there).  With the rows balanced,
``|z|_2 <= sqrt 3 min(|a|, s |b|)``, so ``|z|_1 <= sqrt(3 d) min(...)``; the separated spectra A and sB inherit that error, their
product's error summed over the d bins and divided by d is at most ``sqrt(3 d) P u |a| |b|`` for either factor (``|A|_1 <= d |a|_2``),
and the transform back adds ``P u |C|_1 / d <= P u |a| |b|``:  ``c <= (2 sqrt(3 d) + 1) P + 8`` (8: the packing, the separation's four
sums and product, 1 / d).  Measured, the stand-in stays two to three orders of magnitude below it: rounding errors do not align.

What the stand-in showed about balancing: without it (``no-balance``) a pair with ``|b| = 2^-20 |a|`` misses the bar by a factor of 1.6e4 to 3.5e4 (d = 55, 151, 1015), because the
separation ``(Z_k - conj Z_{d-k}) / 2i`` subtracts numbers of size ``|A_k|`` to get ``|B_k|``; with ``s = 2^e`` from the two sums of
squares every pair of ``pairs(d)`` - ratios 2^+-20 included - stays at the ratio dense pairs have.  The packed form is kept.

``plan`` restates the binder's planner (``plan_stockham`` of csrc/ssn_fft_plan.hpp with the in-place engine forbidden, from d = 2, as
``ssn_binder_create`` of csrc/ssn_bind.hip calls it); wrong binders (``MUTANTS``) are switches of the stand-in.
"""
import functools

import numpy as np

import dft_checks as dc

U32, U64 = 2.0 ** -24, 2.0 ** -53
LENGTHS = (2, 3, 8, 12, 16, 55, 58, 97, 151, 256, 257, 1015, 1024, 1801, 3751, 6400)
LONG = 1801          # from here on a handful of rows
# measure_c0(): the stand-in's worst error / (u32 |a| |b|) per route over pairs(d), d in LENGTHS, rounded up.
# Worst cases: direct d = 3751 (7.644; 5.044 at d = 1015, at most 3.9 below d = 1015); Bluestein d = 1801 (6.823; 6.781 at d = 151)
C0 = {"direct": 7.7, "bluestein": 6.9}
C = {k: 2.0 * v for k, v in C0.items()}
MUTANTS = ("mirror", "no-1-over-d", "no-conj-back", "nyquist-complex", "invert-index", "pairing-mod", "no-balance", "floor-ignored",
           "chirp-phase")


# ---------------------------------------------------------------------------------------------------------------------------
# the planner, restated
class Route:
    __slots__ = ("d", "M", "radices")

    def __init__(self, d, M, radices):
        self.d, self.M, self.radices = d, M, tuple(radices)

    @property
    def L(self):
        return self.M or self.d

    @property
    def cls(self):
        return "bluestein" if self.M else "direct"

    @property
    def threads(self):
        return min(1024, max(64, ((self.L + 3) // 4 + 63) // 64 * 64))

    def key(self):
        return (self.d, self.M, self.radices)

    def __repr__(self):
        return "Route(d %d M %d radices %s)" % self.key()


@functools.lru_cache(maxsize=None)
def plan(d):
    """What ``ssn_binder_create`` plans for an f32 binder of width d, or None (SSN_EUNSUPPORTED)."""
    if d < 2 or d > 6400:
        return None
    rad, M = dc.smooth_radices(d), 0
    if not rad:
        best = -1.0
        for c in range(2 * d - 1, min(6400, 2 * (2 * d - 1)) + 1):
            cost = dc.stockham_cost(c)
            if cost > 0.0 and (best < 0.0 or cost < best):
                best, M = cost, c
        if best < 0.0:
            return None
        rad = dc.smooth_radices(M)
    if not rad or len(rad) > 12:
        return None
    return Route(d, M, rad)


def analytic_c(route):
    P = sum(dc.pass_term(r) for r in route.radices)
    if route.M:
        P = (1 + np.sqrt(route.d)) * P + 13
    return (2.0 * np.sqrt(3.0 * route.d) + 1.0) * P + 8.0


# ---------------------------------------------------------------------------------------------------------------------------
# test rows
def _f32(a):
    return np.asarray(a, dtype=np.float32)


N_SPECIAL = 14


@functools.lru_cache(maxsize=None)
def pairs(d, n=None):
    """(A, B): n row pairs of width d, float32 values widened, read-only.  The first N_SPECIAL: dense x dense, |b| = 2^-20 |a|,
    identity x dense, |a| = 2^-20 |b|, a shifted impulse, ones x dense, ones x ones, alternating signs x dense, alternating x
    alternating, wide-range x wide-range, wide-range x dense, zero x dense, dense x zero, a sparse pair; dense pairs after that."""
    n = N_SPECIAL if n is None else n
    rng = np.random.RandomState(3000 + d)
    dense = lambda: rng.randn(d)
    wide = lambda: rng.choice([-1.0, 1.0], d) * 2.0 ** rng.uniform(-20, 0, d)
    imp = lambda i: np.eye(d)[i % d]
    alt = (-1.0) ** np.arange(d)
    sparse = np.zeros(d)
    sparse[rng.choice(d, max(1, d // 16), replace=False)] = rng.randn(max(1, d // 16))
    rows = [(dense(), dense()), (dense(), dense() * 2.0 ** -20), (imp(0), dense()), (dense() * 2.0 ** -20, dense()), (imp(d // 3 + 1), dense()),
            (np.ones(d), dense()), (np.ones(d), np.ones(d)), (alt, dense()), (alt, alt), (wide(), wide()), (wide(), dense()),
            (np.zeros(d), dense()), (dense(), np.zeros(d)), (sparse, dense())]
    assert len(rows) == N_SPECIAL
    while len(rows) < n:
        rows.append((dense(), dense() * 2.0 ** rng.randint(-3, 4)))
    A = _f32(np.stack([r[0] for r in rows[:n]])).astype(np.float64)
    B = _f32(np.stack([r[1] for r in rows[:n]])).astype(np.float64)
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


def n_rows(d):
    return N_SPECIAL if d >= LONG else 257


# ---------------------------------------------------------------------------------------------------------------------------
# the reference and the bars
def invert(a):
    a = np.atleast_2d(a)
    return a[:, (-np.arange(a.shape[1])) % a.shape[1]]


def pair_index(n, count, mut=()):
    """Operand row of every output row: r // (n / count); the wrong binder takes r % count."""
    r = np.arange(n)
    return r % count if "pairing-mod" in mut else r // (n // count)


def direct(A, B):
    """Row-wise circular convolution as a plain float64 sum (no transform)."""
    A, B = np.atleast_2d(A), np.atleast_2d(B)
    d = A.shape[1]
    return np.stack([np.convolve(a, np.concatenate([b, b]))[d:2 * d] for a, b in zip(A, B)])


def norms(A, B):
    return np.linalg.norm(A, axis=1) * np.linalg.norm(B, axis=1)


def bar32(A, B, c):
    """(n, 1): the f32 bar of every entry of a row."""
    return (c * U32 * norms(A, B))[:, None]


def bar64(A, B):
    d = np.atleast_2d(A).shape[1]
    return (d + 8) * U64 * direct(np.abs(A), np.abs(B))


def normalized(ref, floor):
    return ref / np.maximum(np.linalg.norm(ref, axis=1, keepdims=True), floor)


def bar_normalized(ref, bar, floor, u):
    """First-order propagation of an entry-wise bar through ``c / max(|c|, floor)``, plus 4 u of the quotient."""
    bar = np.broadcast_to(bar, ref.shape)
    nrm = np.linalg.norm(ref, axis=1, keepdims=True)
    N = np.maximum(nrm, floor)
    moving = np.where(nrm >= floor, np.abs(ref) * np.linalg.norm(bar, axis=1, keepdims=True) / N ** 2, 0.0)
    return bar / N + moving + 4.0 * u * np.abs(ref) / N


def worst(out, ref, bar):
    """Worst ``|out - ref| / bar`` over all entries; an entry whose bar is 0 has to be exact (inf otherwise)."""
    err = np.abs(np.asarray(out, dtype=np.float64) - ref)
    bar = np.broadcast_to(bar, err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# the float32 stand-in of k_bind_rows (rows in the leading axis)
def _fft_d(route, x, mut=()):
    d, M = route.d, route.M
    if not M:
        return dc.stockham(x, d, route.radices)
    chirp, fb = dc.chirp_tables(d, M, "chirp-phase" not in mut)
    rows = x[0].shape[0]
    ar, ai = dc.cmul(x, chirp)
    xr, xi = np.zeros((rows, M), np.float32), np.zeros((rows, M), np.float32)
    xr[:, :d], xi[:, :d] = ar, ai
    vr, vi = dc.stockham((xr, xi), M, route.radices)
    yr, yi = dc.cmul((vr, vi), fb)
    vr, vi = dc.stockham((yr, -yi), M, route.radices)
    return dc.cmul((vr[:, :d], -vi[:, :d]), chirp)


def standin(route, A, B, invert_a=False, invert_b=False, normalize=False, floor=1e-8, mut=()):
    """What k_bind_rows computes for the paired rows (A[r], B[r]), in NumPy float32 -> (rows, d) float32."""
    d = route.d
    A, B = _f32(np.atleast_2d(A)), _f32(np.atleast_2d(B))
    gather = (d - 1 - np.arange(d)) if "invert-index" in mut else (-np.arange(d)) % d
    if invert_a:
        A = A[:, gather]
    if invert_b:
        B = B[:, gather]
    sa, sb = np.sum(A.astype(np.float64) ** 2, axis=1), np.sum(B.astype(np.float64) ** 2, axis=1)
    zero = (sa == 0.0) | (sb == 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.frexp(np.where(zero, 1.0, sa / np.where(zero, 1.0, sb)))[1]          # ilogb + 1
    e = np.clip((t - (t & 1)) // 2, -100, 100)
    if "no-balance" in mut:
        e = np.zeros_like(e)
    s = _f32(2.0 ** e)[:, None]
    zr, zi = _fft_d(route, (A, B * s), mut)
    k = np.arange(d)
    m = (d - k - 1) % d if "mirror" in mut else (d - k) % d
    xk, yk, xm, ym = zr, zi, zr[:, m], zi[:, m]
    real_bin = (k == 0) | (2 * k == d)
    if "nyquist-complex" in mut:                       # the Nyquist bin without its mirror term
        nyq = (2 * k == d)
        xm, ym = np.where(nyq, np.float32(0), xm), np.where(nyq, np.float32(0), ym)
        real_bin = k == 0
    ar, ai, br, bi = xk + xm, yk - ym, yk + ym, xm - xk
    cr = np.float32(0.25) * dc.fma(ar, br, -(ai * bi))
    ci = np.float32(-0.25) * dc.fma(ar, bi, ai * br)
    if "no-conj-back" in mut:
        ci = -ci
    cr = np.where(real_bin, xk * yk, cr)
    ci = np.where(real_bin, np.float32(0), ci)
    vr, _ = _fft_d(route, (cr, ci), mut)
    inv_d = np.float32(1.0) if "no-1-over-d" in mut else np.float32(1.0) / np.float32(d)
    v = (vr * inv_d) * _f32(2.0 ** -e)[:, None]
    v = np.where(zero[:, None], np.float32(0), v)
    if normalize:
        nrm = np.sqrt(np.sum(v.astype(np.float64) ** 2, axis=1, keepdims=True))
        if "floor-ignored" not in mut:
            nrm = np.maximum(nrm, floor)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = _f32(v.astype(np.float64) / nrm)
    return v


def standin_ratio(route, A, B, mut=()):
    """The stand-in's worst ``error / (u32 |a| |b|)`` over the pairs (bar constant 1)."""
    return worst(standin(route, A, B, mut=mut), direct(A, B), bar32(A, B, 1.0))


def measure_c0(verbose=True):
    out = {}
    for d in LENGTHS:
        route = plan(d)
        r = standin_ratio(route, *pairs(d, n_rows(d)))
        if verbose:
            print("d %5d %-9s %.3f  analytic %.0f  %r" % (d, route.cls, r, analytic_c(route), route), flush=True)
        if r > out.get(route.cls, (0.0, None))[0]:
            out[route.cls] = (r, route)
    return out


if __name__ == "__main__":
    for cls, (r, route) in sorted(measure_c0().items()):
        print("C0[%r] = %.3f (analytic %.0f) at %r" % (cls, r, analytic_c(route), route))
