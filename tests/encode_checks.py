"""The instrument of the encoder tests (tests only): the float64 host answer and the bars a device encode is held to.

The reference is ``SSPSpace.encode`` in float64 (golden-tested against the reference project's output in
``tests/golden/ssp_spaces.npz``).  With ``(K, M, w) = space.refine_tables()``, ``th = x @ M.T`` and, built here in float64
independently of the package,

    P = [cos th_0, sin th_0, cos th_1, ...]   (N x 2K)        B[2k] = w_k cos(2 pi k c / d),  B[2k + 1] = -w_k sin(2 pi k c / d)   (2K x d)

an encode is ``P @ B``.  Per entry ``S_c = sum_j |P_j B_jc|`` in float64, and

* ``f64``       ``(2K + 8) 2^-53 S_c``: the first-order bound of an ordered sum of 2K products plus the rounding of sincos and of
                the table.
* ``f32``       ``C * REL * S_c`` with ``REL`` of ``decoding_checks`` (the f32 matrix-core product against fp64 at K <= 1024 plus
                the rounding of both operands).  ``C`` is not chosen freely: ``C0`` is the worst ``error / (REL S_c)`` of the CPU
                stand-in below (P and B rounded to f32, a sequential f32 chain over the 2K columns) over every row of every case
                of ``CASES`` and the far case; ``C = 2 C0``, the margin of 2 for the summation order inside a 32-wide K slab,
                which the stand-in does not reproduce.  Entries near the encoded point are sums of same-sign products, which is
                why C0 exceeds 1 (DESIGN.md 3.11 records the same for similarities).  ``measure_c0()`` recomputes it and
                ``tests/test_encode.py`` holds the constant to that; the device never enters.
* ``f32-format`` ``(2K + 8) 2^-24 S_c``: the f64 bound with the f32 unit roundoff, which an ordered f32 chain cannot exceed to first
                order.  For ``special_points`` only (see there).
* far case, f64 the f64 bar plus ``phase_term``: at |th| near 1000 the reference's own rounding of th exceeds the f64 bar (the float64
                stand-in misses it by 1.8 there), which is the reference's error and not a device's.

Wrong encoders (``MUTANTS``) that each have to fail on the CPU are at the end.
"""
import functools

import numpy as np

import decoding_checks as dc
import refine_checks as rc

REL = dc.REL
C0 = 1.65                # measure_c0() gives 1.645 (worst case: d = 1015); rounded up
C = 2 * C0

NS = (1, 63, 64, 65, 130)
# name -> how the space is made; every one has 130 points inside its bounds
CASES = ("d3-1d", "d97-2d", "d127-2d", "d129-2d", "d201-3d", "d64-full", "d1015-2d")
FAR = "far"              # |x| <= 50 at length scale 0.2 on the explicit d = 97 space: |th| reaches 1000 rad and more


@functools.lru_cache(maxsize=None)
def case_space(name):
    from sspslam_amd import harness as H
    if name == "d3-1d":
        return rc.explicit_space("sym", 1, 3)
    if name == "d97-2d":
        return H.make_ssp_space(2, ssp_dim=97)
    if name == "d127-2d":
        return rc.explicit_space("sym", 2, 127)
    if name == "d129-2d":
        return rc.explicit_space("sym", 2, 129)
    if name == "d201-3d":
        return H.make_ssp_space(3, ssp_dim=201, rng=np.random.RandomState(0))
    if name == "d64-full":
        return rc.explicit_space("full", 2, 64)
    if name == "d1015-2d":
        return H.make_ssp_space(2, ssp_dim=1015)
    if name == FAR:
        return rc.explicit_space("sym", 2, 97)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case_points(name):
    """130 points of the case (65 for the far case), read-only."""
    space = case_space(name)
    rng = np.random.RandomState(11)
    if name == FAR:
        x = rng.uniform(-50.0, 50.0, (65, space.domain_dim))
    else:
        b = space.domain_bounds
        x = rng.uniform(b[:, 0], b[:, 1], (130, space.domain_dim))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def special_points(name):
    """The origin (encode(0) is the identity: every cosine 1, entry 0 a sum of 2K equal-signed, nearly equal terms), two corners of
    the domain and a point on one face.  Held to the ``f32-format`` bar in f32: adding one constant again and again rounds the same way
    every time, so the f32 chain drifts systematically there (22 REL S_c at d = 1015 in the stand-in) and says nothing about C."""
    b = case_space(name).domain_bounds
    x = np.stack([np.zeros(b.shape[0]), b[:, 0], b[:, 1], np.where(np.arange(b.shape[0]) == 0, b[:, 1], 0.25 * b[:, 1])])
    x.setflags(write=False)
    return x


def factors(space, x):
    """(P, B, K) in float64."""
    K, M, w = space.refine_tables()
    d = space.ssp_dim
    th = np.atleast_2d(np.asarray(x, dtype=np.float64)) @ M.T
    P = np.empty((th.shape[0], 2 * K))
    P[:, 0::2], P[:, 1::2] = np.cos(th), np.sin(th)
    ang = 2.0 * np.pi * ((np.arange(K)[:, None] * np.arange(d)[None, :]) % d) / d
    B = np.empty((2 * K, d))
    B[0::2], B[1::2] = w[:, None] * np.cos(ang), -w[:, None] * np.sin(ang)
    return P, B, K


class Reference:
    def __init__(self, space, x):
        self.space = space
        self.x = np.atleast_2d(np.asarray(x, dtype=np.float64))
        self.want = space.encode(self.x)
        P, B, K = factors(space, self.x)
        self.K = K
        self.S = np.abs(P) @ np.abs(B)

    def bar(self, mode, rows=slice(None)):
        S = self.S[rows]
        if mode == "f64":
            return (2 * self.K + 8) * 2.0 ** -53 * S
        if mode == "f32-format":
            return (2 * self.K + 8) * 2.0 ** -24 * S
        return C * REL * S

    def phase_term(self, rows=slice(None)):
        """What the rounding of the phases themselves may move an entry by, first order: the reference and the device each evaluate
        ``th_k`` with dim products and dim - 1 sums, each within ``(dim + 1) 2^-53 |th_k|``; d cos = |sin| d th, d sin = |cos| d th.
        Only the far case needs it (it is 2e-16 of an entry at |th| = 1, 2e-13 at |th| = 1000), and only in f64."""
        K, M, w = self.space.refine_tables()
        d = self.space.ssp_dim
        th = self.x[rows] @ M.T
        dth = 2 * (self.space.domain_dim + 1) * 2.0 ** -53 * np.abs(th)
        dP = np.empty((th.shape[0], 2 * K))
        dP[:, 0::2], dP[:, 1::2] = np.abs(np.sin(th)) * dth, np.abs(np.cos(th)) * dth
        return dP @ np.abs(factors(self.space, self.x[:1])[1])

    def ratio(self, got, mode, rows=slice(None), phases=False):
        """|got - want| / bar per entry, for the rows ``rows`` of the reference (``phases``: the bar plus ``phase_term``)."""
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == self.want[rows].shape, (got.shape, self.want[rows].shape)
        bar = self.bar(mode, rows) + (self.phase_term(rows) if phases else 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.abs(got - self.want[rows]) / bar
        return np.where(np.isfinite(r), r, np.inf)

    def check(self, got, mode, rows=slice(None), label="", phases=False):
        """Every entry of every row under its bar; prints and returns the worst ratio."""
        r = self.ratio(got, mode, rows, phases)
        worst = float(r.max()) if r.size else 0.0
        print(f"{label} {mode}: {r.shape[0]} rows x {r.shape[1]}, worst |error| / bar = {worst:.3f}")
        assert worst <= 1.0, (label, mode, worst, np.argwhere(r > 1.0)[:4])
        return worst


@functools.lru_cache(maxsize=None)
def reference(name):
    return Reference(case_space(name), case_points(name))


@functools.lru_cache(maxsize=None)
def special_reference(name):
    return Reference(case_space(name), special_points(name))


# -- stand-ins: what the kernels compute, with NumPy ---------------------------------------------------------------------------
def f64_stand_in(space, x):
    """An ordered float64 sum over the 2K columns."""
    P, B, K = factors(space, x)
    acc = np.zeros((P.shape[0], B.shape[1]))
    for j in range(2 * K):
        acc = acc + P[:, j:j + 1] * B[j][None, :]
    return acc


def f32_stand_in(space, x, f32_phases=False):
    """P and B rounded to f32 and a sequential f32 chain over the 2K columns.  ``f32_phases``: the wrong encoder whose phases (and the
    points and phase matrix they come from) are f32 as well."""
    P, B, K = factors(space, x)
    if f32_phases:
        _, M, _ = space.refine_tables()
        x32, M32 = np.atleast_2d(np.asarray(x)).astype(np.float32), M.astype(np.float32)
        th = np.zeros((x32.shape[0], K), dtype=np.float32)
        for a in range(x32.shape[1]):
            th = th + x32[:, a:a + 1] * M32[None, :, a]
        th = th.astype(np.float64)               # the sincos itself exact: only the phase is f32
        P[:, 0::2], P[:, 1::2] = np.cos(th), np.sin(th)
    P32, B32 = P.astype(np.float32), B.astype(np.float32)
    acc = np.zeros((P.shape[0], B.shape[1]), dtype=np.float32)
    for j in range(2 * K):
        acc = acc + P32[:, j:j + 1] * B32[j][None, :]
    return acc.astype(np.float64)


def measure_c0():
    """Worst error / (REL S_c) of the f32 stand-in over every row of every case: (c0, {case: worst})."""
    per = {}
    for name in CASES + (FAR,):
        ref = reference(name)
        per[name] = float(np.max(np.abs(f32_stand_in(ref.space, ref.x) - ref.want) / (REL * ref.S)))
    return max(per.values()), per


# -- wrong encoders -------------------------------------------------------------------------------------------------------------
def _mutant(space, x, w0=1.0, sine=1.0, swap=False, no_scale=False, drop0=False, shift=0, drop_last=False):
    K, M, w = space.refine_tables()
    d = space.ssp_dim
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    if swap:
        x = x[:, ::-1]
    if no_scale:
        M = np.asarray(space.phase_matrix, dtype=np.float64)[:K]
    w = w.copy()
    w[0] *= w0
    if drop0:
        w[0] = 0.0
    if drop_last:
        w[K - 1] = 0.0
    th = x @ M.T
    ang = 2.0 * np.pi * np.outer(np.arange(K), np.arange(d) + shift) / d
    return (np.cos(th) * w[None, :]) @ np.cos(ang) - sine * (np.sin(th) * w[None, :]) @ np.sin(ang)


MUTANTS = {
    "w0 doubled": lambda s, x: _mutant(s, x, w0=2.0),
    "sign of the sine term": lambda s, x: _mutant(s, x, sine=-1.0),
    "two axes swapped": lambda s, x: _mutant(s, x, swap=True),
    "length scale ignored": lambda s, x: _mutant(s, x, no_scale=True),
    "bin 0 dropped": lambda s, x: _mutant(s, x, drop0=True),
    "c shifted by one": lambda s, x: _mutant(s, x, shift=1),
    "last K bin left out": lambda s, x: _mutant(s, x, drop_last=True),
}
