"""The instrument of the similarity-map tests (tests only): the float64 map and the bars every entry of a device map is held to.

For rows ``u`` (scaled as ``SSPSpace.decode`` scales them when ``normalize``, else raw) and a table ``S`` (n_samples x K), in float64:

* ``W = u @ S.T``        the reference map, ``A = |u| @ |S|.T`` the scale of its rounding errors;
* f64 bar       ``(K + 8) 2^-53 A``: first order, Higham's bound for a K-term product summed in any order, 8 for the normalisation;
* f32 hard cap  ``(K + 8) 2^-24 A``: the same bound, which any correct f32 chain meets;
* f32 bar       ``c REL A`` with ``REL`` of ``decoding_checks`` and ``c`` per case from ``C`` below: twice the worst ratio
                ``|chain - W| / (REL A)`` of ``f32_chain``, the CPU stand-in of what the f32 kernel computes - a k-ordered chain over
                the f32-converted operands, each product exact in float64, added and rounded to f32 once per k.  ``REL`` bare does
                not hold for a k-ordered chain (the stand-in reaches 3.8 REL A at K = 1015), so it is never used without ``c``;
                ``c REL <= (K + 8) 2^-24`` is asserted, so the bar never exceeds the cap;
* power 2       ``2 |W| b + b^2 + u W^2`` with ``b`` the power-1 bar and ``u`` the unit roundoff of the dtype (2^-24, 2^-53).

``C`` was measured with ``python tests/map_checks.py`` (a CPU; the stand-in, not a device), the larger of normalize on and off, times
two, rounded up; ``tests/test_similarity.py`` computes the ratios again and holds them to it.  Every entry of every row is checked.
"""
import functools

import numpy as np

import decoding_checks as dc

REL = dc.REL
U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}

# name -> (dim, ssp_dim asked, n per axis, T) of decoding_checks.standard_case, and how many of its rows are used
STANDARD = {
    "s144":  ((2, 97, 12, 257), 257),       # S = 144: two column tiles, the second ragged; three row tiles, the last of one row
    "s400":  ((2, 201, 20, 129), 129),      # S = 400, d as built 151: a ragged slab
    "line":  ((1, 55, 300, 64), 64),        # half a row tile
    "cube":  ((3, 97, 6, 130), 130),        # S = 216
    "fullk": ((2, 1015, 12, 40), 40),       # full K
    "t1":    ((2, 97, 12, 257), 1),
    "t128":  ((2, 97, 12, 257), 128),
}
# twice the stand-in's worst |chain - W| / (REL A), rounded up (see the module docstring); "w7" is the width-7 table of 5 samples
# measured ratios (raw, normalised): s144 1.553 1.417, s400 2.022 2.203, line 2.556 3.053, cube 1.396 1.396, fullk 3.235 3.826,
# t1 0.611 0.546, t128 1.553 1.417, w7 0.428 0.362; the hard cap is 3.3 (w7), 17.9 - 35.2 and 226.5 (fullk) REL A
C = {"s144": 3.2, "s400": 4.5, "line": 6.2, "cube": 2.8, "fullk": 7.7, "t1": 1.3, "t128": 3.2, "w7": 0.9}


@functools.lru_cache(maxsize=None)
def case(name):
    """(space or None, rows, table, points) of a named case.  Standard cases: the rows of ``decoding_checks.standard_case`` (every
    7th scaled by 3.7) with, from 3 rows on, row 1 all zero and row 2 scaled to norm 1e-7.  Shared: read-only."""
    if name == "w7":
        rng = np.random.RandomState(7)
        space, rows, table, points = None, rng.randn(9, 7), rng.randn(5, 7), rng.uniform(-1, 1, (5, 2))
        rows[3] = 0.0
    else:
        key, T = STANDARD[name]
        space, rows, table, points = dc.standard_case(*key)
        rows = np.array(rows[:T])
        if T >= 3:
            rows[1] = 0.0
            rows[2] *= 1e-7 / np.linalg.norm(rows[2])
    rows.setflags(write=False)
    return space, rows, table, points


def scaled(rows, normalize):
    return dc.scale_rows(rows) if normalize else np.atleast_2d(np.asarray(rows, dtype=np.float64))


class MapReference:
    """W, A and the bars for one (table, rows, normalize); ``c`` is the case's factor of the f32 bar."""

    def __init__(self, table, rows, normalize, c):
        self.table = np.asarray(table, dtype=np.float64)
        self.u = scaled(rows, normalize)
        self.K = self.table.shape[1]
        self.c = float(c)
        assert self.c * REL <= (self.K + 8) * 2.0 ** -24, (self.c, self.K)        # the bar stays below the hard cap
        self.W = self.u @ self.table.T
        self.A = np.abs(self.u) @ np.abs(self.table).T

    def want(self, power):
        return self.W if power == 1 else self.W ** 2

    def _squared(self, b, dtype):
        return 2 * np.abs(self.W) * b + b * b + U[dtype] * self.W ** 2

    def bar(self, dtype, power=1, cap=False):
        if dtype == "f64":
            b = (self.K + 8) * 2.0 ** -53 * self.A
        else:
            b = ((self.K + 8) * 2.0 ** -24 if cap else self.c * REL) * self.A
        return b if power == 1 else self._squared(b, dtype)

    def ok(self, got, dtype, power=1, cap=False):
        """Per entry: within the bar (``cap``: within the f32 hard cap).  NaN or a wrong shape fails."""
        got = np.asarray(got, dtype=np.float64)
        if got.shape != self.W.shape:
            return np.zeros(self.W.shape, dtype=bool)
        return np.abs(got - self.want(power)) <= self.bar(dtype, power, cap)

    def worst(self, got, dtype, power=1):
        """Largest error / bar over the entries whose bar is not zero (an entry with a zero bar must be exact: ``ok``)."""
        err, bar = np.abs(np.asarray(got, dtype=np.float64) - self.want(power)), self.bar(dtype, power)
        return float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), 0.0)))

    def chain_ratio(self, chain):
        """|chain - W| / (REL A) at its worst: what ``C`` holds twice of."""
        err = np.abs(np.asarray(chain, dtype=np.float64) - self.W)
        return float(np.max(np.where(self.A > 0, err / np.where(self.A > 0, REL * self.A, 1.0), 0.0)))


def round_mantissa(x, bits):
    """x rounded to ``bits`` explicit mantissa bits (10: what a half-precision operand would keep)."""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(np.round(m * 2.0 ** (bits + 1)) / 2.0 ** (bits + 1), e)


def f32_chain(table, rows, normalize, power=1, mantissa=None, slabs=None):
    """The CPU stand-in of the f32 map kernel: operands scaled in float64 and converted to f32 (``mantissa``: rounded to that many
    bits instead - a wrong device), then per entry acc = f32(acc + a_k b_k) for k ascending, the product exact in float64; the
    square is one f32 multiply.  ``slabs``: only that many 32-wide K slabs are added (a wrong device that drops the last one)."""
    u = scaled(rows, normalize).astype(np.float32)
    tab = np.asarray(table, dtype=np.float64).astype(np.float32)
    if mantissa is not None:
        u, tab = round_mantissa(u, mantissa).astype(np.float32), round_mantissa(tab, mantissa).astype(np.float32)
    K = tab.shape[1] if slabs is None else min(tab.shape[1], 32 * slabs)
    acc = np.zeros((u.shape[0], tab.shape[0]), dtype=np.float32)
    for k in range(K):
        acc = (acc.astype(np.float64) + np.outer(u[:, k].astype(np.float64), tab[:, k].astype(np.float64))).astype(np.float32)
    return acc * acc if power == 2 else acc


def padding_ok(parent, T, S, sentinel):
    """A map written into ``parent[:T, :S]``: everything else of ``parent`` still holds the sentinel."""
    parent = np.asarray(parent)
    return bool(np.all(parent[:, S:] == sentinel) and np.all(parent[T:] == sentinel))


if __name__ == "__main__":          # the measurement behind C
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for name in C:
        _, rows, table, _ = case(name)
        ratios = [MapReference(table, rows, nz, 0.0).chain_ratio(f32_chain(table, rows, nz)) for nz in (False, True)]
        K = table.shape[1]
        print("%-6s K %4d: worst ratio raw %.3f, normalised %.3f -> c >= %.3f; cap / REL = %.1f" % (
            name, K, ratios[0], ratios[1], 2 * max(ratios), (K + 8) * 2.0 ** -24 / REL))
