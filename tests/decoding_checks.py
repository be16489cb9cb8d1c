"""The instrument of the grid-decoder tests (tests only): the float64 host answer and the bars a device answer is held to.

For rows ``u`` scaled as ``SSPSpace.decode`` scales them and a table ``S`` (n_samples x d), everything in float64:

* ``jstar``   ``np.argmax(S @ u)`` per row (the first copy, should the table hold the best row twice);
* ``gap``     best minus second-best similarity per row;
* ``bar``     ``B = 2 * (1.5e-7 + 2 * 2**-24) * max_j sum_k |u_k S_jk|``: 1.5e-7 is the error of an f32 matrix-core product against
              fp64 at K <= 1024 relative to sum |a b|, 2 * 2**-24 the rounding of both operands to f32, the factor 2 because two
              similarities are compared.

A device index ``j`` passes when it is a real column, ``s[jstar] - s[j] <= B``, and it is the first copy of its table row
(identical rows see the same fmaf chain, so their f32 similarities tie exactly and the lowest column has to win).  A device
similarity passes within ``B / 2`` of ``s[j]``.  f64 indices must equal ``jstar`` wherever the gap exceeds 1e-12.
"""
import functools

import numpy as np

REL = 1.5e-7 + 2 * 2.0 ** -24


def scale_rows(rows):
    """The scaling of SSPSpace.decode: divided by the norm unless it is below 1e-6."""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    nrm = np.linalg.norm(rows, axis=1, keepdims=True)
    return np.where(nrm < 1e-6, rows, rows / np.where(nrm == 0, 1.0, nrm))


class Reference:
    def __init__(self, table, rows):
        self.table = np.asarray(table, dtype=np.float64)
        self.unit = scale_rows(rows)
        self.n_samples = self.table.shape[0]
        self.sims = self.unit @ self.table.T                                   # (T, n_samples)
        _, first, inverse = np.unique(self.table, axis=0, return_index=True, return_inverse=True)
        self.first_copy = first[np.asarray(inverse).reshape(-1)]              # lowest index of an identical table row
        self.jstar = self.first_copy[np.argmax(self.sims, axis=1)]
        t = np.arange(self.sims.shape[0])
        self.top = self.sims[t, self.jstar]
        if self.n_samples > 1:
            rest = self.sims.copy()
            rest[:, self.first_copy != np.arange(self.n_samples)] = -np.inf   # later copies are no second candidates
            rest[t, self.jstar] = -np.inf
            self.gap = self.top - rest.max(axis=1)
        else:
            self.gap = np.full(t.shape, np.inf)
        self.bar = 2 * REL * (np.abs(self.unit) @ np.abs(self.table).T).max(axis=1)

    def guard(self):
        """The inputs separate the best sample from the second by more than the bar: equality with jstar may be demanded."""
        return bool(np.all(self.gap > self.bar))

    def index_ok(self, idx):
        idx = np.asarray(idx).astype(np.int64).reshape(-1)
        real = (idx >= 0) & (idx < self.n_samples)
        j = np.where(real, idx, 0)
        t = np.arange(idx.shape[0])
        return real & (self.top - self.sims[t, j] <= self.bar) & (self.first_copy[j] == j)

    def sims_ok(self, idx, sims):
        idx = np.asarray(idx).astype(np.int64).reshape(-1)
        t = np.arange(idx.shape[0])
        return np.abs(np.asarray(sims, dtype=np.float64).reshape(-1) - self.sims[t, idx]) <= self.bar / 2

    def f64_ok(self, idx):
        idx = np.asarray(idx).astype(np.int64).reshape(-1)
        return (idx == self.jstar) | ((self.gap <= 1e-12) & self.index_ok(idx))


def f32_stand_in(table, rows, chain_sims=False):
    """What the f32 decoder computes, with NumPy: (indices, similarities).  The indices come from an f32 product; the similarity
    of the winner is, as in the decoder, accumulated again in float64 over the f32 operands (``chain_sims``: the f32 product's own
    value instead)."""
    u, tab = scale_rows(rows).astype(np.float32), np.asarray(table, dtype=np.float32)
    s = u @ tab.T
    idx = np.argmax(s, axis=1)
    if chain_sims:
        return idx, s[np.arange(s.shape[0]), idx].astype(np.float64)
    return idx, np.sum(u.astype(np.float64) * tab[idx].astype(np.float64), axis=1)


@functools.lru_cache(maxsize=None)
def standard_case(dim, ssp_dim, n_per_axis, T):
    """(space, rows, table, points) of a standard case: a noisy encoded random path, every 7th row scaled by 3.7.  Shared: treat
    the arrays as read-only."""
    from sspslam_amd import harness as H
    space = H.make_ssp_space(domain_dim=dim, ssp_dim=ssp_dim, rng=np.random.RandomState(0))
    d = space.ssp_dim
    rng = np.random.RandomState(1)
    path = rng.uniform(-0.9, 0.9, (T, dim))
    rows = space.encode(path) + rng.randn(T, d) * 0.5 / np.sqrt(d)
    rows[::7] *= 3.7
    table, points = space.get_sample_pts_and_ssps(n_per_axis, "grid")
    for a in (rows, table, points):
        a.setflags(write=False)
    return space, rows, table, points


@functools.lru_cache(maxsize=None)
def standard_reference(dim, ssp_dim, n_per_axis, T):
    _, rows, table, _ = standard_case(dim, ssp_dim, n_per_axis, T)
    return Reference(table, rows)
