"""The instrument of the region-SSP tests (tests only): float64 host answers for the SSP of an axis-aligned box and the bars a device
``encode_region`` is held to.  The spaces are those of ``encode_checks.CASES``.

With ``(K, M, w) = space.refine_tables()``, a box of centre ``c`` and side lengths ``L``, ``th_k = M_k . c`` and ``B`` of
``encode_checks.factors``, a region SSP is ``[A cos th, A sin th] @ B`` with the real amplitude ``A_k`` of the mode:

    integral   prod_a L_a sinc(M_ka L_a / 2)          mean   the same without L_a
    mesh       prod_a sin(n_a y_a) / sin(y_a),  y_a = M_ka L_a / (2 (n_a - 1))

References, neither of which uses a closed form:

* mesh              ``space.encode`` of the linspace mesh (both ends, ``n`` points per axis), summed in float64.
* integral, mean    a composite Gauss-Legendre rule per axis (``gl_reference``).  It uses only that ``exp(i M_k . x)`` is a product
                    over the axes: per axis, panels of half-width h with ``|M_ka| h <= 8`` and ``GL_NODES`` nodes each (the rule's
                    error on exp(i t), |t| <= 8, with 20 nodes is below 1e-19); ``test_region.py`` doubles the nodes (every panel cut in two)
                    and sees the answer move by under 1/8 of the bar.  A zero-width axis is the integrand at that coordinate (mean) or 0.

Bars, per entry.  ``V`` is the amplitude's envelope - ``prod L_a`` (integral), ``prod n_a`` (mesh), 1 (mean) - and
``Sbar_c = V sum_j |B_jc|``: near a zero of the amplitude it is the absolute error that counts, so the envelope and not the value.

* ``f64``   ``2^-53 V sum_k (2K + c_amp(k)) (|B_2k,c| + |B_2k+1,c|)`` plus ``phase_term``.  ``c_amp(k) = 8 + sum_a (5 + 3 |M_ka| L_a)``:
            8 as in ``encode_checks`` (sincos and the table); per axis, relative to the envelope,
              - the argument: ``L = hi - lo``, ``M L``, the factor ``0.5 / (n - 1)`` and its product are four roundings of ``y``, the
                reduction ``r = y - q pi`` a fifth of ``r``; the mesh ratio moves by at most ``n^2 / 2`` per unit of ``y`` (it is a sum
                of n unit phasors of frequencies up to n - 1), i.e. ``n |y| / 2`` of its envelope n per relative rounding, and
                ``n |y| <= |M| L``: ``5/2 |M| L`` in all, rounded up to 3 (sinc moves by under 1/2 per unit of y: less);
              - the values: two sines (or a sine and the series), ``n r`` (pi/2 of the envelope at worst), a division, the product
                over the axes and with ``L_a``, and the product with cos / sin: under 5.
* ``f32``   ``C REL Sbar_c`` with ``REL`` of ``decoding_checks``.  ``C = 2 C0`` and ``C0`` is the worst ``error / (REL Sbar_c)`` of the
            CPU stand-in (``A o P`` and ``B`` rounded to f32, a sequential f32 chain) over every box of every case, mode and count and
            the special boxes; ``measure_c0()`` recomputes it and ``tests/test_region.py`` holds the constant to it.
* ``phase_term``  what the rounding of the phases may move an entry by: the reference evaluates ``M_k . x`` at nodes anywhere in the box,
            the device at the centre (itself rounded), each within ``(dim + 2) 2^-53 sum_a |M_ka| max(|lo_a|, |hi_a|)``; times V.  It is
            what dominates on the far space (|coordinate| = 50, |th| near 1000).

Wrong encoders (``MUTANTS``) that each have to fail on the CPU are at the end.
"""
import functools

import numpy as np

import encode_checks as ec

REL = ec.REL
C0 = 1.63                # measure_c0() gives 1.627 (worst case: the mean at d = 1015); rounded up
C = 2 * C0
N = 130
NS = (1, 63, 64, 65)
MODES = ("integral", "mean", "mesh")
GL_NODES = 20
U64 = 2.0 ** -53


def counts_for(space):
    """The mesh counts (the same on every axis) a case is tested at."""
    return (2, 3, 20) if space.domain_dim < 3 else (2, 3, 7)


def variants(space):
    """(mode, samples) of every device call a case gets."""
    return [("integral", None), ("mean", None)] + [("mesh", n) for n in counts_for(space)]


@functools.lru_cache(maxsize=None)
def case_boxes(name):
    """130 boxes inside the bounds, (130, dim, 2), side lengths log-uniform from 1e-3 of the domain to the whole domain, read-only."""
    b = ec.case_space(name).domain_bounds
    rng = np.random.RandomState(23)
    span = b[:, 1] - b[:, 0]
    L = span * 10.0 ** rng.uniform(-3.0, 0.0, (N, b.shape[0]))
    L[0] = span                                                   # and one that is the whole domain
    lo = b[:, 0] + rng.uniform(0.0, 1.0, L.shape) * (span - L)
    boxes = np.stack([lo, np.minimum(lo + L, b[:, 1])], axis=2)
    boxes.setflags(write=False)
    return boxes


PI_BIN = 40              # the bin of d97-2d whose y the pi boxes put at pi


@functools.lru_cache(maxsize=None)
def special_boxes(name="d97-2d"):
    """{label: (boxes, mode, samples)}: each the smallest input that reaches a branch.  Zero-width axes in each mode, the whole domain,
    a box straddling the origin, and in mesh mode boxes whose y on axis 0 for bin PI_BIN is pi and pi +- 1e-9 (n = 2: the sign of an
    odd q with an even n; n = 3: where n y is not exact)."""
    space = ec.case_space(name)
    b = space.domain_bounds
    dim = b.shape[0]
    mid, span = 0.5 * (b[:, 0] + b[:, 1]), b[:, 1] - b[:, 0]
    line = np.stack([mid - 0.1 * span, mid + 0.15 * span], axis=1)
    line[0] = mid[0] + 0.2 * span[0]                              # zero width on axis 0
    point = np.stack([mid + 0.2 * span, mid + 0.2 * span], axis=1)
    zero = np.stack([line, point])
    origin = np.stack([-0.013 * span, 0.21 * span], axis=1)[None]
    out = {f"zero width, {m}": (zero, m, s) for m, s in (("integral", None), ("mean", None), ("mesh", 3))}
    for m, s in variants(space):
        out[f"whole domain, {m} {s}"] = (b[None].copy(), m, s)
        out[f"straddling the origin, {m} {s}"] = (origin, m, s)
    _, M, _ = space.refine_tables()
    m0 = abs(M[PI_BIN, 0])
    for n in (2, 3):
        L0 = 2.0 * np.pi * (n - 1) / m0
        assert L0 < 0.9 * span[0], (name, n, L0)
        rows = []
        for off in (0.0, 1e-9, -1e-9):
            box = np.stack([mid - 0.05 * span, mid + 0.1 * span], axis=1)
            box[0] = b[0, 0] + 0.03 * span[0], b[0, 0] + 0.03 * span[0] + L0 * (1.0 + off / np.pi)
            rows.append(box)
        out[f"y = pi and pi +- 1e-9, n = {n}"] = (np.stack(rows), "mesh", n)
    for v in out.values():
        v[0].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def far_boxes():
    """Boxes at |coordinate| = 50 on the far space (length scale 0.2: |th| near 1000 rad)."""
    boxes = np.array([[[49.6, 50.0], [-50.0, -49.7]], [[-50.0, -49.99], [49.0, 50.0]], [[50.0, 50.0], [-50.0, -50.0]]])
    boxes.setflags(write=False)
    return boxes


# -- references ---------------------------------------------------------------------------------------------------------------------
def as_counts(space, samples):
    return None if samples is None else np.full(space.domain_dim, samples) if np.ndim(samples) == 0 else np.asarray(samples)


def mesh_reference(space, boxes, samples):
    """``space.encode`` of every box's linspace mesh, summed in float64."""
    counts = as_counts(space, samples)
    out = np.empty((len(boxes), space.ssp_dim))
    for i, box in enumerate(boxes):
        axes = [np.linspace(box[a, 0], box[a, 1], int(counts[a])) for a in range(space.domain_dim)]
        out[i] = space.encode(np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, space.domain_dim)).sum(axis=0)
    return out


def gl_reference(space, boxes, mean, nodes=GL_NODES, split=1):
    """The integral (or mean) of ``space.encode`` over every box by a composite Gauss-Legendre rule per axis; ``split`` cuts every
    panel into that many (``split=2`` doubles the nodes)."""
    K, M, w = space.refine_tables()
    t, wt = np.polynomial.legendre.leggauss(nodes)
    B = ec.factors(space, np.zeros((1, space.domain_dim)))[1]
    P = np.empty((len(boxes), 2 * K))
    for i, box in enumerate(boxes):
        F = np.ones(K, dtype=complex)
        for a in range(space.domain_dim):
            lo, hi = box[a]
            L = hi - lo
            panels = split * max(1, int(np.ceil(np.abs(M[:, a]).max() * L / 16.0)))
            h = L / (2 * panels)
            x = (lo + h * (2 * np.arange(panels) + 1))[:, None] + h * t[None, :]            # (panels, nodes)
            axis_mean = (np.exp(1j * M[:, a][:, None, None] * x[None]) * wt[None, None, :]).sum(axis=(1, 2)) / (2 * panels)
            F = F * axis_mean * (1.0 if mean else L)
        P[i, 0::2], P[i, 1::2] = F.real, F.imag
    return P @ B


def envelope(space, boxes, mode, samples):
    L = boxes[:, :, 1] - boxes[:, :, 0]
    if mode == "integral":
        return np.prod(L, axis=1)
    if mode == "mean":
        return np.ones(len(boxes))
    return np.full(len(boxes), float(np.prod(as_counts(space, samples))))


class Reference:
    def __init__(self, space, boxes, mode, samples=None, nodes=GL_NODES):
        self.space, self.mode, self.samples = space, mode, samples
        self.boxes = np.asarray(boxes, dtype=np.float64)
        self.want = mesh_reference(space, self.boxes, samples) if mode == "mesh" else gl_reference(space, self.boxes, mode == "mean", nodes)
        K, M, w = space.refine_tables()
        self.K = K
        absB = np.abs(ec.factors(space, np.zeros((1, space.domain_dim)))[1])
        self.pairB = absB[0::2] + absB[1::2]                                                # (K, d)
        self.V = envelope(space, self.boxes, mode, samples)
        L = self.boxes[:, :, 1] - self.boxes[:, :, 0]
        self.c_amp = 8.0 + 5.0 * space.domain_dim + 3.0 * L @ np.abs(M).T                   # (N, K)
        self.Sbar = self.V[:, None] * self.pairB.sum(axis=0)[None, :]
        reach = np.abs(self.boxes).max(axis=2) @ np.abs(M).T                                # (N, K)
        self.phase = self.V[:, None] * ((2 * (space.domain_dim + 2) * U64 * reach) @ self.pairB)

    def bar(self, dtype, rows=slice(None)):
        if dtype == "f64":
            return U64 * self.V[rows, None] * ((2 * self.K + self.c_amp[rows]) @ self.pairB) + self.phase[rows]
        return C * REL * self.Sbar[rows]

    def ratio(self, got, dtype, rows=slice(None)):
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == self.want[rows].shape, (got.shape, self.want[rows].shape)
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.abs(got - self.want[rows]) / self.bar(dtype, rows)
        r = np.where(got == self.want[rows], 0.0, r)                  # a zero-volume integral: 0 against 0 under a bar of 0
        return np.where(np.isnan(r), np.inf, r)

    def check(self, got, dtype, rows=slice(None), label="", limit=1.0):
        """Every entry of every row under ``limit`` of its bar; prints and returns the worst ratio."""
        r = self.ratio(got, dtype, rows)
        worst = float(r.max()) if r.size else 0.0
        print(f"{label} {self.mode} {self.samples} {dtype}: {r.shape[0]} boxes x {r.shape[1]}, worst |error| / bar = {worst:.3f}")
        assert worst <= limit, (label, self.mode, self.samples, dtype, worst, np.argwhere(r > limit)[:4])
        return worst


@functools.lru_cache(maxsize=None)
def reference(name, mode, samples=None):
    return Reference(ec.case_space(name), case_boxes(name), mode, samples)


@functools.lru_cache(maxsize=None)
def special_reference(label, name="d97-2d"):
    boxes, mode, samples = special_boxes(name)[label]
    return Reference(ec.case_space(name), boxes, mode, samples)


@functools.lru_cache(maxsize=None)
def far_reference(mode, samples=None):
    return Reference(ec.case_space(ec.FAR), far_boxes(), mode, samples)


# -- the closed form, with NumPy, and its wrong variants ------------------------------------------------------------------------------
def _sinc(y, guard=True):
    small = np.abs(y) < 2.0 ** -10
    y2 = y * y
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(small, 1.0 + y2 * (y2 / 120.0 - 1.0 / 6.0), np.sin(y) / np.where(small, 1.0, y)) if guard else np.sin(y) / y


PI_A = float(np.float32(np.pi))
PI_B = float(np.float32(np.pi - PI_A))
PI_C = (np.pi - PI_A - PI_B) + 1.2246467991473532e-16


def _dirichlet(y, n, guard=True):
    if not guard:                                                    # guarded at y = 0 alone
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(y == 0, n, np.sin(n * y) / np.sin(y))
    q = np.rint(y / np.pi)
    r = ((y - q * PI_A) - q * PI_B) - q * PI_C
    small = np.abs(r) < 2.0 ** -26
    v = np.where(small, n * _sinc(n * r), np.sin(n * r) / np.sin(np.where(small, 1.0, r)))
    return np.where((np.mod(np.abs(q), 2.0) == 1.0) & (n % 2 == 0), -v, v)


def factors(space, boxes, mode, samples=None, fault=None):
    """(A o P, B, K) in float64: what ``k_encode_phase_box`` writes and the encoder's table.  ``fault``: one of MUTANTS."""
    assert fault is None or fault in MUTANTS
    K, M, w = space.refine_tables()
    boxes = np.asarray(boxes, dtype=np.float64)
    lo, hi = boxes[:, :, 0], boxes[:, :, 1]
    L = hi - lo
    counts = as_counts(space, samples)
    at = lo if fault == "corner instead of centre" else 0.5 * (lo + hi)
    th = np.zeros((len(boxes), K))
    for a in range(space.domain_dim):
        th = th + at[:, a:a + 1] * M[None, :, a]
    amp = np.ones((len(boxes), K))
    ft = np.float32 if fault == "amplitude in f32" else np.float64
    for a in range(space.domain_dim if fault != "amplitude of one axis only" else 1):
        mL = (L[:, a:a + 1].astype(ft) * M[None, :, a].astype(ft)).astype(ft)
        if mode == "mesh":
            n = float(counts[a])
            y = mL * ft(0.5 / (n if fault == "L / n instead of L / (n - 1)" else n - 1.0))
            f = _dirichlet(y, ft(n), guard=fault != "no guard at y = pi")
        else:
            f = _sinc(ft(0.5) * mL, guard=fault != "no guard at y = 0")
            if mode == "integral" and fault != "missing L factor":
                f = f * L[:, a:a + 1].astype(ft)
        amp = amp * np.asarray(f, dtype=ft).astype(np.float64)
    P = np.empty((len(boxes), 2 * K))
    P[:, 0::2], P[:, 1::2] = amp * np.cos(th), amp * np.sin(th) * (-1.0 if fault == "sign of the sine term" else 1.0)
    return P, ec.factors(space, np.zeros((1, space.domain_dim)))[1], K


def f64_stand_in(space, boxes, mode, samples=None, fault=None):
    """An ordered float64 sum over the 2K columns."""
    P, B, K = factors(space, boxes, mode, samples, fault)
    acc = np.zeros((P.shape[0], B.shape[1]))
    for j in range(2 * K):
        acc = acc + P[:, j:j + 1] * B[j][None, :]
    return acc


def f32_stand_in(space, boxes, mode, samples=None):
    """A o P and B rounded to f32 and a sequential f32 chain over the 2K columns."""
    P, B, K = factors(space, boxes, mode, samples)
    P32, B32 = P.astype(np.float32), B.astype(np.float32)
    acc = np.zeros((P.shape[0], B.shape[1]), dtype=np.float32)
    for j in range(2 * K):
        acc = acc + P32[:, j:j + 1] * B32[j][None, :]
    return acc.astype(np.float64)


def all_references():
    """Every (label, Reference) the constant C is measured over."""
    for name in ec.CASES:
        for mode, samples in variants(ec.case_space(name)):
            yield f"{name} {mode} {samples}", reference(name, mode, samples)
    for label in special_boxes():
        yield label, special_reference(label)
    for mode, samples in variants(ec.case_space(ec.FAR)):
        yield f"far {mode} {samples}", far_reference(mode, samples)


def measure_c0():
    """Worst error / (REL Sbar_c) of the f32 stand-in over everything ``all_references`` lists: (c0, {label: worst})."""
    per = {}
    for label, ref in all_references():
        got = f32_stand_in(ref.space, ref.boxes, ref.mode, ref.samples)
        live = ref.Sbar > 0                                           # a zero-volume integral: 0 against 0
        per[label] = float(np.max(np.abs(got - ref.want)[live] / (REL * ref.Sbar[live]))) if live.any() else 0.0
    return max(per.values()), per


# -- area queries ---------------------------------------------------------------------------------------------------------------------
AREA_STEPS = 300
AREA_LOCATIONS = np.array([[-0.6, -0.5], [0.5, -0.4], [0.0, 0.6]])
AREA_HALF = np.array([0.15, 0.2])                                    # half sides of the query boxes: one trained location in each


def area_network(n=600, d_val=16, seed=5, dt=0.001):
    """An inverse memory alone (slam_map_new.py:243-250 in small): keys are the SSPs of three locations on the d = 55 space, values
    three SPs, the next pair every 100 timesteps, learning on (the error path at tau = 5 ms, so that a value meets its own key and not
    the one before).  -> (network, dict(memory, space, keys, vocab, boxes)); ``boxes[i]`` holds location i and no other."""
    from sspslam_amd import frontend as nengo
    from sspslam_amd import harness as H
    from sspslam_amd.networks.associativememory import AssociativeMemory
    from sspslam_amd.sspspace import SPSpace
    space = H.make_ssp_space(2, ssp_dim=55)
    keys = space.encode(AREA_LOCATIONS)
    vocab = np.asarray(SPSpace(3, d_val, seed=seed).vectors, dtype=np.float64)
    which = lambda t: int(round(t / dt) - 1) // 100 % 3      # noqa: E731
    net = nengo.Network(seed=seed)
    with net:
        key_in = nengo.Node(lambda t: keys[which(t)], label="key")
        val_in = nengo.Node(lambda t: vocab[which(t)], label="value")
        learn = nengo.Node(lambda t: np.zeros(1), label="learn")
        mem = AssociativeMemory(n, space.ssp_dim, d_val, 0.1, voja_learning_rate=5e-3, pes_learning_rate=4e-3, tau=0.005, seed=seed)
        nengo.Connection(key_in, mem.key_input, synapse=None)
        nengo.Connection(val_in, mem.value_input, synapse=None)
        nengo.Connection(learn, mem.learning, synapse=None)
    boxes = np.stack([AREA_LOCATIONS - AREA_HALF, AREA_LOCATIONS + AREA_HALF], axis=2)
    return net, dict(memory=mem, space=space, keys=keys, vocab=vocab, boxes=boxes)


# wrong encoders: name -> the (mode, samples) they are visible in ("pi": the special boxes at y = pi with n = 3)
MUTANTS = {
    "L / n instead of L / (n - 1)": ("mesh", 3),
    "corner instead of centre": ("integral", None),
    "missing L factor": ("integral", None),
    "amplitude of one axis only": ("mean", None),
    "no guard at y = 0": ("mean", None),
    "no guard at y = pi": ("pi", 3),
    "sign of the sine term": ("mesh", 20),
    "amplitude in f32": ("integral", None),
}
