"""One-step float64 restart instrument for the f32 step, every operator (tests only; neither a test module nor a conftest).

The closed loop of a SLAM network decorrelates an f32 run from the float64 oracle as soon as one spike moves by a timestep, so
the suite's f32 bars on whole runs are 1e-3 cosine and 2e-2 in norm.  ONE step from the device's own state has no such
amplification: the device's state is read (``fork_from_device``), a float64 ``OracleSimulator`` takes one step from it with a
first-order error bound carried beside every signal element and every state / learned buffer (``bounded_step``), the device takes
the same step, and what the device carries into the next step is compared element by element (``check_restart_step``).

What is compared: ``carried(model)``
    the signal elements that some operator reads before the step has rewritten them (derived from the read and write ranges of
    every operator kind, as ``OracleSimulator.step`` uses them), the ranges of the probes, and every buffer of role ``state`` or
    ``learned``.  A fused kernel need not materialise a signal that is dead at the end of a step, so nothing else is asked of a device.

Bound rules, u = 2^-24, first order; b(x) is the bound carried by x; the initial bound is zero (the state is the device's own)
    fill, table       u |value|
    axpy, lincomb,    (terms + 1) u sum|term| + sum |coefficient| b(input): one rounding of each coefficient, one of each product,
    lowpass           terms - 1 additions
    matvec            the smaller of two bounds, both valid for any summation order; t_j = W_j x_j, n = number of NONZERO x_j (a zero
                      adds exactly: the decoded sum of a spike vector has as many roundings as spikes):
                        worst case      (n + 2) u sum|t|
                        probabilistic   LAMBDA u sqrt(2 sum t^2 + sum_k p_k^2): the rounding of W and of the product on every term, and
                                        n - 1 additions whose results p_k are partial sums.  In ANY summation tree the k-th smallest
                                        node has at most k + 1 leaves (a node of m leaves holds m - 1 nodes no larger than itself),
                                        so |p_k| <= the sum of the k + 1 largest |t|, and <= max(sum of the positive t, sum of the
                                        negative ones) as a subset sum.  Rounding errors are taken as independent with variance
                                        0.18 u^2 value^2 (uniform in +-ulp/2, logarithmically distributed mantissas) and the bound
                                        is six standard deviations, LAMBDA = 6 sqrt(0.18): exceeded with probability 3e-8 per element
                                        if every partial sum were as large as its bound.  The worst-case rule alone is 300 times the
                                        NumPy f32 error of a 55-term product, and it reaches the neurons behind it: the condition
                                        of tests/test_slam_restart.py (bound / error of the NumPy f32 oracle, median <= 64) asks for this.
                      input bounds pass through as the smaller of |W| b(x) and LAMBDA sqrt(W^2 b(x)^2) (independent errors, each
                      uniform within its bound or better); "inc" adds b(dst) + u (|dst| + |y|)
    encode / decode   (n + 2) u (|W| |x|) + |W| b(x) with n = din, or the spikes of the member
    of an ensarray
    matvec with dft   the larger of the matvec rule (the dense route) and the FFT route's: a pass of radix r is a dense r-point
                      transform on every sub-vector, variance proportional to r + 2, twice that for the twiddle products and for
                      passes taken together; an element of the output has magnitude |W|_F |x|_2 / sqrt(rows cols) on average:
                      LAMBDA u sqrt(2 sum_passes (r + 2)) |W|_F |x|_2 / sqrt(rows cols), r over the prime factors of d.  At d = 55 this
                      is 9e-7 |x|_2 forward, a sixteenth of the 2e-6 sqrt(d) that test_dft_kernel_matches_the_transform_matrices holds
                      k_dft to (that bar is 250 u |x|_2: behind it the product neurons' bound would be 200 times their f32 error)
    neurons, LIF of   the bV / bR recursion of lif_open_loop.restart_reference for ONE step from an exact state, with the bound of
    an ensarray       the input current from above and the step's own terms taken apart (that module doubles their sum into
                      4 u g, g = 1 + |J| + |V|; the rounding of J is b(J) here): bV = em b(J) + 3 u em |J - V| (subtraction, em,
                      product) + 0.2 u g (the polynomial's coefficients) + [partial step] (2.3e-7 |J - V| + |J - V| exp(-delta /
                      tau_rc) bR0 / tau_rc); the rounding of V' itself is the comparison's 2 u |V'|.  A spike: bR = tau_rc ((bV +
                      q b(J)) / ((J - 1)(1 - q)) + 5e-8 + 4 u) + eR (dt_spike/dJ = tau_rc q / ((J - 1)(1 - q))); bR0 = eR = 2^-22
                      tau_ref where the device holds a refractory time (its time word).  The per-timestep kernels are held to the
                      block kernel's terms, as that module decides.  Rate types: d rate / dJ b(J) + 8 u rate (LIF rate), b(J) + u (ReLU)
    pes               on the INCREMENT after - before, both read from the device: 3 u |kappa err act| + |kappa| (b(err) |act| +
                      |err| b(act)) + u |W|
    voja              the same on rows with a != 0: 3 u (|lr L s a key| + |lr L a E|) + the bounds of key and L + u |E|; a row with
                      a == 0 must be bit-unchanged
    cleanup, gate     decisions, below
    everything is compared under  bound + 2 u |value|  (refractory times: bR + eR, as in lif_open_loop).

Decisions
    neuron    MARGINAL as in lif_open_loop: |V' - 1| <= bV at the spike test or |R' - dt| <= bR + eR at the refractory flag.
    cleanup   marginal: the float64 top-two gap <= B = 2 (cols + 2) u sum_j |S_j| |x_j| + 2 |S| b(x); it may then return any row
              whose float64 similarity is within B of the best.  Otherwise it returns the float64 row, compared with the table row
              under atol 2e-6 (test_slam_3d_matches_oracle).
    gate      marginal: |dot - thres| <= b(dot) (or ||flag| - 1e-3| <= b(flag)); otherwise open or closed as in float64, the
              output under the axpy bound.
    A restart point is SKIPPED when a marginal decision came out differently on the device: its values are not compared, and
    decisions of operators behind the flipped one in program order are not judged (everything downstream differs legitimately).
    A different decision on an item that is not marginal, in the flipped operator or before it, stays a failure, as does any
    such decision at a point without a flip.  ``run_points`` admits one skip.
"""
import copy

import numpy as np

import sspslam_amd.frontend as nengo
from sspslam_amd import harness as H
from sspslam_amd.builder import build as build_model
from oracle import OracleSimulator

from lif_open_loop import BLOCK_TERMS, U24 as U, canonical_R

CLEANUP_ATOL = 2e-6
FLAG_EPS = 1e-3
# a rounding error is uniform in +-ulp/2, ulp/2 = u 2^e <= u |value|: variance (u 2^e)^2 / 3, and 0.18 u^2 value^2 over logarithmically
# distributed mantissas (the mean of (2^e / value)^2 is 3 / (8 ln 2)).  A sum of independent ones with weights w exceeds six standard
# deviations = LAMBDA u |w|_2 with probability 2 exp(-18) = 3e-8
LAMBDA = 6.0 * np.sqrt(0.18)


# ---- read and write ranges --------------------------------------------------------------------------------------------------
def op_access(model, o):
    """-> (reads, writes): lists of index arrays / (lo, hi) of the signal vector one operator reads and fully rewrites."""
    k = o["kind"]
    r = lambda lo, n: (int(lo), int(lo) + int(n))
    if k == "fill":
        return [], [r(o["dst"], o["len"])]
    if k == "table":
        return [], [r(o["dst"], o["width"])]
    if k == "axpy":
        return [r(o["src"], o["len"])] + ([r(o["dst"], o["len"])] if o["mode"] != "set" else []), [r(o["dst"], o["len"])]
    if k == "lincomb":
        return [r(s, o["len"]) for s in o["srcs"]] + ([r(o["dst"], o["len"])] if o["self"] else []), [r(o["dst"], o["len"])]
    if k == "matvec":
        return [r(o["src"], o["cols"])] + ([r(o["dst"], o["rows"])] if o["mode"] != "set" else []), [r(o["dst"], o["rows"])]
    if k == "lowpass":
        return [r(o["src"], o["len"]), r(o["dst"], o["len"])], [r(o["dst"], o["len"])]
    if k == "ensarray":
        return [r(o["x"], o["K"] * o["din"])], [np.asarray(model.buffers[o["dst_idx"]]).reshape(-1)]
    if k == "neurons":
        return [r(o["j"], o["n"])], [r(o["out"], o["n"])]
    if k == "pes":
        return [r(o["err"], o["rows"]), r(o["act"], o["cols"])], []
    if k == "voja":
        return [r(o["spk"], o["rows"]), r(o["key"], o["cols"]), r(o["learn"], 1)], []
    if k == "cleanup":
        return [r(o["src"], o["cols"])], [r(o["dst"], o["cols"])]
    if k == "gate":
        return [r(o["src"], 2 * o["d"] + 1)], [r(o["dst"], o["d"])]
    raise ValueError(f"unknown op {k}")


def _sel(a):
    return slice(*a) if isinstance(a, tuple) else a


def _ranges(mask):
    edges = np.flatnonzero(np.diff(np.concatenate([[0], mask.astype(np.int8), [0]])))
    return [(int(lo), int(hi)) for lo, hi in zip(edges[::2], edges[1::2])]


class Carried:
    """``signals`` / ``probes``: merged (lo, hi) ranges; ``buffers``: ids of the state and learned buffers; ``mask`` = signals or
    probes, ``written`` = every element some operator writes; ``writer[i]`` = index of the LAST operator that writes element i (-1)."""


def carried(model):
    n = int(model.sig_size)
    written = np.zeros(n, dtype=bool)
    live = np.zeros(n, dtype=bool)
    writer = np.full(n, -1, dtype=np.int64)
    for j, o in enumerate(model.ops):
        reads, writes = op_access(model, o)
        for a in reads:
            s = _sel(a)
            live[s] |= ~written[s]
        for a in writes:
            s = _sel(a)
            written[s] = True
            writer[s] = j
    c = Carried()
    live &= written                      # (a signal nothing writes is a constant: the device holds what it was given)
    pm = np.zeros(n, dtype=bool)
    for p in model.probes:
        if "src" in p:
            pm[p["src"]:p["src"] + p["width"]] = True
    c.signals, c.probes = _ranges(live), _ranges(pm)
    c.buffers = [i for i, meta in enumerate(model.buffer_meta) if meta["role"] in ("state", "learned")]
    c.mask, c.written, c.writer = live | (pm & written), written, writer
    return c


# ---- the device's state as a float64 oracle ---------------------------------------------------------------------------------
def _refractory_buffers(model):
    return {o["r"] for o in model.ops if o["kind"] in ("ensarray", "neurons")}


def read_state(model, sim):
    """-> (sig, {buffer id: array}) of a device (or stand-in), refractory times in the packed-word convention (canonical_R)."""
    sig = np.array(sim.read_signal(0, int(model.sig_size)), dtype=np.float64)
    rb = _refractory_buffers(model)
    bufs = {}
    for i, meta in enumerate(model.buffer_meta):
        if meta["role"] in ("state", "learned"):
            b = np.array(sim.read_buffer(i), dtype=np.float64).reshape(np.shape(model.buffers[i]))
            bufs[i] = canonical_R(b, model.dt) if i in rb else b
    return sig, bufs


def fork_from_device(model, sim, state=None):
    sig, bufs = state if state is not None else read_state(model, sim)
    ref = OracleSimulator(model)
    ref.sig = sig.copy()
    for i, b in bufs.items():
        ref.buf[i] = b.copy()
    ref.n_steps = int(sim.n_steps)
    return ref


def _single_op_runner(ref):
    """apply(o): ONE operator executed by ``OracleSimulator.step`` itself on ``ref`` (its clock is left on the step being taken)."""
    one = copy.copy(ref.model)
    one.probes = []
    full = ref.model

    def apply(o):
        one.ops = [o]
        ref.model = one
        ref.n_steps -= 1
        try:
            ref.step()
        finally:
            ref.model = full
    return apply


# ---- one float64 step with bounds --------------------------------------------------------------------------------------------
def _lif_bounds(neuron, J, bJ, V0, R0, dt, terms):
    """One LIF step from the exact state (V0, R0): -> Vt (the spike test's operand), spiked, bV, bR, marginal."""
    tau_rc, tau_ref = neuron["tau_rc"], neuron["tau_ref"]
    eR = 2.0 ** -22 * tau_ref
    bR0 = np.where(R0 > dt, eR, 0.0)
    delta = np.clip(dt - (R0 - dt), 0.0, dt)
    em = -np.expm1(-delta / tau_rc)
    Vt = V0 + (J - V0) * em
    partial = (delta > 0) & (delta < dt)
    moving = delta > 0
    g = 1.0 + np.abs(J) + np.abs(V0)
    own = em * np.abs(J - V0) * 3 * U + 0.2 * U * g + partial * terms["em"] * np.abs(J - V0)      # (V' itself: the comparison's 2 u |V'|)
    bV = np.where(moving, em * bJ + own + partial * np.abs(J - V0) * np.exp(-delta / tau_rc) * bR0 / tau_rc, 0.0)
    spiked = Vt > 1
    marginal = moving & (np.abs(Vt - 1.0) <= bV)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (Vt - 1.0) / (J - 1.0)
        bR_spike = tau_rc * ((bV + np.abs(q) * bJ) / (np.abs(J - 1.0) * np.maximum(1.0 - q, 1e-3)) + terms["log"] + 4 * U) + eR
        t_spike = dt + tau_rc * np.log1p(-q)
    R1 = np.where(spiked, tau_ref + t_spike, R0 - dt)
    bR_kept = np.where(spiked, bR_spike, bR0 + eR)
    marginal |= (np.abs(R1 - dt) <= bR_kept + eR) & (spiked | (R0 > dt))
    bR = np.where(R1 > dt, bR_kept, 0.0)
    bV = np.where(spiked, 0.0, bV)
    return Vt, spiked, bV, bR, marginal


def _activity_bounds(neuron, J, bJ, V0, R0, dt, terms):
    """-> (activity at unit amplitude, its bound, bV, bR, marginal, LIF details or None) for one neuron operator; V0 / R0: the state
    BEFORE the operator."""
    t = neuron["type"]
    zero = np.zeros_like(J)
    if t == "lif":
        Vt, spiked, bV, bR, marginal = _lif_bounds(neuron, J, bJ, V0, canonical_R(R0, dt), dt, terms)
        return spiked.astype(np.float64), zero, bV, bR, marginal, dict(Vt=Vt, J=J.copy(), spiked=spiked)
    none = np.zeros(J.shape, dtype=bool)
    if t == "relu":
        return np.maximum(J, 0.0), bJ + U * np.abs(J), zero, zero, none, None
    tau_rc, tau_ref = neuron["tau_rc"], neuron["tau_ref"]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(J > 1, 1.0 / (tau_ref + tau_rc * np.log1p(1.0 / (J - 1.0))), 0.0)
        slope = np.where(J > 1, a * a * tau_rc / (J * (J - 1.0)), 0.0)
    return a, slope * bJ + 8 * U * a, zero, zero, (np.abs(J - 1.0) <= bJ + 2 * U), None


def _product_bound(W, x):
    """Rounding of y = W x in f32, any summation order, per row (module docstring, ``matvec``)."""
    t = W * x[None, :]
    nz = int(np.count_nonzero(x))
    S = np.abs(t).sum(axis=1)
    P = np.maximum(t, 0.0).sum(axis=1)
    worst = (nz + 2) * U * S
    # the nz - 1 partial sums of ANY summation tree: the k-th smallest node has at most k + 1 leaves (a node of m leaves holds m - 1
    # nodes no larger than itself), so its value is at most the sum of the k + 1 largest |terms|, and at most max(P, N) as a subset sum
    L = np.cumsum(-np.sort(-np.abs(t), axis=1), axis=1)[:, 1:max(nz, 1)]
    partial2 = (np.minimum(L, np.maximum(P, S - P)[:, None]) ** 2).sum(axis=1)
    prob = LAMBDA * U * np.sqrt(2.0 * (t * t).sum(axis=1) + partial2)
    return np.minimum(worst, prob)


def _prime_factors(n):
    out, p = [], 2
    while p * p <= n:
        while n % p == 0:
            out.append(p)
            n //= p
        p += 1
    return out + ([n] if n > 1 else [])


def _fft_bound(W, x, d):
    """Rounding of the same product taken as a d-point FFT (module docstring, ``matvec with dft``); one figure for every row."""
    c2 = 2.0 * sum(r + 2 for r in _prime_factors(int(d)))
    return LAMBDA * U * np.sqrt(c2) * float(np.linalg.norm(W)) * float(np.linalg.norm(x)) / np.sqrt(W.shape[0] * W.shape[1])


class StepBounds:
    """What ``bounded_step`` leaves: ``bs`` (bound per signal element), ``bb[buffer id]`` (bound per element of V, R and of the learned
    INCREMENT), ``marginal[v buffer id]``, ``lif[v buffer id]`` (Vt, J, spiked of a ``neurons`` operator), ``cleanup`` / ``gate`` / ``pes`` / ``voja``: one record per operator of that kind."""


def bounded_step(model, ref, terms=BLOCK_TERMS):
    """``ref`` (a float64 oracle holding the device's state) takes one step, operator by operator through ``OracleSimulator.step``
    itself; the bounds of the module docstring are propagated beside it."""
    dt = model.dt
    sig, buf = ref.sig, ref.buf
    out = StepBounds()
    bs = out.bs = np.zeros(sig.shape)
    out.bb, out.marginal, out.cleanup, out.gate, out.pes, out.voja, out.lif = {}, {}, [], [], [], [], {}
    ref.n_steps += 1
    apply = _single_op_runner(ref)
    for j, o in enumerate(model.ops):
        k = o["kind"]
        if k in ("fill", "table"):
            apply(o)
            n = o["len"] if k == "fill" else o["width"]
            bs[o["dst"]:o["dst"] + n] = U * np.abs(sig[o["dst"]:o["dst"] + n])
        elif k == "axpy":
            d, s = slice(o["dst"], o["dst"] + o["len"]), slice(o["src"], o["src"] + o["len"])
            t = np.abs(o["alpha"] * sig[s])
            if o["mode"] == "set":
                nb = 2 * U * t + abs(o["alpha"]) * bs[s]
            else:
                nb = 3 * U * (np.abs(sig[d]) + t) + bs[d] + abs(o["alpha"]) * bs[s]
            apply(o)
            bs[d] = nb
        elif k == "lincomb":
            d = slice(o["dst"], o["dst"] + o["len"])
            mag = np.full(o["len"], abs(o["const"]))
            nb = np.zeros(o["len"])
            nt = 1 if o["const"] else 0
            for src, alpha in zip(o["srcs"], o["alphas"]):
                mag = mag + np.abs(alpha * sig[src:src + o["len"]])
                nb = nb + abs(alpha) * bs[src:src + o["len"]]
                nt += 1
            if o["self"]:
                mag = mag + np.abs(o["self"] * sig[d])
                nb = nb + abs(o["self"]) * bs[d]
                nt += 1
            apply(o)
            bs[d] = nb + (nt + 1) * U * mag
        elif k == "matvec":
            Wm = buf[o["w"]]
            s, d = slice(o["src"], o["src"] + o["cols"]), slice(o["dst"], o["dst"] + o["rows"])
            x = sig[s].copy()
            by = _product_bound(Wm, x)
            if o.get("dft"):
                by = np.maximum(by, _fft_bound(Wm, x, o["rows"] if o["dft"] == 5 else o["cols"]))
            by = by + np.minimum(np.abs(Wm) @ bs[s], LAMBDA * np.sqrt((Wm * Wm) @ (bs[s] * bs[s])))
            if o["mode"] != "set":
                y = Wm @ x
                by = by + bs[d] + U * (np.abs(sig[d]) + np.abs(y))
            apply(o)
            bs[d] = by
        elif k == "lowpass":
            d, s = slice(o["dst"], o["dst"] + o["len"]), slice(o["src"], o["src"] + o["len"])
            b = (1.0 - o["a"]) * o["gain"]
            nb = 3 * U * (np.abs(o["a"] * sig[d]) + np.abs(b * sig[s])) + abs(o["a"]) * bs[d] + abs(b) * bs[s]
            apply(o)
            bs[d] = nb
        elif k == "neurons":
            js = slice(o["j"], o["j"] + o["n"])
            J, bJ = sig[js].copy(), bs[js].copy()
            _, ba, bV, bR, marg, out.lif[o["v"]] = _activity_bounds(o["neuron"], J, bJ, buf[o["v"]].copy(), buf[o["r"]].copy(), dt, terms)
            apply(o)
            bs[o["out"]:o["out"] + o["n"]] = abs(o["amp"]) * ba + U * np.abs(sig[o["out"]:o["out"] + o["n"]])
            out.bb[o["v"]], out.bb[o["r"]], out.marginal[o["v"]] = bV, bR, marg
        elif k == "ensarray":
            K, n, din = o["K"], o["n"], o["din"]
            xs = slice(o["x"], o["x"] + K * din)
            x, bx = sig[xs].reshape(K, din).copy(), bs[xs].reshape(K, din).copy()
            enc, bias = buf[o["enc"]], buf[o["bias"]]
            J = bias + np.einsum("kdn,kd->kn", enc, x)
            bJ = (din + 2) * U * (np.abs(bias) + np.einsum("kdn,kd->kn", np.abs(enc), np.abs(x))) + np.einsum("kdn,kd->kn", np.abs(enc), bx)
            a, ba, bV, bR, marg, _ = _activity_bounds(o["neuron"], J, bJ, buf[o["v"]].copy(), buf[o["r"]].copy(), dt, terms)
            apply(o)
            nzk = np.count_nonzero(a, axis=1)[:, None]
            dabs = np.abs(buf[o["dec"]])
            bdec = (nzk + 2) * U * np.einsum("krn,kn->kr", dabs, a) + np.einsum("krn,kn->kr", dabs, ba)
            bs[np.asarray(buf[o["dst_idx"]]).reshape(-1)] = bdec.reshape(-1)
            out.bb[o["v"]], out.bb[o["r"]], out.marginal[o["v"]] = bV, bR, marg
        elif k == "pes":
            err, act = sig[o["err"]:o["err"] + o["rows"]], sig[o["act"]:o["act"] + o["cols"]]
            berr, bact = bs[o["err"]:o["err"] + o["rows"]], bs[o["act"]:o["act"] + o["cols"]]
            inc = o["kappa"] * np.outer(err, act)
            binc = 3 * U * np.abs(inc) + abs(o["kappa"]) * (np.outer(berr, np.abs(act)) + np.outer(np.abs(err), bact))
            apply(o)
            out.bb[o["w"]] = binc + U * np.abs(buf[o["w"]])
            out.pes.append(dict(op=j, w=o["w"], inc=inc, live=bool(np.abs(inc).max() > 0)))
        elif k == "voja":
            E0 = buf[o["w"]].copy()
            a = sig[o["spk"]:o["spk"] + o["rows"]].copy()
            key, bkey = sig[o["key"]:o["key"] + o["cols"]], bs[o["key"]:o["key"] + o["cols"]]
            L, bL = 1.0 + sig[o["learn"]], bs[o["learn"]]
            scale = buf[o["scale_buf"]]
            t1 = o["lr_dt"] * L * (scale * a)[:, None] * key[None, :]
            t2 = o["lr_dt"] * L * a[:, None] * E0
            binc = 3 * U * (np.abs(t1) + np.abs(t2)) + o["lr_dt"] * abs(L) * np.abs(scale * a)[:, None] * bkey[None, :]
            if L:
                binc = binc + (np.abs(t1) + np.abs(t2)) * bL / abs(L)
            apply(o)
            out.bb[o["w"]] = binc + U * np.abs(buf[o["w"]])
            out.voja.append(dict(op=j, w=o["w"], inc=buf[o["w"]] - E0, rows=np.flatnonzero(a), silent=np.flatnonzero(a == 0),
                                 live=bool(np.count_nonzero(a))))
        elif k == "cleanup":
            T = buf[o["w"]]
            s = slice(o["src"], o["src"] + o["cols"])
            x, bx = sig[s].copy(), bs[s].copy()
            apply(o)
            sims = np.zeros(T.shape[0])
            for c in range(T.shape[1]):      # (the oracle's own summation order: the pick below is the oracle's)
                sims += T[:, c] * x[c]
            best = int(np.argmax(sims))
            assert np.array_equal(sig[o["dst"]:o["dst"] + o["cols"]], T[best])
            B = 2 * (o["cols"] + 2) * U * float(np.abs(T[best]) @ np.abs(x)) + 2 * float(np.abs(T[best]) @ bx)
            second = float(np.partition(sims, -2)[-2]) if sims.size > 1 else -np.inf
            out.cleanup.append(dict(op=j, dst=o["dst"], cols=o["cols"], w=o["w"], best=best, sims=sims, B=B,
                                    marginal=bool(sims[best] - second <= B)))
            bs[o["dst"]:o["dst"] + o["cols"]] = U * np.abs(T[best])
        elif k == "gate":
            d = o["d"]
            xs = sig[o["src"]:o["src"] + 2 * d + 1].copy()
            bx = bs[o["src"]:o["src"] + 2 * d + 1].copy()
            est, cur, flag = xs[:d], xs[d:2 * d], xs[2 * d]
            dot = float(est @ cur)
            bdot = (d + 2) * U * float(np.abs(est) @ np.abs(cur)) + float(np.abs(est) @ bx[d:2 * d] + np.abs(cur) @ bx[:d])
            is_open = abs(flag) <= FLAG_EPS and dot > o["thres"]
            marginal = abs(abs(flag) - FLAG_EPS) <= bx[2 * d] or (abs(flag) <= FLAG_EPS + bx[2 * d] and abs(dot - o["thres"]) <= bdot)
            apply(o)
            assert bool(np.any(sig[o["dst"]:o["dst"] + d] != 0)) <= is_open
            nb = 3 * U * abs(o["rate"]) * (np.abs(est) + np.abs(cur)) + abs(o["rate"]) * (bx[:d] + bx[d:2 * d])
            bs[o["dst"]:o["dst"] + d] = nb if is_open else 0.0
            out.gate.append(dict(op=j, dst=o["dst"], d=d, open=bool(is_open), marginal=bool(marginal), dot=dot, bdot=bdot,
                                 open_value=o["rate"] * (est - cur), open_bound=nb))
        else:
            raise ValueError(f"unknown op {k}")
    return out


# ---- the check ---------------------------------------------------------------------------------------------------------------
def _ratio(diff, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(diff == 0, 0.0, diff / bound)


def _worst(d, key, value):
    d[key] = max(d.get(key, 0.0), float(value))


def check_restart_step(model, sim, terms=BLOCK_TERMS):
    """The device (``sim``: read_signal, read_buffer, run_steps, n_steps) is read, takes ONE step and is read again; the float64
    oracle takes the same step from the first reading with its bounds.  -> report: ``kind`` / ``region`` = worst
    |device - float64| / (bound + 2 u |value|) per operator kind (of the last writer) and per compared region, ``marginal`` counts,
    ``skipped``, ``failures`` (decisions that differ on items that are not marginal, silent Voja rows that changed), ``live``,
    and ``tight[kind]`` = bound / |device - float64| of every compared element the device did not get exactly."""
    c = carried(model)
    state0 = read_state(model, sim)
    ref = fork_from_device(model, sim, state0)
    sim.run_steps(1)
    sig1, buf1 = read_state(model, sim)
    b = bounded_step(model, ref, terms)
    dt = model.dt
    rep = dict(step=int(ref.n_steps), kind={}, region={}, tight={}, failures=[], skipped=False, skip_reasons=[],
               marginal=dict(neurons=0, cleanup=0, gate=0), live=dict(pes=False, voja=False, gate_open=False, voja_rows=0, pes_inc=0.0))
    mask = c.mask
    failures, flips = [], []                 # (operator index, text) / operator index of every marginal decision that came out differently
    kinds = np.array([o["kind"] for o in model.ops] + ["none"])

    def tight(kind, diff, bound):
        m = diff > 0
        if m.any():
            rep["tight"].setdefault(kind, []).append((bound[m] / diff[m]).ravel())

    # decisions first: clean-up rows and gates (their regions are then compared like any other, unless the point is skipped)
    for cl in b.cleanup:
        rep["marginal"]["cleanup"] += cl["marginal"]
        sl = slice(cl["dst"], cl["dst"] + cl["cols"])
        if not mask[sl].all():
            continue
        T = ref.buf[cl["w"]]
        row = sig1[sl]
        if np.abs(row - T[cl["best"]]).max() <= CLEANUP_ATOL:
            continue
        got = int(np.argmax(T @ row))
        if np.abs(row - T[got]).max() > CLEANUP_ATOL:
            failures.append((cl["op"], "cleanup op %d: the output is no row of the table (nearest %d, off by %.3g)" % (cl["op"], got, np.abs(row - T[got]).max())))
        elif cl["marginal"] and cl["sims"][got] >= cl["sims"][cl["best"]] - cl["B"]:
            flips.append(cl["op"])
            rep["skip_reasons"].append("cleanup op %d: marginal, row %d for %d" % (cl["op"], got, cl["best"]))
        else:
            failures.append((cl["op"], "cleanup op %d: row %d for %d, similarity short by %.3g, bound %.3g, marginal %s"
                             % (cl["op"], got, cl["best"], cl["sims"][cl["best"]] - cl["sims"][got], cl["B"], cl["marginal"])))
    for g in b.gate:
        rep["marginal"]["gate"] += g["marginal"]
        rep["live"]["gate_open"] |= g["open"]
        sl = slice(g["dst"], g["dst"] + g["d"])
        if not mask[sl].all():
            continue
        got = sig1[sl]
        if g["open"]:
            differs = not got.any() and bool(np.any(np.abs(g["open_value"]) > g["open_bound"] + 2 * U * np.abs(g["open_value"])))
        else:
            differs = bool(got.any())
        if differs and g["marginal"]:
            flips.append(g["op"])
            rep["skip_reasons"].append("gate op %d: marginal (dot %.6g, bound %.3g), open %s in float64" % (g["op"], g["dot"], g["bdot"], g["open"]))
        elif differs:
            failures.append((g["op"], "gate op %d: float64 %s (dot %.6g, bound %.3g), the device decided otherwise"
                             % (g["op"], "opens" if g["open"] else "stays closed", g["dot"], g["bdot"])))
    # neurons
    for j, o in enumerate(model.ops):
        if o["kind"] not in ("neurons", "ensarray"):
            continue
        v, r = o["v"], o["r"]
        Vr, Rr = ref.buf[v], canonical_R(ref.buf[r], dt)
        Vd, Rd = buf1[v], buf1[r]
        marg = b.marginal[v]
        rep["marginal"]["neurons"] += int(marg.sum())
        if o["neuron"]["type"] != "lif":
            continue
        eR = 2.0 ** -22 * o["neuron"]["tau_ref"]
        flip = (Rd > 0) != (Rr > 0)
        if (flip & ~marg).any():
            failures.append((j, "%s op v=%d: %d refractory flags differ on neurons that are not marginal (first %s)"
                             % (o["kind"], v, int((flip & ~marg).sum()), np.argwhere(flip & ~marg)[:4].tolist())))
        elif flip.any():
            flips.append(j)
            rep["skip_reasons"].append("%s v=%d: %d marginal neurons on the other side" % (o["kind"], v, int(flip.sum())))
        same = ~flip
        dV, dR = np.abs(Vd - Vr), np.abs(Rd - Rr)
        if not (np.isfinite(Vd).all() and np.isfinite(Rd).all()):
            failures.append((-1, "%s v=%d: state not finite" % (o["kind"], v)))
        bV, bR = b.bb[v] + 2 * U * np.abs(Vr), b.bb[r] + eR
        name = model.buffer_meta[v]["name"]
        _worst(rep["kind"], o["kind"], max(_ratio(dV, bV)[same].max(initial=0), _ratio(dR, bR)[same].max(initial=0)))
        _worst(rep["region"], "V " + name, _ratio(dV, bV)[same].max(initial=0))
        _worst(rep["region"], "R " + name, _ratio(dR, bR)[same].max(initial=0))
        tight(o["kind"], dV[same], bV[same])
        tight(o["kind"], dR[same], bR[same])
    # learned matrices: increments
    W0 = state0[1]
    for p in b.pes:
        inc_dev = buf1[p["w"]] - W0[p["w"]]
        diff = np.abs(inc_dev - p["inc"])
        bound = b.bb[p["w"]] + 2 * U * np.abs(p["inc"])
        _worst(rep["kind"], "pes", _ratio(diff, bound).max())
        _worst(rep["region"], "pes " + model.buffer_meta[p["w"]]["name"], _ratio(diff, bound).max())
        tight("pes", diff, bound)
        rep["live"]["pes"] |= bool(p["live"] and np.abs(inc_dev).max() > 0)
        rep["live"]["pes_inc"] = max(rep["live"]["pes_inc"], float(np.abs(inc_dev).max()))
    for p in b.voja:
        inc_dev = buf1[p["w"]] - W0[p["w"]]
        rows = p["rows"]
        if inc_dev[p["silent"]].any():
            failures.append((p["op"], "voja op %d: %d silent rows changed" % (p["op"], int(inc_dev[p["silent"]].any(axis=1).sum()))))
        if rows.size:
            diff = np.abs(inc_dev - p["inc"])[rows]
            bound = (b.bb[p["w"]] + 2 * U * np.abs(p["inc"]))[rows]
            _worst(rep["kind"], "voja", _ratio(diff, bound).max())
            _worst(rep["region"], "voja " + model.buffer_meta[p["w"]]["name"], _ratio(diff, bound).max())
            tight("voja", diff, bound)
            rep["live"]["voja"] |= bool(np.abs(inc_dev[rows]).max() > 0)
            rep["live"]["voja_rows"] += int(rows.size)
    # every compared signal element
    diff = np.abs(sig1 - ref.sig)
    bound = b.bs + 2 * U * np.abs(ref.sig)
    for cl in b.cleanup:                     # (row against table row: atol 2e-6)
        bound[cl["dst"]:cl["dst"] + cl["cols"]] = CLEANUP_ATOL
    if not np.isfinite(sig1[mask]).all():
        failures.append((-1, "signals not finite"))
    ratio = _ratio(diff, bound)
    for lo, hi in _ranges(mask):
        w = c.writer[lo:hi]
        for j in np.unique(w):
            m = np.flatnonzero(w == j) + lo
            kind = str(kinds[j])
            _worst(rep["kind"], kind, ratio[m].max())
            _worst(rep["region"], "sig %d:%d %s" % (m[0], m[-1] + 1, kind), ratio[m].max())
            if kind != "cleanup":
                tight(kind, diff[m], bound[m])
    # a flipped marginal decision skips the comparison of values: whatever lies behind it in program order differs legitimately.  A
    # decision that differs on an item that is NOT marginal, at or before the first flipped operator, cannot come from the flip: it stays.
    rep["skipped"] = bool(flips)
    first = min(flips) if flips else len(model.ops)
    rep["failures"] = [text for op, text in failures if op <= first]
    rep["ignored"] = [text for op, text in failures if op > first]
    rep["worst"] = max(rep["kind"].values(), default=0.0)
    rep["ok"] = not rep["failures"] and (rep["skipped"] or rep["worst"] <= 1.0)
    return rep


def run_points(model, sim, points, max_skips=1, **kw):
    """``points``: values of n_steps at which a restart step is checked (the step from n_steps to n_steps + 1); in between the
    device advances with one ordinary ``run_steps`` call per gap.  -> summary with ``ok``."""
    reports = []
    for p in sorted(points):
        assert p >= sim.n_steps, (p, sim.n_steps)
        if p > sim.n_steps:
            sim.run_steps(p - sim.n_steps)
        reports.append(check_restart_step(model, sim, **kw))
    return summarize(reports, max_skips)


def summarize(reports, max_skips=1):
    s = dict(points=[r["step"] for r in reports], kind={}, region={}, failures=[], skipped=0, skip_reasons=[], tight={},
             marginal=dict(neurons=0, cleanup=0, gate=0), live=dict(pes=0, voja=0, gate_open=0, voja_rows=0, pes_inc=0.0))
    for r in reports:
        s["failures"] += ["step %d: %s" % (r["step"], f) for f in r["failures"]]
        for k in r["marginal"]:
            s["marginal"][k] += r["marginal"][k]
        for k in ("pes", "voja", "gate_open", "voja_rows"):
            s["live"][k] += int(r["live"][k])
        s["live"]["pes_inc"] = max(s["live"]["pes_inc"], r["live"]["pes_inc"])
        if r["skipped"]:
            s["skipped"] += 1
            s["skip_reasons"] += ["step %d: %s" % (r["step"], x) for x in r["skip_reasons"]]
            continue
        for name in ("kind", "region"):
            for k, v in r[name].items():
                _worst(s[name], k, v)
        for k, v in r["tight"].items():
            s["tight"].setdefault(k, []).extend(v)
    s["worst"] = max(s["kind"].values(), default=0.0)
    s["tightness"] = {k: float(np.median(np.concatenate(v))) for k, v in s["tight"].items()}
    del s["tight"]
    s["ok"] = not s["failures"] and s["worst"] <= 1.0 and s["skipped"] <= max_skips
    return s


def describe(summary, label=""):
    over = {k: v for k, v in summary["region"].items() if v > 1.0}
    return ("%s points %s worst %.3g by kind %s marginal %s skipped %d %s live %s tightness %s failures %s over the bound %s"
            % (label, summary["points"], summary["worst"], {k: round(v, 4) for k, v in summary["kind"].items()}, summary["marginal"],
               summary["skipped"], summary["skip_reasons"], summary["live"], {k: round(v, 1) for k, v in summary["tightness"].items()},
               summary["failures"][:6], over))


# ---- the NumPy stand-in ------------------------------------------------------------------------------------------------------
class OracleDevice:
    """``OracleSimulator(model, dtype)`` behind the few methods of ``Simulator`` the checks use, stepping ONE operator at a time
    through the oracle's own ``step`` so that a CPU test can wrap one: ``wrap = {operator index: fn(dev, o, apply)}`` replaces the
    operator by ``fn``, which may call ``apply(o2)`` with an altered operator and edit ``dev.o.sig`` / ``dev.o.buf`` around it.
    ``dev.start[-1]`` / ``dev.start[-2]``: the signal vector at the start of this / of the previous step.  ``after_step(dev)`` runs
    behind the last operator."""

    def __init__(self, model, dtype=np.float32, wrap=None, after_step=None):
        self.model, self.wrap, self.after_step = model, dict(wrap or {}), after_step
        self.o = OracleSimulator(model, dtype=dtype)
        self.start = [self.o.sig.copy(), self.o.sig.copy()]
        self.active = True                   # (a test switches a mutation on for the checked steps only)

    @property
    def n_steps(self):
        return self.o.n_steps

    def read_signal(self, off, count):
        return np.array(self.o.sig[off:off + count], dtype=np.float64)

    def read_buffer(self, buffer_id):
        return np.array(self.o.buf[buffer_id], dtype=np.float64)

    def write_buffer(self, buffer_id, values):
        self.o.buf[buffer_id][...] = np.asarray(values).reshape(self.o.buf[buffer_id].shape)

    def run_steps(self, n):
        for _ in range(int(n)):
            self.start = [self.start[1], self.o.sig.copy()]
            self.o.n_steps += 1
            apply = _single_op_runner(self.o)
            for j, o in enumerate(self.model.ops):
                if self.active and j in self.wrap:
                    self.wrap[j](self, o, apply)
                else:
                    apply(o)
            if self.active and self.after_step is not None:
                self.after_step(self)


# ---- the models of the CPU and GPU tests -------------------------------------------------------------------------------------
def with_decision_probes(sm):
    """Probes on the clean-up and the gate nodes: their outputs become part of the carried set, so a device has to show them."""
    with sm.model:
        nengo.Probe(sm.slam.gridcells)
        nengo.Probe(sm.slam.update_state)
    return sm


def small_slam():
    """``_small_slam`` of tests/test_gpu_parity.py (d = 55, 15 200 neurons) with the decision probes -> (SlamModel, BuiltModel)."""
    s = H.make_ssp_space(2, 55)
    path, vels = H.make_random_path(20.0, limit=0.1, seed=0)
    sm = with_decision_probes(H.make_slam_model(s, path, vels, n_landmarks=10, pi_n_neurons=100, mem_n_neurons=300,
                                                circonv_n_neurons=50, view_rad=0.6, weights_sample_every=None))
    return sm, build_model(sm.model)
