"""The instrument of the time-batched stage tests (tests only; neither a test module nor a conftest).

The feed-forward half of every model runs a block of B timesteps at a time through a runtime of its own: ``stages.py`` marks the
operators, ``stage::optimise`` / ``stage::pack`` / ``stage::ZeroMap`` (csrc/ssn_stage_plan.hpp; ``Sim::run_batch`` of
csrc/ssn_host.hip walks what they planned) order, pack and zero-skip them, ``stage::kernel_for`` picks ``kb_gemm`` /
``kb_gemm_mfma_f32`` and ``kb_lowpass`` / ``kb_lowpass_chunked`` for ``launch_batch_op`` (csrc/ssn_kernels.hpp), row B of the block
buffer becomes row 0 of the next block.  Here every operator of such a stage, at every step, is held to a float64 evaluation of the same
operator list under a first-order bound, on models without neurons (every operator has ``stage == 2`` and the device reports
``launches_per_step == 0``: all it computes runs time-batched).

The models (``products_model``, ``scans_model``, ``elementwise_model``, ``chain_model``, ``zero_model``, ``probes_model``)
    table-driven Nodes (``Rows``: the row of step s is test vector s - first, zeros outside the window; every value is made as float32
    and widened, so the device sees what the reference sees) feed passthrough Nodes through ``Connection(transform=, synapse=)``; every
    Node is probed.  Transforms come from a seeded RNG (no DFT matrix).  A connection with a synapse is a product into a temporary
    (``set``), a scan, and a hand-off that reads the scan's state with ``src_prev = 1``; without one it is a product or a sum onto the
    node input (``inc``).  A product whose OWN source is a previous-row read cannot be written in the frontend: ``delay_product`` moves a
    built product in front of the table operator it reads and sets its ``src_prev`` - the operator list then says y(t) += W u(t - 1),
    which the oracle (step order) and the device (``border`` order and the flag) both execute.

The float64 evaluator (``evaluate``)
    walks ``model.ops`` in ``border`` order, every operator for all timesteps at once (a scan is a loop along time), reading row t or,
    under ``src_prev``, row t - 1; row 0 is ``sig_init``.  tests/test_stages.py holds it to ``OracleSimulator`` (which steps the list in
    step order) at 1e-12.  Beside every element of every step it carries the bound of tests/slam_restart.py, whose rules are imported,
    not copied: fill / table ``u |value|``; axpy ``2 u |t| + |alpha| b(x)`` (set), ``3 u (|dst| + |t|) + b(dst) + |alpha| b(x)`` (inc);
    matvec ``_product_bound`` plus the input bounds through ``min(|W| b, LAMBDA sqrt(W^2 b^2))``, ``inc`` adds ``b(dst) + u (|dst| +
    |y|)``; lowpass ``b <- |a| b + |(1 - a) gain| b(x) + 3 u (|a y| + |(1 - a) gain x|)``.  Everything is compared under ``bound + 2 u
    |value|``.  u = 2^-24; the rules are linear in u, so the f64 kernels are held to the same figures times 2^-29 (u = 2^-53), against
    the evaluator run in extended precision (``np.longdouble``) so that the reference's own rounding stays outside the comparison.
    No constant is fitted to the device.

The chunked scan's own term
    ``kb_lowpass_chunked`` (f32, B >= 256) cuts a block into 32 chunks of per = ceil(B / 32) steps.  Chunk c runs from a ZERO state to
    L_c (z <- a z + b x: the sequential rule on z, not on y - |z| may exceed |y|), forms p_c = a^n_c by n_c multiplications beginning
    at 1 (n_c - 1 roundings and n_c times the rounding of the coefficient: |p_c - a^n_c| <= 2 n_c u a^n_c), chains the carries
    C_{c+1} = fl(fl(p_c C_c) + L_c), and re-runs the chunk from C_c under the sequential rule.  So, for the state C_c at the start of
    chunk c:   b(C_{c+1}) = a^n b(C_c) + 2 n u |a^n C_c| + b(L_c) + u |a^n C_c| + u |C_{c+1}|,   b(C_0) = the bound of row 0,
    and the outputs of chunk c follow the sequential recursion started at b(C_c); input bounds enter L_c (for later chunks) and the
    re-run (for this chunk) once each.  Empty trailing chunks (B = 257: per = 9, chunks 29 .. 31) multiply nothing.  ``evaluate(...,
    cuts=)`` applies this per block of 256 steps or more; the sequential kernels and f64 keep the plain recursion.

The stand-in (``StandIn``)
    NumPy float32 restatement of what the kernels do: the stage's operators cut, levelled, sorted and re-joined as ``stage::optimise``
    does (``optimise``; the GPU tests hold it to the library's own listing under SSN_DEBUG_PLAN), packed into lists of at most 24 as
    ``stage::pack`` does (``pack``), with the zero map of ``stage::ZeroMap`` (``zero_walk``) - tests/test_stage_plan.py holds the
    header itself to these three, ``hazard`` and ``dispatch`` on a CPU; a k-sequential fused-multiply-add chain per output element for
    both GEMMs; the sequential scan and the 32-chunk scan with its ``pw`` products; one persistent block buffer whose row B is copied to row 0; ``src_prev``.  It
    proves that the bars hold and are not slack (tests/test_stages.py: error <= half a bar everywhere, median bound / error <= 64 per
    operator kind), and its switches are the wrong devices (``MUTANTS``) that each have to fail a case of the GPU module's list.

``dispatch`` restates the choice of kernel (``stage::kernel_for``); ``parse_listing`` reads the ``[ssn]   batch op kind ...`` lines.
``expected_skips`` derives ``batch_products_skipped`` from input windows and block cuts alone.
"""
import contextlib
import functools
import os
import re

import numpy as np

import sspslam_amd.frontend as nengo
from sspslam_amd.builder import build as build_model

from slam_restart import LAMBDA, U, _product_bound

U64 = 2.0 ** -53
DT = 0.001
K_FILL, K_AXPY_INC, K_AXPY_SET, K_LOWPASS, K_TABLE, K_MATVEC_INC, K_MATVEC_SET, K_PROBE = 1, 2, 3, 4, 5, 6, 7, 11     # ssn::MicroKind
ELEMENTWISE = {K_FILL, K_AXPY_INC, K_AXPY_SET, K_TABLE, K_PROBE}
WRITES = {K_FILL, K_AXPY_INC, K_AXPY_SET, K_LOWPASS, K_TABLE, K_MATVEC_INC, K_MATVEC_SET}
READS = {K_AXPY_INC, K_AXPY_SET, K_LOWPASS, K_MATVEC_INC, K_MATVEC_SET, K_PROBE}
PRODUCTS = {K_MATVEC_INC, K_MATVEC_SET}
MAX_BATCH_OPS, MULTI_ROWS, MAX_PIECES, CHUNKS, CHUNKED_FROM = 24, 8, 32, 32, 256



@contextlib.contextmanager
def environment(**env):
    for k in env:
        os.environ.pop(k, None)
    os.environ.update({k: v for k, v in env.items() if v is not None})
    try:
        yield
    finally:
        for k in env:
            os.environ.pop(k, None)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
class Rows:
    """Node function of a table: the row of (1-based) step s is ``X[s - first]`` for first <= s < first + len(X), zeros elsewhere."""

    def __init__(self, X, first=1):
        self.X, self.first = np.asarray(X, dtype=np.float64), int(first)

    def row(self, s):
        j = s - self.first
        return self.X[j] if 0 <= j < len(self.X) else np.zeros(self.X.shape[1])

    def __call__(self, t):
        return self.row(int(round(t / DT)))

    def stored(self, steps):
        """Which of these steps have a row in the device's table (``tabulate``: a row of zeros is not stored)."""
        return np.array([bool(np.any(self.row(int(s)))) for s in steps])


class StoredRows(Rows):
    """The same through the vectorised provider interface (``fn.table``): EVERY step gets a stored row, rows of zeros included."""

    def table(self, steps):
        return np.array([self.row(int(s)) for s in steps]).reshape(len(steps), -1), np.arange(len(steps), dtype=np.int32)

    def stored(self, steps):
        return np.ones(len(steps), dtype=bool)


def f32_values(rng, shape, scale=1.0):
    return (scale * rng.uniform(-1.0, 1.0, shape)).astype(np.float32).astype(np.float64)


def cuts_of(block, calls):
    """Block lengths of ``run_steps(n) for n in calls`` at block length ``block``: every call starts a block of its own."""
    out = []
    for n in calls:
        out += [block] * (n // block) + ([n % block] if n % block else [])
    return out


def ragged(block):
    """Three blocks with a ragged last one (two seams)."""
    return 2 * block + max(1, block // 2) + (1 if block > 2 else 0)


# ---- the stage's operators as the device sees them -----------------------------------------------------------------------------
def batch_ops(model):
    """``BatchOp`` records of the (only) stage in ``border`` order, the probe samples behind them (plan(), csrc/ssn_host.hip)."""
    out = []
    for j, o in sorted(enumerate(model.ops), key=lambda jo: jo[1]["border"]):
        k = o["kind"]
        b = dict(op=j, dst=int(o.get("dst", 0)), src=int(o.get("src", 0)), cols=0, prev=int(o.get("src_prev", 0)), a=0.0, b=0.0)
        if k == "fill":
            b.update(kind=K_FILL, len=o["len"], a=o["value"])
        elif k == "table":
            b.update(kind=K_TABLE, len=o["width"], table=o["table"])
        elif k == "axpy":
            b.update(kind=K_AXPY_SET if o["mode"] == "set" else K_AXPY_INC, len=o["len"], a=o["alpha"])
        elif k == "lowpass":
            b.update(kind=K_LOWPASS, len=o["len"], a=o["a"], b=(1.0 - o["a"]) * o["gain"])
        elif k == "matvec":
            b.update(kind=K_MATVEC_SET if o["mode"] == "set" else K_MATVEC_INC, len=o["rows"], cols=o["cols"], w=o["w"])
        else:
            raise ValueError("operator %r cannot run in a time-batched stage" % k)
        out.append(b)
    for i, p in enumerate(model.probes):
        out.append(dict(op=-1, kind=K_PROBE, dst=0, src=int(p["src"]), len=int(p["width"]), cols=0, prev=0, a=0.0, b=0.0, probe=i))
    return out


def _read_len(o):
    return o["cols"] if o["kind"] in PRODUCTS else o["len"]


def hazard(a, b):
    """``stage::hazard``: 0 none; 1 only on elements both touch at the same index of the same row (two element-wise operators may then
    share a launch); 2 anything else."""
    kind = 0

    def pair(x, xl, y, yl, prev):
        nonlocal kind
        if x < y + yl and y < x + xl:
            kind = max(kind, 1 if (x == y and not prev) else 2)
    aw, bw, ar, br = a["kind"] in WRITES, b["kind"] in WRITES, a["kind"] in READS, b["kind"] in READS
    if aw and bw:
        pair(a["dst"], a["len"], b["dst"], b["len"], False)
    if aw and br:
        pair(a["dst"], a["len"], b["src"], _read_len(b), bool(b["prev"]))
    if ar and bw:
        pair(a["src"], _read_len(a), b["dst"], b["len"], bool(a["prev"]))
    if kind == 1 and not (a["kind"] in ELEMENTWISE and b["kind"] in ELEMENTWISE):
        kind = 2
    return kind


def optimise(ops, real=np.float32):
    """``stage::optimise``: resets and sums cut at the range endpoints of the other operators (kept whole beyond 32 pieces), every
    operator at the earliest level its hazards allow, sorted by level and class, neighbouring scans with equal coefficients joined."""
    if len(ops) < 2:
        return [dict(o) for o in ops]
    pts = set()
    for o in ops:
        if o["kind"] in WRITES:
            pts |= {o["dst"], o["dst"] + o["len"]}
        if o["kind"] in READS:
            pts |= {o["src"], o["src"] + _read_len(o)}
    cut = []
    for o in ops:
        axpy = o["kind"] in (K_AXPY_INC, K_AXPY_SET)
        if not (axpy or o["kind"] == K_FILL) or o["len"] <= 1:
            cut.append(dict(o))
            continue
        offs = {0, o["len"]}
        for base in (o["dst"], o["src"] if axpy else o["dst"]):
            offs |= {p - base for p in pts if base < p < base + o["len"]}
        offs = sorted(offs)
        if len(offs) > MAX_PIECES:
            cut.append(dict(o))
            continue
        for lo, hi in zip(offs, offs[1:]):
            cut.append(dict(o, dst=o["dst"] + lo, len=hi - lo, src=o["src"] + lo if axpy else o["src"]))
    level = [0] * len(cut)
    for j in range(len(cut)):
        for i in range(j):
            if level[i] + 1 > level[j] and hazard(cut[i], cut[j]):
                level[j] = level[i] + 1
    cls = lambda o: 0 if o["kind"] in ELEMENTWISE else 1 if o["kind"] == K_LOWPASS else 2
    order = sorted(range(len(cut)), key=lambda k: (level[k], cls(cut[k]), cut[k]["dst"] if cut[k]["kind"] == K_LOWPASS else 0))
    out, last = [], -1
    for k in order:
        o = cut[k]
        p = out[-1] if out else None
        if (p is not None and level[k] == last and o["kind"] == K_LOWPASS and p["kind"] == K_LOWPASS and real(p["a"]) == real(o["a"])
                and real(p["b"]) == real(o["b"]) and p["prev"] == o["prev"] and p["dst"] + p["len"] == o["dst"]
                and p["src"] + p["len"] == o["src"]):
            p["len"] += o["len"]
            continue
        out.append(dict(o))
        last = level[k]
    return out


def pack(ops, stage_batch=True, drop_overflow=False):
    """The launches of ``stage::pack``: [('list', [operators])] for consecutive element-wise operators without a cross-thread hazard, at most
    24 to a list, [('op', operator)] for everything else (a list of one is an ordinary launch).  ``drop_overflow``: the wrong device
    that loses the operator a full list has no slot for."""
    out, i = [], 0
    while i < len(ops):
        if ops[i]["kind"] in ELEMENTWISE and stage_batch:
            lst, j = [ops[i]], i + 1
            while j < len(ops) and len(lst) < MAX_BATCH_OPS and ops[j]["kind"] in ELEMENTWISE:
                if any(hazard(q, ops[j]) == 2 for q in lst):
                    break
                lst.append(ops[j])
                j += 1
            if drop_overflow and len(lst) == MAX_BATCH_OPS and j < len(ops) and ops[j]["kind"] in ELEMENTWISE \
                    and not any(hazard(q, ops[j]) == 2 for q in lst):
                j += 1
            if len(lst) > 1:
                out.append(("list", lst))
                i = j
                continue
        out.append(("op", ops[i]))
        i += 1
    return out


def zero_walk(ops, table_zero_per_block, zero_skip=True, skip_prev=False, inc_as_set=False):
    """The zero map of ``run_batch`` (``stage::ZeroMap``) over the operators a block executes, in order: which signal elements are zero
    in every row of the block, and the products that are therefore not multiplied out.  ``table_zero_per_block``: per block {table
    id: the table has no stored row in the block}.  -> per block {index of a skipped product: its rows are marked zero (a ``set``)}.
    ``skip_prev`` / ``inc_as_set``: the wrong devices that skip a previous-row product / clear the rows of a skipped increment."""
    n = max([0] + [o["dst"] + o["len"] for o in ops] + [o["src"] + _read_len(o) for o in ops])
    out = []
    for table_zero in table_zero_per_block:
        zero = np.zeros(n, dtype=bool)
        all_zero = lambda lo, k: k > 0 and bool(zero[lo:lo + k].all())
        skipped = {}
        for i, o in enumerate(ops):
            k, d = o["kind"], slice(o["dst"], o["dst"] + o["len"])
            if not zero_skip:
                continue
            if k in PRODUCTS and (not o["prev"] or skip_prev) and all_zero(o["src"], o["cols"]):
                skipped[i] = k == K_MATVEC_SET or inc_as_set
                if skipped[i]:
                    zero[d] = True
                continue
            if k == K_TABLE:
                zero[d] = bool(table_zero[o["table"]])
            elif k == K_FILL:
                zero[d] = o["a"] == 0
            elif k == K_AXPY_SET:
                zero[d] = (not o["prev"]) and all_zero(o["src"], o["len"])
            elif k == K_AXPY_INC:
                if o["prev"] or not all_zero(o["src"], o["len"]):
                    zero[d] = False
            elif k != K_PROBE:
                zero[d] = False
        out.append(skipped)
    return out


def plan_key(ops):
    """What a listing line carries, for every operator but the probe samples' pointers: (kind, dst, src, len, cols, prev)."""
    return [(o["kind"], o["dst"], o["src"], o["len"], o["cols"], o["prev"]) for o in ops]


def parse_listing(err):
    """The ``[ssn]   batch op kind`` lines of an SSN_DEBUG_PLAN listing -> [(kind, dst, src, len, cols, prev)]."""
    return [tuple(int(v) for v in m.groups()) for m in
            re.finditer(r"^\[ssn\]   batch op kind (\d+) dst (-?\d+) src (-?\d+) len (\d+) cols (\d+) prev (\d+)$", err, re.M)]


def dispatch(kind, length, cols, B, f32=True):
    """``stage::kernel_for``: the kernel one operator of a block of B steps goes to (None: nothing is launched)."""
    if B <= 0 or length <= 0:
        return None
    if kind == K_LOWPASS:
        return "kb_lowpass_chunked" if f32 and B >= CHUNKED_FROM else "kb_lowpass"
    if kind in PRODUCTS:
        return "kb_gemm_mfma_f32" if f32 and cols >= 64 and length >= 32 and B >= 32 else "kb_gemm"
    return "kb_elementwise"


def reached(listing, blocks, f32=True):
    """{kernel: set of (len, cols, B)} that the operators of a listing reach over these block lengths."""
    out = {}
    for kind, _, _, length, cols, _ in listing:
        for B in set(blocks):
            k = dispatch(kind, length, cols, B, f32)
            if k:
                out.setdefault(k, set()).add((length, cols, B))
    return out


def expected_skips(products, cuts):
    """``batch_products_skipped`` from input windows alone.  ``products``: one ``Rows`` per product that reads (without ``src_prev``)
    nothing but that table or sums of it; a product is skipped in every block in which its table has no stored row."""
    n, s0 = 0, 0
    for B in cuts:
        steps = range(s0 + 1, s0 + B + 1)
        n += sum(1 for rows in products if not rows.stored(steps).any())
        s0 += B
    return n


# ---- the float64 evaluator with its bound ------------------------------------------------------------------------------------
class Evaluation:
    """``V[t]``, ``B[t]``: value and bound (u = 2^-24) of every signal element after step t (row 0: the initial state);
    ``kind[i]``: kind of the last operator that writes element i."""


def _scan_plain(a, bc, y, by, X, bX, Y, BY):
    for t in range(len(X)):
        t1, t2 = a * y, bc * X[t]
        by = abs(a) * by + abs(bc) * bX[t] + 3 * U * (np.abs(t1) + np.abs(t2)).astype(np.float64)
        y = t1 + t2
        Y[t], BY[t] = y, by


def _scan_chunked(a, bc, y, by, X, bX, Y, BY):
    """One block of ``kb_lowpass_chunked`` (module docstring): values as the plain scan's, bounds by the kernel's arithmetic."""
    B = len(X)
    per = (B + CHUNKS - 1) // CHUNKS
    C, bC = y, by
    for c in range(CHUNKS):
        t0 = min(B, c * per)
        t1 = min(B, t0 + per)
        n = t1 - t0
        if n == 0:
            break
        _scan_plain(a, bc, C, bC, X[t0:t1], bX[t0:t1], Y[t0:t1], BY[t0:t1])
        z, ez = np.zeros_like(C), np.zeros(C.shape)
        for t in range(t0, t1):
            t1_, t2_ = a * z, bc * X[t]
            ez = abs(a) * ez + abs(bc) * bX[t] + 3 * U * (np.abs(t1_) + np.abs(t2_)).astype(np.float64)
            z = t1_ + t2_
        p = a ** n
        Cn = Y[t1 - 1]                                                 # (= p C + z in exact arithmetic)
        bC = p * bC + ez + ((2 * n + 1) * U * np.abs(p * C) + U * np.abs(Cn)).astype(np.float64)
        C = Cn


def evaluate(model, n_steps, cuts=None, real=np.float64):
    """-> Evaluation of steps 1 .. n_steps.  ``cuts``: the block lengths of an f32 run; blocks of 256 steps or more then carry the
    chunked scan's bound, everything else does not depend on the cuts (a prefix of a longer evaluation is the evaluation of a shorter
    run).  ``real``: the arithmetic of the values (np.longdouble to judge the f64 kernels); bounds are float64."""
    N, n = int(n_steps), int(model.sig_size)
    V = np.empty((N + 1, n), dtype=real)
    V[:] = np.asarray(model.sig_init, dtype=real)[None, :]
    Bd = np.zeros((N + 1, n))
    kind = np.full(n, "none", dtype=object)
    f64 = lambda x: np.asarray(x, dtype=np.float64)
    for o in sorted(model.ops, key=lambda o: o["border"]):
        assert o["stage"] == 2, o
        k = o["kind"]
        rows = slice(0, N) if o.get("src_prev") else slice(1, N + 1)
        exact_before = np.asarray(V[1:, o["dst"]:o["dst"] + o["len"]] != 0) if k == "axpy" else None
        if k == "fill":
            d = slice(o["dst"], o["dst"] + o["len"])
            V[1:, d] = o["value"]
            Bd[1:, d] = U * abs(o["value"])
        elif k == "table":
            d = slice(o["dst"], o["dst"] + o["width"])
            fn = model.tables[o["table"]]["fn"]
            V[1:, d] = np.array([np.asarray(fn(s * model.dt), dtype=np.float64).reshape(-1) for s in range(1, N + 1)]).reshape(N, -1)
            Bd[1:, d] = U * np.abs(f64(V[1:, d]))
        elif k == "axpy":
            d, s = slice(o["dst"], o["dst"] + o["len"]), slice(o["src"], o["src"] + o["len"])
            t = o["alpha"] * V[rows, s]
            if o["mode"] == "set":
                Bd[1:, d] = 2 * U * np.abs(f64(t)) + abs(o["alpha"]) * Bd[rows, s]
                V[1:, d] = t
            else:
                Bd[1:, d] = 3 * U * (np.abs(f64(V[1:, d])) + np.abs(f64(t))) + Bd[1:, d] + abs(o["alpha"]) * Bd[rows, s]
                V[1:, d] = V[1:, d] + t
        elif k == "matvec":
            assert not o.get("dft"), o
            W = np.asarray(model.buffers[o["w"]], dtype=np.float64)
            d, s = slice(o["dst"], o["dst"] + o["rows"]), slice(o["src"], o["src"] + o["cols"])
            X, bX = V[rows, s], Bd[rows, s]
            Y = X @ np.asarray(W, dtype=real).T
            by = np.array([_product_bound(W, x) for x in f64(X)])
            by += np.minimum(bX @ np.abs(W).T, LAMBDA * np.sqrt((bX * bX) @ (W * W).T))
            if o["mode"] != "set":
                by += Bd[1:, d] + U * (np.abs(f64(V[1:, d])) + np.abs(f64(Y)))
                Y = V[1:, d] + Y
            V[1:, d], Bd[1:, d] = Y, by
        elif k == "lowpass":
            d, s = slice(o["dst"], o["dst"] + o["len"]), slice(o["src"], o["src"] + o["len"])
            a, bc = real(o["a"]), real((1.0 - o["a"]) * o["gain"])
            X, bX = V[rows, s].copy(), Bd[rows, s].copy()
            Y, BY = np.empty((N, o["len"]), dtype=real), np.empty((N, o["len"]))
            t0 = 0
            for B in (cuts if cuts is not None else [N]):
                B = min(B, N - t0)
                if B <= 0:
                    break
                y, by = (V[0, d], Bd[0, d]) if t0 == 0 else (Y[t0 - 1], BY[t0 - 1])
                scan = _scan_chunked if (cuts is not None and B >= CHUNKED_FROM) else _scan_plain
                scan(a, bc, y.copy(), by.copy(), X[t0:t0 + B], bX[t0:t0 + B], Y[t0:t0 + B], BY[t0:t0 + B])
                t0 += B
            assert t0 == N, (t0, N, cuts)
            V[1:, d], Bd[1:, d] = Y, BY
        else:
            raise ValueError("operator %r cannot run in a time-batched stage" % k)
        w = o["width"] if k == "table" else o["rows"] if k == "matvec" else o["len"]
        if k == "axpy" and abs(o["alpha"]) == 1.0 and o["mode"] != "set" and not exact_before.any():
            kind[o["dst"]:o["dst"] + w] = kind[o["src"]:o["src"] + w]      # a hand-off onto a reset: the source's values, the source's kind
        else:
            kind[o["dst"]:o["dst"] + w] = k
    ev = Evaluation()
    ev.V, ev.B, ev.kind, ev.n_steps = V, Bd, kind, N
    return ev


def judge(model, ev, data, u=U, tight=None):
    """Every element of every step of every unsampled probe against the evaluation, under ``bound + 2 u |value|`` -> {probe index:
    (worst |device - float64| / bar, step, element)}.  ``data[i]``: the (steps, width) rows of probe i.  ``tight``: a dict that collects
    bar / error of every element the device did not get exactly, per kind of the last writer."""
    out = {}
    scale = u / U
    for i, p in enumerate(model.probes):
        if p["every"] != 1:
            continue
        got = np.asarray(data[i], dtype=ev.V.dtype)
        n = got.shape[0]
        assert n <= ev.n_steps and got.shape[1] == p["width"], (i, got.shape, ev.n_steps)
        s = slice(p["src"], p["src"] + p["width"])
        want = ev.V[1:n + 1, s]
        diff = np.abs(np.asarray(got - want, dtype=np.float64))
        bar = scale * ev.B[1:n + 1, s] + 2 * u * np.abs(np.asarray(want, dtype=np.float64))
        assert np.isfinite(np.asarray(got, dtype=np.float64)).all(), "probe %d: not finite" % i
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(diff == 0, 0.0, diff / bar)
        j = int(np.argmax(r)) if r.size else 0
        out[i] = (float(r.max()) if r.size else 0.0, j // p["width"] + 1 if r.size else 0, j % p["width"] if r.size else 0)
        if tight is not None:
            for k in set(ev.kind[s]):
                m = (diff > 0) & (ev.kind[s] == k)[None, :]
                if m.any():
                    tight.setdefault(k, []).append(bar[m] / diff[m])
    return out


def worst(report):
    return max((r[0] for r in report.values()), default=0.0)


def tightness(tight):
    return {k: float(np.median(np.concatenate(v))) for k, v in tight.items()}


# ---- the NumPy float32 stand-in ------------------------------------------------------------------------------------------------
MUTANTS = ("carry-row", "no-src-prev", "prev-product-skipped", "zero-map-kept", "inc-skipped-as-set", "memset-wide", "k-tail",
           "tile-edge", "chunk-power", "multi-tail", "op-25", "coefficient", "probe-early", "scan-tail")


def _fma(a, b, c):
    """fmaf on float32 arrays: the product is exact in float64, the sum rounds once more than the instruction (one case in 2^29)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


class StandIn:
    """``run_steps`` / ``data`` / ``counters`` of a float32 device that computes what the kernels compute (module docstring).
    ``mutant``: one of MUTANTS; ``zero_skip`` / ``reorder`` / ``stage_batch``: SSN_NO_ZERO_SKIP, SSN_NO_BATCH_REORDER and
    SSN_PLAN_NO_STAGE_BATCH, inverted."""

    def __init__(self, model, block, mutant=None, zero_skip=True, reorder=True, stage_batch=True, real=np.float32):
        assert mutant is None or mutant in MUTANTS, mutant
        self.model, self.block, self.mutant, self.zero_skip, self.stage_batch = model, int(block), mutant, zero_skip, stage_batch
        self.T = T = np.dtype(real).type                      # (float64: the parity mode - plain products and sums, no chunked scan)
        self.fma = _fma if T is np.float32 else (lambda a, b, c: a * b + c)
        ops = batch_ops(model)
        self.ops = optimise(ops, T) if reorder else ops
        self.R = np.tile(np.asarray(model.sig_init, dtype=T), (self.block + 1, 1))
        self.W = {o["w"]: np.asarray(model.buffers[o["w"]], dtype=T) for o in self.ops if o["kind"] in PRODUCTS}
        self.n_steps, self.skipped = 0, 0
        self.rows = [[] for _ in model.probes]
        self.kept_zero = {}

    def data(self):
        return [np.array(r, dtype=np.float64).reshape(len(r), p["width"]) for r, p in zip(self.rows, self.model.probes)]

    def counters(self):
        return dict(batch_products_skipped=self.skipped, launches_per_step=0)

    def run_steps(self, n):
        done = 0
        while done < n:
            B = min(self.block, n - done)
            self._block(B, self.n_steps)
            row = B - 1 if (self.mutant == "carry-row" and B > 1) else B
            self.R[0] = self.R[row]
            self.n_steps += B
            done += B

    # one block: run_batch
    def _table_zero(self, o, B, step0):
        fn = self.model.tables[o["table"]]["fn"]
        if self.mutant == "zero-map-kept":
            if o["table"] not in self.kept_zero:
                self.kept_zero[o["table"]] = not fn.stored(range(step0 + 1, step0 + B + 1)).any()
            return self.kept_zero[o["table"]]
        return not fn.stored(range(step0 + 1, step0 + B + 1)).any()

    def _block(self, B, step0):
        prev = lambda o: o["prev"] and self.mutant != "no-src-prev"
        launches = pack(self.ops, self.stage_batch, self.mutant == "op-25")
        executed = [o for what, item in launches for o in (item if what == "list" else [item])]
        tables = {o["table"]: self._table_zero(o, B, step0) for o in executed if o["kind"] == K_TABLE} if self.zero_skip else {}
        skipped = zero_walk(executed, [tables], self.zero_skip, self.mutant == "prev-product-skipped", self.mutant == "inc-skipped-as-set")[0]
        at = 0                                                      # index into `executed`
        for what, item in launches:
            if what == "list":
                for o in item:
                    self._elementwise(o, B, step0, prev(o), B - B % MULTI_ROWS if self.mutant == "multi-tail" else B)
                at += len(item)
                continue
            o, at = item, at + 1
            if at - 1 in skipped:
                self.skipped += 1
                if skipped[at - 1]:
                    wide = 1 if self.mutant == "memset-wide" else 0
                    self.R[1:B + 1, o["dst"]:o["dst"] + o["len"] + wide] = 0
                continue
            if o["kind"] in PRODUCTS:
                self._product(o, B, prev(o))
            elif o["kind"] == K_LOWPASS:
                self._scan(o, B, prev(o))
            else:
                self._elementwise(o, B, step0, prev(o), B)

    def _elementwise(self, o, B, step0, prev, rows):
        """Rows 1 .. rows of one element-wise operator (rows < B: the wrong device that drops the tail of the 8-row walk)."""
        k, R = o["kind"], self.R
        d = slice(o["dst"], o["dst"] + o["len"])
        s = slice(o["src"], o["src"] + o["len"])
        X = R[(0 if prev else 1):(rows if prev else rows + 1), s]
        if rows <= 0:
            return
        if k == K_FILL:
            R[1:rows + 1, d] = self.T(o["a"])
        elif k == K_TABLE:
            fn = self.model.tables[o["table"]]["fn"]
            R[1:rows + 1, d] = np.array([fn.row(step0 + t) for t in range(1, rows + 1)], dtype=self.T).reshape(rows, -1)
        elif k == K_AXPY_SET:
            R[1:rows + 1, d] = self.T(o["a"]) * X
        elif k == K_AXPY_INC:
            R[1:rows + 1, d] = self.fma(self.T(o["a"]), X, R[1:rows + 1, d])
        elif k == K_PROBE:
            every = self.model.probes[o["probe"]]["every"]
            for t in range(1, rows + 1):
                if (step0 + t) % every == 0:
                    self.rows[o["probe"]].append(np.array(R[t - 1 if self.mutant == "probe-early" else t, s], dtype=np.float64))

    def _product(self, o, B, prev):
        """A k-sequential fused-multiply-add chain per output element (kb_gemm's slabs and the matrix cores' accumulators alike)."""
        R, W = self.R, self.W[o["w"]]
        A = R[(0 if prev else 1):(B if prev else B + 1), o["src"]:o["src"] + o["cols"]]
        cols = o["cols"]
        if self.mutant == "k-tail" and cols % 32:
            cols -= cols % 32
        acc = np.zeros((B, o["len"]), dtype=self.T)
        for c in range(cols):
            acc = self.fma(A[:, c:c + 1], W[None, :, c], acc)
        if self.mutant == "tile-edge":
            for t in range(15, B - 1, 32):                         # rows 15 and 16 of every 32-row tile change places
                acc[[t, t + 1]] = acc[[t + 1, t]]
        d = slice(o["dst"], o["dst"] + o["len"])
        R[1:B + 1, d] = acc if o["kind"] == K_MATVEC_SET else R[1:B + 1, d] + acc

    def _scan(self, o, B, prev):
        R = self.R
        a = self.T(o["a"] + (1e-4 if self.mutant == "coefficient" else 0.0))
        b = self.T(o["b"])
        d = slice(o["dst"], o["dst"] + o["len"])
        X = R[(0 if prev else 1):(B if prev else B + 1), o["src"]:o["src"] + o["len"]].copy()
        step = lambda y, x: self.fma(a, y, b * x)
        if B < CHUNKED_FROM or self.T is not np.float32:
            y = R[0, d].copy()
            for t in range(B - B % 8 if self.mutant == "scan-tail" else B):
                y = step(y, X[t])
                R[t + 1, d] = y
            return
        per = (B + CHUNKS - 1) // CHUNKS
        carry = R[0, d].copy()
        for c in range(CHUNKS):
            t0 = min(B, c * per)
            t1 = min(B, t0 + per)
            y, z, pw = carry, np.zeros_like(carry), np.float32(1.0)
            for t in range(t0, t1):
                y = step(y, X[t])
                R[t + 1, d] = y
                z = step(z, X[t])
                pw = pw * a
            if self.mutant == "chunk-power" and t1 > t0:
                pw = np.float32(pw / a)
            carry = self.fma(pw, carry, z)


# ---- models ------------------------------------------------------------------------------------------------------------------
class Built:
    """``model``: the built model; ``probes``: {name: index into model.probes}; ``tables``: {name: Rows}; ``steps``: the longest run."""


def _finish(net, names, tables, steps, state_seed=None):
    model = build_model(net)
    assert all(o["stage"] == 2 for o in model.ops) and model.stage_info["enabled"], [o for o in model.ops if o["stage"] != 2][:3]
    assert not any(o["kind"] == "matvec" and o.get("dft") for o in model.ops)
    assert len(model.probes) == len(names)
    if state_seed is not None:                  # non-zero initial filter states (sig_init is what oracle, evaluator and device start from)
        rng = np.random.RandomState(state_seed)
        model.sig_init = np.array(model.sig_init, dtype=np.float64)
        for o in model.ops:
            if o["kind"] == "lowpass":
                model.sig_init[o["dst"]:o["dst"] + o["len"]] = f32_values(rng, o["len"])
    b = Built()
    b.model, b.probes, b.tables, b.steps = model, {n: i for i, n in enumerate(names)}, tables, steps
    return b


class _Net:
    """A network under construction: every Node is probed under its name."""

    def __init__(self, seed, steps):
        self.rng, self.steps, self.names, self.tables = np.random.RandomState(seed), steps, [], {}
        self.net = nengo.Network(seed=seed)

    def table(self, name, width, rows=None, first=1, scale=1.0, cls=Rows):
        X = f32_values(self.rng, (self.steps, width), scale) if rows is None else rows
        fn = cls(X, first)
        self.tables[name] = fn
        return self.node(name, nengo.Node(fn, size_out=width))

    def node(self, name, node=None, width=None, **probe):
        node = nengo.Node(size_in=width) if node is None else node
        nengo.Probe(node, **probe)
        self.names.append(name)
        return node

    def matrix(self, rows, cols):
        return self.rng.randn(rows, cols) / np.sqrt(cols)


PRODUCT_SHAPES = ((1, 129), (31, 65), (32, 65), (33, 63), (33, 64), (63, 31), (64, 33), (65, 1), (150, 100), (150, 32))
PRODUCT_BLOCKS = (1, 31, 32, 33, 63, 64, 65, 100)


@functools.lru_cache(maxsize=None)
def products_model():
    """Every (rows, cols) of PRODUCT_SHAPES as an ``inc`` product from a table; rows and cols sweep {1, 31, 32, 33, 63, 64, 65, 150} x
    {1, 31, 32, 33, 63, 64, 65, 100, 129}, and with the block lengths of PRODUCT_BLOCKS every threshold of ``launch_batch_op`` is met
    from both sides with the other two conditions true: cols 63 | 64 at (33 rows, B >= 32), rows 31 | 32 at (65 cols, B >= 32),
    B 31 | 32 at (33 x 64) and (150 x 100).  Beside them: a ``set`` product behind a synapse (150 x 100, tau 5 ms), a node that a table,
    a product and a product of a SLICED transform (33 rows from columns 3 .. 68 of a 33 x 70 matrix: an odd source origin, and rows
    padded to a leading dimension that is not the column count) add to in turn, and a product (70 x 65) behind a filtered node whose
    state is handed over with ``src_prev = 1``."""
    steps = ragged(max(PRODUCT_BLOCKS))
    n = _Net(11, steps)
    with n.net:
        src = {}
        for rows, cols in PRODUCT_SHAPES:
            if cols not in src:
                src[cols] = n.table("u%d" % cols, cols)
            tgt = n.node("y%dx%d" % (rows, cols), width=rows)
            nengo.Connection(src[cols], tgt, transform=n.matrix(rows, cols), synapse=None)
        tgt = n.node("set150x100", width=150)
        nengo.Connection(src[100], tgt, transform=n.matrix(150, 100), synapse=0.005)
        u70, t33 = n.table("u70", 70), n.table("t33", 33)
        tgt = n.node("inc33", width=33)
        nengo.Connection(t33, tgt, synapse=None)
        nengo.Connection(src[64], tgt, transform=n.matrix(33, 64), synapse=None)
        nengo.Connection(u70[3:68], tgt, transform=n.matrix(33, 70)[:, 3:68], synapse=None)
        mid = n.node("mid65", width=65)
        nengo.Connection(src[65], mid, synapse=0.002)
        tgt = n.node("behind70x65", width=70)
        nengo.Connection(mid, tgt, transform=n.matrix(70, 65), synapse=None)
    return _finish(n.net, n.names, n.tables, steps, state_seed=5)


SCAN_SHAPES = ((1, 0.001), (31, 0.002), (32, 0.005), (33, 0.01), (64, 0.03), (65, 0.1))
SCAN_BLOCKS = (1, 7, 8, 9, 63, 64, 255)
CHUNKED_BLOCKS = (256, 257, 263, 300, 511, 1000)
TAU_JOINED, TAU_APART = 0.007, (0.011, 0.013)


@functools.lru_cache(maxsize=None)
def scans_model(steps):
    """One filter per (element count, tau) of SCAN_SHAPES, from non-zero initial states; two filters of TAU_JOINED over adjacent halves
    of one source into adjacent halves of one node, and two of TAU_APART.  A tap on the first half of each source makes the stage
    split (``stages._split_elementwise``) cut at 17, so the model holds two scans per node: ``optimise_batch`` joins the equal pair
    and must keep the other apart."""
    n = _Net(12, steps)
    with n.net:
        for width, tau in SCAN_SHAPES:
            u = n.table("u%d" % width, width)
            nengo.Connection(u, n.node("f%d" % width, width=width), synapse=tau)
        for name, taus in (("joined", (TAU_JOINED, TAU_JOINED)), ("apart", TAU_APART)):
            u, f = n.table("u_" + name, 40), n.node("f_" + name, width=40)
            nengo.Connection(u[:17], f[:17], synapse=taus[0])
            nengo.Connection(u[17:], f[17:], synapse=taus[1])
            nengo.Connection(u[:17], n.node("tap_" + name, width=17), synapse=None)      # (a range endpoint at 17: the stage split cuts there)
    return _finish(n.net, n.names, n.tables, steps, state_seed=6)


ELEMENTWISE_BLOCKS = (1, 7, 8, 9, 13, 16, 17)
N_SOURCES = 26


@functools.lru_cache(maxsize=None)
def elementwise_model():
    """``sum``: a node of 40 that 26 tables of different widths add to (scaled sums of different lengths: more operators than a list
    holds); ``next``: the hand-off of that sum (reset / sums / hand-off on equal range origins: hazard class 1, one launch);
    ``filtered``: the same sum through a synapse (the previous-row read of its state breaks the chain: class 2); ``wide``: a node of 48
    that one table of 48 and 40 one-element sources add to, so the full-width reset and sum would be cut into more than 32 pieces."""
    steps = ragged(max(ELEMENTWISE_BLOCKS))
    n = _Net(13, steps)
    with n.net:
        total = n.node("sum", width=40)
        for i in range(N_SOURCES):
            w = 40 if i % 3 == 0 else 5 + i
            nengo.Connection(n.table("s%d" % i, w), total[:w], transform=float(np.float32(0.25 + 0.125 * i)), synapse=None)
        nengo.Connection(total, n.node("next", width=40), synapse=None)
        nengo.Connection(total, n.node("filtered", width=40), synapse=0.003)
        wide = n.node("wide", width=48)
        nengo.Connection(n.table("w48", 48), wide, synapse=None)
        one = n.table("ones", 40)
        for i in range(40):
            nengo.Connection(one[i], wide[i], transform=-1.5, synapse=None)
    return _finish(n.net, n.names, n.tables, steps)


@functools.lru_cache(maxsize=None)
def chain_model():
    """Few enough ranges that the reset is cut to line up with its consumers: reset / two sums / hand-off of ``sum`` on equal range
    origins share one launch (hazard class 1); ``filtered`` reads a filter state of the sum in the previous row (class 2)."""
    steps = ragged(max(ELEMENTWISE_BLOCKS))
    n = _Net(16, steps)
    with n.net:
        total = n.node("sum", width=21)
        nengo.Connection(n.table("p", 21), total, transform=0.75, synapse=None)
        nengo.Connection(n.table("q", 21), total, transform=-1.25, synapse=None)
        nengo.Connection(total, n.node("next", width=21), synapse=None)
        nengo.Connection(total, n.node("filtered", width=21), synapse=0.003)
    return _finish(n.net, n.names, n.tables, steps)


ZERO_BLOCK, ZERO_STEPS = 64, 300            # five blocks, the last one ragged


def delay_product(model, name_of_buffer_shape, table_id):
    """The product of matrix shape ``name_of_buffer_shape`` that reads table ``table_id`` is moved in front of the table operator in
    step order and reads the previous row: y(t) += W u(t - 1).  (Module docstring: no frontend construct says this.)"""
    ops = list(model.ops)
    tj = [j for j, o in enumerate(ops) if o["kind"] == "table" and o["table"] == table_id]
    assert len(tj) == 1
    tab = ops[tj[0]]
    mj = [j for j, o in enumerate(ops) if o["kind"] == "matvec" and o["src"] == tab["dst"] and o["cols"] == tab["width"]
          and np.shape(model.buffers[o["w"]]) == name_of_buffer_shape and o["mode"] == "inc"]
    assert len(mj) == 1 and mj[0] > tj[0], mj
    mv = dict(ops.pop(mj[0]), src_prev=1)
    assert all(o["kind"] != "fill" or j < tj[0] for j, o in enumerate(ops)), "the reset of the target has to stay in front"
    assert mv["border"] > tab["border"]
    ops.insert(tj[0], mv)
    model.ops = ops
    return mv


@functools.lru_cache(maxsize=None)
def zero_model():
    """Block length 64, 300 steps.  Tables: ``a`` non-zero in steps 70 .. 120 and 200 .. 250 only (blocks 1 and 3 of five); ``b`` whose
    only non-zero row is step 128, the last of block 1; ``c`` (StoredRows) whose stored rows are all zeros - they count as non-zero;
    ``d`` non-zero throughout; ``e`` non-zero up to step 128 and zero from block 2 on.  From a, b, c and d each: a ``set`` product
    (through a synapse) and an ``inc`` product.  a's ``set`` product is the last one made and reads a hand-off node: its temporary
    lies between c's temporary and the first filter state (d's, which ``d_set`` shows), and its reset runs a level behind the scans
    (the memset's width: one column more would clear that state behind its update); from e a product that reads the PREVIOUS row
    (``delay_product``): row 129 is W e(128) although e has no entry in that block."""
    steps = ZERO_STEPS
    n = _Net(14, steps)
    Xa = np.zeros((steps, 9))
    Xa[69:120], Xa[199:250] = f32_values(n.rng, (51, 9)), f32_values(n.rng, (51, 9))
    Xb = np.zeros((steps, 7))
    Xb[127] = f32_values(n.rng, 7)
    Xe = np.zeros((steps, 6))
    Xe[:128] = f32_values(n.rng, (128, 6))
    with n.net:
        a, b, e = n.table("a", 9, rows=Xa), n.table("b", 7, rows=Xb), n.table("e", 6, rows=Xe)
        c = n.table("c", 5, rows=np.zeros((steps, 5)), cls=StoredRows)
        d = n.table("d", 8)
        a_in = n.node("a_in", width=9)
        nengo.Connection(a, a_in, synapse=None)
        nengo.Connection(d, n.node("d_set", width=11), transform=n.matrix(11, 8), synapse=0.004)
        nengo.Connection(b, n.node("b_set", width=10), transform=n.matrix(10, 7), synapse=0.004)
        nengo.Connection(c, n.node("c_set", width=10), transform=n.matrix(10, 5), synapse=0.004)
        nengo.Connection(a_in, n.node("a_set", width=10), transform=n.matrix(10, 9), synapse=0.004)
        mix = n.node("mix", width=12)               # inc products onto one node, beside a table that is never zero
        nengo.Connection(d, mix, transform=n.matrix(12, 8), synapse=None)
        for t, w in ((a, 9), (b, 7), (c, 5)):
            nengo.Connection(t, mix, transform=n.matrix(12, w), synapse=None)
        nengo.Connection(e, n.node("delayed", width=13), transform=n.matrix(13, 6), synapse=None)
    built = _finish(n.net, n.names, n.tables, steps)
    delay_product(built.model, (13, 6), [i for i, t in enumerate(built.model.tables) if t["fn"] is n.tables["e"]][0])
    # the products the zero map may skip, by the table each depends on (the delayed one never: it reads a previous row)
    t = n.tables
    built.skippable = [t["d"], t["b"], t["c"], t["a"], t["d"], t["a"], t["b"], t["c"]]
    tmp = [o for o in built.model.ops if o["kind"] == "matvec" and o["mode"] == "set" and o["src"] == built.model.probes[built.probes["a_in"]]["src"]]
    first_state = min(o["dst"] for o in built.model.ops if o["kind"] == "lowpass")
    d_state = [o for o in built.model.ops if o["kind"] == "lowpass" and o["len"] >= 11 and o["dst"] == first_state]
    assert len(tmp) == 1 and tmp[0]["dst"] + tmp[0]["rows"] == first_state and d_state, "the layout the memset check relies on"
    return built


PROBE_RUNS = ((64, (100, 1, 199)), (256, (300, 301)))


@functools.lru_cache(maxsize=None)
def probes_model():
    """A filtered product and its input, each probed at every step, every 3rd and every 7th."""
    steps = max(sum(c) for _, c in PROBE_RUNS)
    n = _Net(15, steps)
    with n.net:
        u = n.table("u", 6)
        f = n.node("f", width=9)
        nengo.Connection(u, f, transform=n.matrix(9, 6), synapse=0.01)
        for name, target in (("u", u), ("f", f)):
            for every in (3, 7):
                n.node("%s/%d" % (name, every), target, sample_every=every * DT)
    return _finish(n.net, n.names, n.tables, steps)


# ---- the case list of the GPU module -----------------------------------------------------------------------------------------
class Case:
    """One run: ``family`` (products | scans | elementwise | chain | zero | probes), the model, the block length and the ``run_steps`` calls."""

    def __init__(self, family, built, block, calls):
        self.family, self.built, self.block, self.calls = family, built, int(block), tuple(calls)
        self.steps, self.cuts = sum(calls), cuts_of(block, calls)
        self.id = "%s-B%d-%s" % (family, block, "+".join(str(c) for c in calls))

    @property
    def model(self):
        return self.built().model

    def __repr__(self):
        return self.id


SCAN_STEPS = ragged(max(CHUNKED_BLOCKS))
the_scans_model = functools.partial(scans_model, SCAN_STEPS)
UNEVEN = (100, 1, 199)                          # at block 64: 64 + 36 | 1 | 64 + 64 + 64 + 7
CASES = ([Case("products", products_model, B, (ragged(B),)) for B in PRODUCT_BLOCKS]
         + [Case("scans", the_scans_model, B, (ragged(B),)) for B in SCAN_BLOCKS + CHUNKED_BLOCKS]
         + [Case("scans", the_scans_model, 64, UNEVEN)]
         + [Case("elementwise", elementwise_model, B, (ragged(B),)) for B in ELEMENTWISE_BLOCKS]
         + [Case("chain", chain_model, B, (ragged(B),)) for B in ELEMENTWISE_BLOCKS]
         + [Case("zero", zero_model, ZERO_BLOCK, (ZERO_STEPS,))]
         + [Case("probes", probes_model, B, calls) for B, calls in PROBE_RUNS])


@functools.lru_cache(maxsize=None)
def _evaluation(built, steps, cuts, real):
    ev = evaluate(built().model, steps, list(cuts) if cuts is not None else None, real)
    for a in (ev.V, ev.B):
        a.setflags(write=False)
    return ev


def evaluation(case, f32=True):
    """The evaluation a case is judged by, shared between the cases of a model: only a chunked scan's bound depends on the cuts, and
    a shorter run is a prefix of a longer one (f64 is judged against extended precision, module docstring)."""
    if not f32:
        return _evaluation(case.built, case.steps, None, np.longdouble)
    if case.family == "scans" and max(case.cuts) >= CHUNKED_FROM:
        return _evaluation(case.built, case.steps, tuple(case.cuts), np.float64)
    longest = max(c.steps for c in CASES if c.built is case.built and not (c.family == "scans" and max(c.cuts) >= CHUNKED_FROM))
    return _evaluation(case.built, max(longest, case.steps), None, np.float64)


def run_case(case, dev):
    for n in case.calls:
        dev.run_steps(n)
    return dev


def sampling_failures(case, data, tranges=None):
    """Probes with ``sample_every``: as many samples as ``trange(sample_every=)`` has times, sample k the unsampled probe's row of step
    every * (k + 1).  ``tranges``: {probe index: the device's trange for that probe} (the times themselves are then held to it)."""
    out = []
    model, names = case.model, case.built().probes
    for name, i in names.items():
        p = model.probes[i]
        if p["every"] == 1:
            continue
        full = np.asarray(data[names[name.split("/")[0]]])
        want_t = DT * p["every"] * np.arange(1, case.steps // p["every"] + 1)
        got = np.asarray(data[i])
        if got.shape != (len(want_t), p["width"]):
            out.append("probe %s: %s samples, expected %s" % (name, got.shape, (len(want_t), p["width"])))
            continue
        if tranges is not None and not np.array_equal(np.asarray(tranges[i]), want_t):
            out.append("probe %s: sample times differ from trange(sample_every=)" % name)
        rows = p["every"] * np.arange(1, len(want_t) + 1) - 1
        if not np.array_equal(got, full[rows]):
            out.append("probe %s: %d samples are not the unsampled probe's rows" % (name, int((got != full[rows]).any(axis=1).sum())))
    return out


def failures_of(case, dev, f32=True, tight=None):
    """Everything a case asks of a device that has run it -> (failures, worst |device - float64| / bar)."""
    data = dev.data()
    rep = judge(case.model, evaluation(case, f32), data, U if f32 else U64, tight)
    names = {i: n for n, i in case.built().probes.items()}
    out = ["probe %s: %.3g of the bar at step %d element %d" % (names[i], r, s, e) for i, (r, s, e) in rep.items() if not r <= 1.0]
    if case.family == "zero":
        want, got = expected_skips(case.built().skippable, case.cuts), dev.counters()["batch_products_skipped"]
        if got != want:
            out.append("batch_products_skipped %d, derived %d" % (got, want))
    if case.family == "probes":
        out += sampling_failures(case, data)
    return out, worst(rep)
