"""k_dft against the float64 matrices it replaces: every transform length 8..256 and the long ones, every engine, all five kinds,
``set`` and ``inc`` stores (tests/dft_checks.py is the instrument and derives the bar; tests/test_dft.py proves it on the CPU).

Every case asserts its route: ``counters()["fft_transforms"]`` and ``["fft_bluestein"]`` equal what the lengths imply, and the
planner's own listing under SSN_DEBUG_PLAN (one ``[ssn] dft`` line per transform, read from stderr) equals the Python restatement of
the planner that drives the stand-in - radices, M, in place or not, N1 x N2.  The figures are printed before they are asserted
(run with -s)."""
import contextlib
import functools
import os

import numpy as np
import pytest

from sspslam_amd import simulator as PLAN
from sspslam_amd.builder import build, dft_structure
from oracle import OracleSimulator

import dft_checks as D

pytestmark = pytest.mark.gpu

N_MODELS = 8
GROUPS = D.deal(D.SWEEP, N_MODELS)
# lengths that also get a second transform into one target (inc onto a non-zero destination) and a synapse (set into the filter):
# direct with in-register and generic passes, out-of-place Bluestein (37: M = 80, 74: even, M = 160), in-place (97, 106, 251)
EXTRAS = (8, 24, 37, 45, 74, 97, 106, 251)
FOURSTEP, BIG, NO_FFT, NO_ROUNDS = PLAN.SSN_PLAN_FOUR_STEP_FFT, PLAN.SSN_PLAN_BLUESTEIN_FFT, PLAN.SSN_PLAN_NO_FFT, PLAN.SSN_PLAN_NO_ROUNDS


@pytest.fixture(scope="module")
def Simulator():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from sspslam_amd.simulator import Simulator
    return Simulator


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


@functools.lru_cache(maxsize=None)
def built(lengths, kinds=(1, 2, 3, 4, 5), extras=EXTRAS):
    """One model per group of lengths and its oracle run, shared by every test that needs it -> (model, cases, steps, oracle outputs)."""
    net, cases, steps = D.transform_model(lengths, kinds, extras)
    model = build(net, staged=False)
    dfts = [o for o in model.ops if o["kind"] == "matvec" and o.get("dft")]
    assert len(dfts) == D.n_transforms([c for c in cases if c.d >= 8]) and all(o["stage"] == 1 for o in dfts)    # (d < 8: no DFT map by name)
    assert not any(o["kind"] in ("neurons", "ensarray") for o in model.ops)           # a neuron-free core
    ref = OracleSimulator(model)
    ref.run_steps(steps)
    want = [np.array(ref.probe_data(c.index)) for c in cases]
    for w in want:
        w.setflags(write=False)
    return model, cases, steps, want


def run_group(Simulator, capfd, lengths, label, flags=0, env=None, four_step=False, no_inplace=False, kinds=(1, 2, 3, 4, 5),
              fft=True, c_of=None):
    """Build under SSN_DEBUG_PLAN (the environment is set around ``Simulator(...)`` only), run every row in one ``run_steps``, assert
    the route and hold every element of every row to the bar -> the plans that ran."""
    model, cases, steps, want = built(tuple(lengths), tuple(kinds))
    out = capfd.readouterr()
    print(out.out, end="")
    with environment(SSN_DEBUG_PLAN="1", **(env or {})):
        sim = Simulator(None, model=model, dtype="f32", flags=flags)
    listing = D.parse_listing(capfd.readouterr().err)
    with sim:
        sim.run_steps(steps)
        got = [np.array(sim.data[c.p_out]) for c in cases]
        cnt = sim.counters()
    plans = [D.plan(c.d, k, four_step, no_inplace) for c in cases for k in c.kinds]
    if not fft:
        assert cnt["fft_transforms"] == 0 and cnt["fft_bluestein"] == 0, cnt
        c_of = c_of or (lambda d, k: D.C["direct"])
    else:
        assert all(p is not None for p in plans)
        assert sorted(listing) == sorted(p.key() for p in plans), (label, sorted(set(listing) ^ {p.key() for p in plans})[:6])
        assert cnt["fft_transforms"] == len(plans) and cnt["fft_bluestein"] == sum(1 for p in plans if p.M), (label, cnt)
        c_of = c_of or (lambda d, k: D.C[D.plan(d, k, four_step, no_inplace).cls])
    res = D.judge(cases, steps, lambda c: got[cases.index(c)], lambda c: want[cases.index(c)], c_of)
    by_cls = {}
    for case, r, c, row in res:
        cls = D.plan(case.d, case.kinds[0], four_step, no_inplace).cls if fft else "matrix"
        if r / c > by_cls.get(cls, (-1.0,))[0]:
            by_cls[cls] = (r / c, r, case, row)
    for cls, (frac, r, case, row) in sorted(by_cls.items()):
        print("%s: %-18s worst %.2f of the bar (error %.2f u A) at %r row %d" % (label, cls, frac, r, case, row))
    bad = [(repr(case), r, c, row) for case, r, c, row in res if not r <= c]
    assert not bad, (label, bad[:8])
    return [p for p in plans if p is not None]


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", range(N_MODELS))
def test_default_plan_every_length(Simulator, capfd, g):
    """Every d in 8..256 in eight models (lengths dealt round-robin, so every model and every round mixes direct, in-place and
    out-of-place plans): the transforms as bodies of the round grid."""
    run_group(Simulator, capfd, GROUPS[g], "default %d" % g)


@pytest.mark.parametrize("g", range(N_MODELS))
def test_own_launches_every_length(Simulator, capfd, g):
    """SSN_PLAN_NO_ROUNDS: the same lengths as k_dft launches of their own - launch_dft's thread sizing, batches of mixed lengths and
    engines."""
    run_group(Simulator, capfd, GROUPS[g], "no rounds %d" % g, flags=NO_ROUNDS)


@pytest.mark.parametrize("g", range(N_MODELS))
def test_four_step_every_length(Simulator, capfd, g):
    """SSN_PLAN_FOUR_STEP_FFT: the same lengths on the matrix cores, any N1 x N2, dense primes (N1 = 1), Bluestein for the rest."""
    run_group(Simulator, capfd, GROUPS[g], "four-step %d" % g, flags=FOURSTEP, four_step=True)


def test_coverage_of_the_sweep():
    """What the sweep claims to reach, from the restated planner (which the tests above hold to the planner's listing for every
    length): the fifteen radices, both Bluestein orders, an even Bluestein length, a dense-prime four-step and a four-step Bluestein."""
    D.assert_coverage()


def test_which_kernels_run(Simulator):
    """Default plan: the transforms are bodies of k_round.  SSN_PLAN_NO_ROUNDS: launches of k_dft.  The four-step engine never runs
    inside k_round (its accumulators would cost every body of every round a wave per SIMD): k_dft launches next to the rounds."""
    model, _, steps, _ = built(GROUPS[0])
    names = {}
    for flags in (0, NO_ROUNDS, FOURSTEP):
        with Simulator(None, model=model, dtype="f32", flags=flags) as sim:
            sim.run_steps(16, profile=2)
            names[flags] = set(sim.kernel_times())
    assert "k_round" in names[0] and "k_dft" not in names[0], sorted(names[0])
    assert "k_dft" in names[NO_ROUNDS] and "k_round" not in names[NO_ROUNDS], sorted(names[NO_ROUNDS])
    assert "k_dft" in names[FOURSTEP], sorted(names[FOURSTEP])


INPLACE = tuple(d for d in D.SWEEP if D.plan(d, 1).inplace)


@pytest.mark.parametrize("g", range(2))
def test_no_inplace_lengths(Simulator, capfd, g):
    """SSN_DFT_NO_INPLACE=1: the 60 in-place lengths out of place (M = 128, 256, 512 through dft_stockham)."""
    assert len(INPLACE) == 60
    plans = run_group(Simulator, capfd, D.deal(INPLACE, 2)[g], "no in-place %d" % g, env={"SSN_DFT_NO_INPLACE": "1"}, no_inplace=True)
    assert all(p.M and not p.inplace for p in plans)


def test_serial_chain_members(Simulator, capfd):
    """SSN_SOLO_DFT=1: every fifth length as a member of a serial chain (the radix list in the constant address space)."""
    out = capfd.readouterr()
    lengths = D.SWEEP[::5]
    model = built(lengths)[0]
    with environment(SSN_DEBUG_PLAN="1", SSN_SOLO_DFT="1"):
        with Simulator(None, model=model, dtype="f32"):
            pass
    err = capfd.readouterr().err
    assert "serial chain in round" in err and " dft" in err.split("serial chain in round", 1)[1], "no transform is a chain member"
    run_group(Simulator, capfd, lengths, "serial chains", env={"SSN_SOLO_DFT": "1"})


def test_dense_matrices_agree(Simulator, capfd):
    """SSN_PLAN_NO_FFT on one group: the matrix path (``fft_transforms == 0``) is held to the same bar as the direct transforms."""
    run_group(Simulator, capfd, GROUPS[3], "matrices", flags=NO_FFT, fft=False)


def test_short_lengths_fall_back(Simulator, capfd):
    """d = 4..7: ``dft_structure`` does not name them and ``plan_dft`` would not plan them: the matrix, still right."""
    run_group(Simulator, capfd, (4, 5, 6, 7), "short", fft=False)


@pytest.mark.parametrize("d,big,no_inplace,kinds", D.LONG, ids=["%d%s" % (e[0], "-oop" if e[2] else "") for e in D.LONG])
def test_long_lengths(Simulator, capfd, d, big, no_inplace, kinds):
    """512 (8,8,8), 961 (31,31), 1015, 1024 (8,8,4,4), 1089 (11,11,9), 2048, 2187 (9,9,9,3), 2197 (13^3), 3125 (5^5); 1801 (M = 4096 in
    place, and out of place: the only out-of-place transform of four radix-8 passes), 2049 (M = 4608) and 3199 (M = 6400, the LDS
    ceiling; kinds 1 and 5 only: its matrices are 164 MB each) under SSN_PLAN_BLUESTEIN_FFT.  Each length is held to twice its own
    stand-in figure (``dft_checks.C0_LONG``)."""
    c = 2.0 * D.C0_LONG[(d, no_inplace)]
    p = D.plan(d, 1, no_inplace=no_inplace)
    assert bool(p.M) == big and (not big or D.needs_flag(p)) and c < D.analytic_c(p)
    plans = run_group(Simulator, capfd, (d,), "long %d" % d, flags=BIG if big else 0, no_inplace=no_inplace, kinds=kinds,
                      env={"SSN_DFT_NO_INPLACE": "1"} if no_inplace else None, c_of=lambda d_, k: c)
    assert all(bool(q.inplace) == (d == 1801 and not no_inplace) for q in plans)


def test_long_bluestein_lengths_keep_the_matrix_by_default(Simulator, capfd):
    """Without SSN_PLAN_BLUESTEIN_FFT a convolution length M >= 2048 is not worth one workgroup: 1801, 2049 and 3199 keep the matrix
    (kind 1 only: the route is what is asserted)."""
    for d in (1801, 2049, 3199):
        model = built((d,), (1,))[0]
        with Simulator(None, model=model, dtype="f32") as sim:
            c = sim.counters()
        assert c["fft_transforms"] == 0 and c["fft_bluestein"] == 0, (d, c)


def test_near_and_scaled_matrices(Simulator):
    """Seams of the recognition: a matrix within 1e-12 of a DFT takes the FFT and is held to the exact matrix's bar plus its own
    distance; ``0.5 * transform_in`` is no DFT map and keeps the matrix.  (6399 and 6401 - no plan - are left out: their matrices are
    0.65 GB each.)"""
    import sspslam_amd.frontend as nengo
    d = 45
    H, X = d // 2 + 1, D.forward_rows(d)
    rng = np.random.RandomState(5)
    near = D.matrix(d, 1) + rng.uniform(-9e-13, 9e-13, (4 * H, d))
    half = 0.5 * D.matrix(d, 2)
    assert dft_structure(near) == 1 and dft_structure(half) == 0
    with nengo.Network(seed=1) as net:
        u = nengo.Node(D._table(X), size_out=d)
        t1, t2 = nengo.Node(size_in=4 * H), nengo.Node(size_in=4 * H)
        nengo.Connection(u, t1, transform=near, synapse=None)
        nengo.Connection(u, t2, transform=half, synapse=None)
        p1, p2 = nengo.Probe(t1), nengo.Probe(t2)
    model = build(net, staged=False)
    assert sorted(o.get("dft", 0) for o in model.ops if o["kind"] == "matvec") == [0, 1]
    ref = OracleSimulator(model)
    ref.run_steps(len(X))
    with Simulator(None, model=model, dtype="f32") as sim:
        sim.run_steps(len(X))
        got1, got2, c = np.array(sim.data[p1]), np.array(sim.data[p2]), sim.counters()
    assert c["fft_transforms"] == 1 and c["fft_bluestein"] == 0, c
    A = D.scale(d, 1, X)
    r1 = D.ratios(got1, ref.probe_data(0), A).max()        # (9e-13 ||x||_1 is 1.5e-5 u A: the matrix's distance does not show)
    r2 = D.ratios(got2, ref.probe_data(1), 0.5 * A).max()
    print("near matrix %.2f u A, scaled matrix %.2f u A" % (r1, r2))
    assert r1 <= D.C["direct"] + 1e-3 and r2 <= D.C["direct"]
