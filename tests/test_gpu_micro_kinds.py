"""Every glue micro-operator kind (``ssn::MicroKind``, csrc/ssn_micro.hpp) through every kernel that runs it.

The 17 kinds are computed by one definition each and walked by four kernels: ``k_program`` and ``k_vecops`` (the item plan,
``SSN_PLAN_NO_ROUNDS``), the glue / serial-chain bodies of ``k_round`` (the default plan and its switches) and the time-batched
stages (``kb_elementwise`` alone under ``SSN_PLAN_NO_STAGE_BATCH``, ``kb_elementwise_multi`` otherwise).  Each model below runs
40 timesteps in f64 and f32 under six plans.  In f64 every plan has to match the float64 oracle at 1e-9 (the bar of
test_gpu_fuzz.py), and - no plan reorders a sum - all plans have to give the same probe arrays bit for bit.  The one exception
is a model with a gate (``GATED``): the gate's dot product is summed over the 4 waves of a round block in one plan and over the
16 waves of the program's workgroup in the other, so those models are held to the oracle bar only.  In f32 every filtered probe
has to stay within the cosine bar that test_gpu_fuzz.py applies to the first 40 timesteps.

Which model supplies which kind (asserted from the planner's own listing under SSN_DEBUG_PLAN, so that an operator that was
quietly planned some other way fails the test):

* ``pathint``  (``small_pathint(ssp_dim=7, n=64)``: one recurrent array, the fused core)  the time-batched stages: fill, axpy
  inc / set, table, probe
* ``fuzz 8``   (``random_network(8)``: pre and post stages around the core)   in the timestep axpy inc / set, lowpass, small
  matvec inc / set, probe, step end, row in / out, lincomb; in the batched stages fill, axpy inc, table, probe
* ``fuzz 7``   (``random_network(7)``: everything in the core)   fill, axpy inc / set, lowpass, table, small matvec inc / set,
  probe, step end, lincomb
  (Most fuzz seeds hold a dense product, a transform or an ensemble array that the item plan and the round plan sum in
  different orders, so their probes differ in the last bits between the plans whatever the micro-operators do; of seeds 1 - 40
  the probes are equal between all six plans for 5, 7, 8, 9, 10, 11, 18, 24, 28 and 40.)
* ``sizes``    reduce set / inc, ensemble finish, small matvec inc, lincomb, row in / out.  Two LIF populations of 4200 and 6300 neurons: their spike-sparse decodes are reduced over 17 and 25 chunks of
  256 neurons (the 16-, 8- and 1-deep parts of the reduction); an array of two ensembles of 4400 neurons: 9 partial sums per
  decoded row in f64 (2200 vectors of two doubles in sweeps of 256; the eight-deep part and the tail of the finish); an encoder
  product of 257 rows and an incrementing reduction of 257 rows (one past ``GLUE_ROWS``); 1-element operators
* ``cleanup``  a clean-up memory over a 50 x 50 grid of SSPs (2500 candidates: more than one trip of either argmax holds in
  flight) in a loop with a 1025-element filter (one past ``GLUE_CHUNK``); argmax + gather, lowpass
* ``gate``     the loop-closure gate on 257-element vectors, open and closed within the window; gate
"""
import contextlib
import os
import re

import numpy as np
import pytest

import sspslam_amd.frontend as nengo
from sspslam_amd import harness as H
from sspslam_amd import simulator as PLAN
from sspslam_amd.builder import build
from sspslam_amd.networks.slam import make_cleanup, make_gate
from oracle import OracleSimulator

from helpers import random_network, small_pathint

pytestmark = pytest.mark.gpu

STEPS = 40
PLANS = (("default", 0), ("no pipeline", PLAN.SSN_PLAN_NO_PIPELINE), ("no chains", PLAN.SSN_PLAN_NO_CHAINS),
         ("no rounds", PLAN.SSN_PLAN_NO_ROUNDS), ("no rounds, no item batch", PLAN.SSN_PLAN_NO_ROUNDS | PLAN.SSN_PLAN_NO_ITEM_BATCH),
         ("no stage batch", PLAN.SSN_PLAN_NO_STAGE_BATCH))
# positions in ``enum MicroKind`` (csrc/ssn_launch.hpp), as the plan listing prints them
(M_FILL, M_AXPY_INC, M_AXPY_SET, M_LOWPASS, M_TABLE, M_MATVEC_INC, M_MATVEC_SET, M_ENS_FINISH, M_GATE, M_ARGMAX_GATHER, M_PROBE,
 M_STEP_END, M_ROW_IN, M_ROW_OUT, M_REDUCE_SET, M_REDUCE_INC, M_LINCOMB) = range(1, 18)
GATED = ("gate",)


def sizes_network():
    with nengo.Network(seed=11) as net:
        u = nengo.Node(lambda t: [np.sin(7.0 * t), np.cos(5.0 * t)])
        one = nengo.Node(lambda t: 0.5 * np.sin(9.0 * t + 1.0))
        a = nengo.Ensemble(4200, 2)                      # ceil(4200 / 256) = 17 spike-list chunks
        b = nengo.Ensemble(6300, 3)                      # 25
        c = nengo.Ensemble(257, 1)                       # encoder product of 257 rows
        arr = nengo.EnsembleArray(4400, 2)               # f64: 2200 two-double vectors -> 9 workgroups per ensemble
        wide = nengo.Node(size_in=1025)
        dot = nengo.Node(size_in=1)
        nengo.Connection(u, a, synapse=None)
        nengo.Connection(a, a, synapse=0.05, transform=0.5)
        nengo.Connection(a, b, synapse=0.01, transform=np.array([[0.6, -0.3], [0.2, 0.5], [-0.4, 0.1]]))
        # (unfiltered spikes onto currents: the sparse product adds to what the encoder product left - a reduction that increments, 257 rows)
        nengo.Connection(a.neurons, c.neurons, synapse=None, transform=np.random.RandomState(4).uniform(-2e-3, 2e-3, size=(257, 4200)))
        nengo.Connection(b, b, synapse=0.05, transform=0.4)
        nengo.Connection(one, c, synapse=None)
        nengo.Connection(c, c, synapse=0.02, transform=0.3)
        nengo.Connection(b[:2], arr.input, synapse=0.01)
        nengo.Connection(arr.output, arr.input, synapse=0.05, transform=0.3)
        nengo.Connection(a, wide, synapse=0.01, transform=np.random.RandomState(3).uniform(-1, 1, size=(1025, 2)))
        nengo.Connection(c, dot, synapse=0.01)
        probes = [nengo.Probe(a, synapse=0.01), nengo.Probe(b, synapse=0.01), nengo.Probe(c, synapse=0.01),
                  nengo.Probe(arr.output, synapse=0.01), nengo.Probe(wide, synapse=0.01), nengo.Probe(dot)]
    return net, probes


def cleanup_network():
    space = H.make_ssp_space(2, ssp_dim=55)
    S, _ = space.get_sample_pts_and_ssps(50, "grid")           # 2500 candidates
    d = S.shape[1]
    rs = np.random.RandomState(5)
    with nengo.Network(seed=12) as net:
        u = nengo.Node(lambda t: space.encode(np.array([[0.7 * np.sin(40.0 * t), 0.6 * np.cos(25.0 * t)]]))[0])
        mem = nengo.Node(lambda t, x, f=make_cleanup(S): f(x), size_in=d, size_out=d)
        mem.native = ("cleanup", S, space.grid_factors(50))
        wide = nengo.Node(size_in=1025)                         # (in the loop through the clean-up: a filter of the core)
        nengo.Connection(u, mem, synapse=0.005)
        nengo.Connection(mem, wide, synapse=0.01, transform=rs.uniform(-1, 1, size=(1025, d)) / np.sqrt(d))
        nengo.Connection(wide, mem, synapse=0.02, transform=0.1 * rs.uniform(-1, 1, size=(d, 1025)) / np.sqrt(1025))
        probes = [nengo.Probe(mem), nengo.Probe(mem, synapse=0.01), nengo.Probe(wide, synapse=0.01)]
    return net, probes


def gate_network():
    d = 257
    rs = np.random.RandomState(6)
    est = rs.randn(d) / np.sqrt(d)
    w, ph = rs.uniform(2.0, 12.0, size=d), rs.uniform(0, 6.28, size=d)
    with nengo.Network(seed=13) as net:
        # <est, cur> crosses the threshold inside the window; the flag leaves zero for its last quarter
        a = nengo.Node(lambda t: est)
        b = nengo.Node(lambda t: est * (40.0 * t) + 0.02 * np.sin(w * t + ph))
        flag = nengo.Node(lambda t: 0.0 if t < 0.0305 else 1.0)
        gate = nengo.Node(make_gate(d, 0.4, 0.1), size_in=2 * d + 1, size_out=d)
        gate.native = ("gate", d, 0.4, 0.1)
        out = nengo.Node(size_in=d)
        nengo.Connection(a, gate[:d], synapse=None)
        nengo.Connection(b, gate[d:2 * d], synapse=None)
        nengo.Connection(out, gate[d:2 * d], synapse=0.01, transform=0.5)
        nengo.Connection(flag, gate[2 * d], synapse=None)
        nengo.Connection(gate, out, synapse=0.005)
        probes = [nengo.Probe(gate), nengo.Probe(out, synapse=0.01)]
    return net, probes


def pathint_network():
    pm = small_pathint(ssp_dim=7, n=64)
    return pm.model, [pm.probe]


MODELS = {
    "pathint": (pathint_network, {}),
    "fuzz 8": (lambda: random_network(8), {}),
    "fuzz 7": (lambda: random_network(7), {}),
    "sizes": (sizes_network, dict(n_eval_points=600)),
    "cleanup": (cleanup_network, {}),
    "gate": (gate_network, {}),
}
# kinds every listed plan of the model has to show, as (kind, length or None); batched: in a time-batched stage of every plan
REQUIRED = {
    "pathint": dict(batched=[(M_FILL, None), (M_AXPY_INC, None), (M_AXPY_SET, None), (M_TABLE, None), (M_PROBE, None)], step=[]),
    "fuzz 8": dict(batched=[(M_FILL, None), (M_AXPY_INC, None), (M_TABLE, None), (M_PROBE, None)],
                   step=[(k, None) for k in (M_AXPY_INC, M_AXPY_SET, M_LOWPASS, M_MATVEC_INC, M_MATVEC_SET, M_PROBE, M_STEP_END, M_ROW_IN,
                                             M_ROW_OUT, M_LINCOMB)]),
    "fuzz 7": dict(batched=[], step=[(k, None) for k in (M_FILL, M_AXPY_INC, M_AXPY_SET, M_LOWPASS, M_TABLE, M_MATVEC_INC, M_MATVEC_SET,
                                                         M_PROBE, M_STEP_END, M_LINCOMB)]),
    "sizes": dict(batched=[], step=[(M_REDUCE_SET, None), (M_REDUCE_INC, 257), (M_ENS_FINISH, None), (M_MATVEC_INC, 257),
                                    (M_MATVEC_INC, 4200), (M_LOWPASS, 1), (M_LINCOMB, None), (M_ROW_IN, None), (M_ROW_OUT, None)]),
    "cleanup": dict(batched=[], step=[(M_ARGMAX_GATHER, 55), (M_LOWPASS, 1025), (M_TABLE, 55), (M_LINCOMB, None)]),
    "gate": dict(batched=[(M_FILL, None), (M_TABLE, None)], step=[(M_GATE, 257), (M_ROW_IN, None), (M_ROW_OUT, None)]),
}


@contextlib.contextmanager
def environment(**env):
    for k in env:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k in env:
            os.environ.pop(k, None)


def listed_kinds(err):
    """An SSN_DEBUG_PLAN listing -> ({(kind, len)} of the timestep's micro-operators, {(kind, len)} of the batched stages,
    {reduction chunks})."""
    step, batched = set(), set()
    for line in err.splitlines():
        m = re.match(r"\[ssn\]\s+micro (\d+)/(\d+) ", line)
        if m:
            step.add((int(m.group(1)), int(m.group(2))))
        if re.match(r"\[ssn\] plan item +\d+ program:", line):
            step.update((int(k), int(n)) for k, n in re.findall(r" (\d+)/(\d+)", line.split("elements:", 1)[1]))
        m = re.match(r"\[ssn\]\s+batch op kind (\d+) dst -?\d+ src -?\d+ len (\d+)", line)
        if m:
            batched.add((int(m.group(1)), int(m.group(2))))
    return step, batched


def has(found, kind, length):
    return any(k == kind and (length is None or n == length) for k, n in found)


@pytest.fixture(scope="module")
def Simulator():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from sspslam_amd.simulator import Simulator
    return Simulator


@pytest.fixture(scope="module")
def seen():
    """(kind, role) pairs that some model's listing showed, collected over the parametrised cases for the closing test."""
    return {"step": set(), "batched": set()}


def cosine_errors(got, want):
    big = np.linalg.norm(want, axis=1) > 0.05
    if big.sum() < 10:
        return None
    return 1.0 - np.sum(want[big] * got[big], axis=1) / (np.linalg.norm(want[big], axis=1) * np.linalg.norm(got[big], axis=1))


@pytest.mark.parametrize("name", list(MODELS))
def test_every_plan_computes_the_same_timestep(Simulator, capfd, seen, name):
    make, build_kw = MODELS[name]
    net, probes = make()
    model = build(net, **build_kw)
    ref = OracleSimulator(model)
    ref.run_steps(STEPS)
    index = {id(p): [i for i, mp in enumerate(model.probes) if mp["probe"] is p][0] for p in probes}
    want = {id(p): ref.probe_data(index[id(p)]) for p in probes}
    first, report = None, []
    try:
        for plan, flags in PLANS:
            worst = {"f64": 0.0, "f32": 0.0}
            for dtype in ("f64", "f32"):
                capfd.readouterr()
                with environment(SSN_DEBUG_PLAN="1"):
                    sim = Simulator(None, model=model, dtype=dtype, flags=flags)
                step, batched = listed_kinds(capfd.readouterr().err)
                with sim:
                    sim.run_steps(STEPS)
                    got = {id(p): np.array(sim.data[p]) for p in probes}
                if dtype == "f64":
                    report.append(f"{name}, {plan}: kinds of the timestep {sorted({k for k, _ in step})}, of the batched stages "
                                  f"{sorted({k for k, _ in batched})}")
                    seen["step"] |= {k for k, _ in step}
                    seen["batched"] |= {k for k, _ in batched}
                for kind, length in REQUIRED[name]["step"]:
                    assert has(step, kind, length), f"{name}, {plan}, {dtype}: no micro-operator {kind}/{length} in {sorted(step)}"
                for kind, length in REQUIRED[name]["batched"]:
                    assert has(batched, kind, length), f"{name}, {plan}, {dtype}: no batched operator {kind}/{length} in {sorted(batched)}"
                for p in probes:
                    g, w = got[id(p)], want[id(p)]
                    assert g.shape == w.shape and np.all(np.isfinite(g)), (name, plan, dtype, index[id(p)])
                    ce = cosine_errors(g, w) if dtype == "f32" and p.synapse is not None else None
                    if dtype == "f64":
                        worst[dtype] = max(worst[dtype], float(np.max(np.abs(g - w))))
                    elif ce is not None:
                        worst[dtype] = max(worst[dtype], float(ce.max()))
                report.append(f"{name}, {plan}, {dtype}: " + ("largest difference to the oracle %.2e (bar 1e-9)" if dtype == "f64" else
                                                              "largest cosine error of a filtered probe %.2e (bar 1e-3)") % worst[dtype])
                for p in probes:
                    if dtype == "f64":
                        np.testing.assert_allclose(got[id(p)], want[id(p)], atol=1e-9, rtol=0, err_msg=f"{name}, {plan}, probe {index[id(p)]}")
                assert dtype == "f64" or worst[dtype] < 1e-3, (name, plan, worst[dtype])
                if dtype == "f64":
                    if first is None:
                        first = (plan, got)
                    elif name not in GATED:
                        for p in probes:
                            assert np.array_equal(got[id(p)], first[1][id(p)]), \
                                f"{name}: probe {index[id(p)]} differs between the plans '{first[0]}' and '{plan}'"
    finally:
        with capfd.disabled():
            print("\n" + "\n".join(report))


def test_the_models_cover_all_seventeen_kinds(seen):
    """(runs after the cases above: the kinds their f64 listings showed, over all models and plans)"""
    assert seen["step"] | seen["batched"] == set(range(1, 18)), sorted(set(range(1, 18)) - seen["step"] - seen["batched"])
    assert seen["batched"] >= {M_FILL, M_AXPY_INC, M_AXPY_SET, M_TABLE, M_PROBE}, sorted(seen["batched"])
