"""Direct neuron input of EnsembleArray members on the device: the drive columns of ``k_ensarray_drv``.

f64 runs are compared with ``oracle.graphwalk`` (J = bias + scaled_encoders . x + direct neuron input), spike for spike where
the arithmetic is the same on both sides: a drive scalar is 0 or 1 wherever it decides a spike, so ``w * s`` is exact, and
where several columns are on together the first one's weight of at most -10 silences the member whatever the rounding
(``bias + |encoders|`` stays below 4.9: the current of a 150 Hz LIF neuron).  f32 runs are compared with the f64 run under the
project's 1e-3 cosine bar.  Every case asserts through ``counters()`` that no whole-block kernel ran.

What the exact cases do not check: since rounding never decides a spike in them, the documented order of the sum (bias, encoder
product, then the columns in connection order) is checked at rounding level only by the filtered oscillator of case 2 and by the
decoded sources of case 2b, whose scalars are arbitrary reals.  ``counters()`` does not say which kernel stepped a driven array
beyond "not the block kernel": the fused-core plan with block-row sources is reached by ``gated_array`` under flags 0 only (its
array is the whole core and its gate a pre-stage signal), and that it was reached is not asserted."""
import ctypes as C

import numpy as np
import pytest

import sspslam_amd.frontend as nengo
from sspslam_amd import harness as H
from sspslam_amd import simulator as PLAN
from sspslam_amd import _lib
from sspslam_amd.builder import build
from sspslam_amd.networks import AdditiveInputGatedMemory
from oracle.graphwalk import GraphWalkSimulator

from helpers import small_pathint
from test_neuron_input import gated_memory, check_memory_behaviour

pytestmark = pytest.mark.gpu

DT = 0.001
STEPS = 300
NO_ITEM_PLAN = PLAN.SSN_PLAN_NO_FUSED_CORE | PLAN.SSN_PLAN_NO_ROUNDS
RATES = dict(max_rates=nengo.Uniform(80, 150), intercepts=nengo.Uniform(-0.5, 0.5))      # bias + |encoders| <= 4.85 < 10


@pytest.fixture(scope="module")
def Simulator():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from sspslam_amd.simulator import Simulator
    return Simulator


def window(lo, hi):
    """1 during timesteps lo + 1 .. hi, else 0 (t-only)."""
    return lambda t: 1.0 if lo < int(round(t / DT)) <= hi else 0.0


def no_block_kernel(c):
    assert c["block_tpb"] == 0 and c["launches_per_step"] >= 1, c


# ---- 1. an array inhibited through add_neuron_input(), both fast modes --------------------------------------------------------
_GATED = {}


def gated_array(form):
    """K = 5, n = 60; ``dense``: din = dout = 1; ``sparse``: 3-dimensional members with a 5-wide function output."""
    if form not in _GATED:
        K, n = 5, 60
        din = 1 if form == "dense" else 3
        with nengo.Network(seed=3) as net:
            stim = nengo.Node(lambda t: [0.8 * np.sin(7 * t + 0.4 * i) for i in range(K * din)])
            gate = nengo.Node(window(100, 200))
            ea = nengo.EnsembleArray(n, K, ens_dimensions=din, seed=5, **RATES)
            nengo.Connection(stim, ea.input, synapse=0.005)
            out = ea.output if form == "dense" else ea.add_output("f", lambda x: [x[0], x[1], x[2], x[0] * x[1], x[2] ** 2])
            nengo.Connection(gate, ea.add_neuron_input(), transform=np.ones((K * n, 1)) * -10, synapse=None)
            probes = {"out": nengo.Probe(out, synapse=0.01), "tap0": nengo.Probe(ea.ea_ensembles[0].neurons),
                      "tap3": nengo.Probe(ea.ea_ensembles[3].neurons[7:50])}
        model = build(net)
        eo = [o for o in model.ops if o["kind"] == "ensarray"][0]
        assert (eo["din"], eo["dout"], eo["drive"]["m"]) == ((1, 1, 1) if form == "dense" else (3, 5, 1))
        for k, e in enumerate(ea.ea_ensembles):
            be = model.params[e]
            assert (be.bias + np.abs(be.scaled_encoders).sum(axis=1)).max() < 10.0
        walk = GraphWalkSimulator(net, model)
        walk.run_steps(STEPS)
        want = {k: np.array(walk.probe_data(p)) for k, p in probes.items()}
        assert (want["tap0"][:100] != 0).sum() > 50 and (want["tap0"][200:] != 0).sum() > 50
        _GATED[form] = (model, probes, want)
    return _GATED[form]


@pytest.mark.parametrize("flags", [0, PLAN.SSN_PLAN_SEPARATE_FINISH, PLAN.SSN_PLAN_NO_FUSED_CORE, NO_ITEM_PLAN])
@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_f64_gated_array_equals_the_graph_walk(Simulator, form, flags):
    model, probes, want = gated_array(form)
    with Simulator(None, model=model, dtype="f64", block_steps=96, flags=flags) as sim:
        runs = []
        for _ in range(2):
            sim.run_steps(STEPS)
            no_block_kernel(sim.counters())
            runs.append({k: np.array(sim.data[p]) for k, p in probes.items()})
            sim.reset()
    got = runs[0]
    err = float(np.max(H.cosine_error(got["out"][20:], want["out"][20:])))
    print("%s flags %d: decoded cosine error %.3e, max abs %.3e; tap mismatches %d / %d" % (
        form, flags, err, np.abs(got["out"] - want["out"]).max(), int((got["tap0"] != want["tap0"]).sum()),
        int((got["tap3"] != want["tap3"]).sum())))
    assert err < 1e-9
    for k in ("tap0", "tap3"):
        np.testing.assert_array_equal(got[k], want[k])
        assert not got[k][100:200].any()                   # samples of timesteps 101 .. 200: the gated window
        assert got[k][:100].any() and got[k][200:].any()
    for k in got:
        np.testing.assert_array_equal(runs[1][k], got[k])


# ---- 1b. the drive on the second of two arrays --------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, NO_ITEM_PLAN])
def test_f64_drive_on_the_second_of_two_arrays(Simulator, flags):
    """Two arrays of K = 2 members of 64 neurons, both tapped, the drive on the second one only (drive columns belong to an
    operator by its index in the model, and the first array has none to be mistaken for); 20 steps, spike for spike.  Default
    rates of up to 400 Hz: -10 thins the driven members' spikes out during timesteps 9 .. 14, it does not silence them."""
    steps = 20
    with nengo.Network(seed=14) as net:
        stim = nengo.Node(lambda t: [0.8 * np.sin(40 * t), 0.6 * np.cos(30 * t)])
        gate = nengo.Node(window(8, 14))
        first = nengo.EnsembleArray(64, 2, seed=15)
        second = nengo.EnsembleArray(64, 2, seed=16)
        nengo.Connection(stim, first.input, synapse=0.005)
        nengo.Connection(stim, second.input, synapse=0.005)
        nengo.Connection(gate, second.add_neuron_input(), transform=np.ones((2 * 64, 1)) * -10, synapse=None)
        probes = {"free": nengo.Probe(first.ea_ensembles[1].neurons), "driven": nengo.Probe(second.ea_ensembles[1].neurons)}
        p_out = nengo.Probe(second.output, synapse=0.01)
    model = build(net)
    assert ["drive" in o for o in model.ops if o["kind"] == "ensarray"] == [False, True]
    walk = GraphWalkSimulator(net, model)
    walk.run_steps(steps)
    want = {k: np.array(walk.probe_data(p)) for k, p in probes.items()}
    spikes = want["driven"] != 0
    assert spikes[:8].sum() > 20 and spikes[14:].sum() > 20 and 0 < spikes[8:14].sum() < 0.5 * spikes[:8].sum()
    assert (want["free"][8:14] != 0).sum() > 20
    with Simulator(None, model=model, dtype="f64", flags=flags) as sim:
        sim.run_steps(steps)
        no_block_kernel(sim.counters())
        for k, p in probes.items():
            got = np.array(sim.data[p])
            print("flags %d %s: %d spikes, %d mismatches" % (flags, k, int((want[k] != 0).sum()), int((got != want[k]).sum())))
            np.testing.assert_array_equal(got, want[k])
        np.testing.assert_allclose(np.array(sim.data[p_out]), walk.probe_data(p_out), atol=1e-9, rtol=0)


# ---- 2. the path integrator with two driven oscillators, every plan -----------------------------------------------------------
_DRIVEN_PI = {}


def driven_pathint():
    if not _DRIVEN_PI:
        n = 64
        pm = small_pathint(ssp_dim=7, n=n, T=10.0, limit=0.2)
        ens = pm.pathintegrator.oscillators.ea_ensembles
        with pm.model:
            gate = nengo.Node(window(100, 200), label="gate")
            nengo.Connection(gate, ens[1].neurons, transform=np.ones((n, 1)) * -10, synapse=0.005, seed=21)
            nengo.Connection(gate, ens[2].neurons[8:40], transform=np.ones((32, 1)) * -10, synapse=None, seed=22)
            probes = {"filtered": nengo.Probe(ens[1].neurons), "slice": nengo.Probe(ens[2].neurons), "decoded": pm.probe}
        model = build(pm.model)
        walk = GraphWalkSimulator(pm.model, model)
        walk.run_steps(STEPS)
        want = {k: np.array(walk.probe_data(p)) for k, p in probes.items()}
        # (the oscillators' default rates of up to 400 Hz put bias + |encoders| above 10: -10 thins the driven neurons' spikes out,
        #  it does not silence all of them)
        before, during = want["slice"][:100] != 0, want["slice"][100:200] != 0
        print("graph walk, member 2: spikes of [8:40] %d -> %d under the drive, of the other neurons %d -> %d" % (
            before[:, 8:40].sum(), during[:, 8:40].sum(), before.sum() - before[:, 8:40].sum(), during.sum() - during[:, 8:40].sum()))
        assert during[:, 8:40].sum() < 0.5 * before[:, 8:40].sum() and during[:, :8].any() and (want["filtered"] != 0).sum() > 100
        _DRIVEN_PI.update(model=model, probes=probes, want=want)
    return _DRIVEN_PI["model"], _DRIVEN_PI["probes"], _DRIVEN_PI["want"]


PI_PLANS = [("default", 0), ("per-timestep", PLAN.SSN_PLAN_NO_BLOCK_KERNEL), ("rounds", PLAN.SSN_PLAN_NO_FUSED_CORE),
            ("no-rounds", PLAN.SSN_PLAN_NO_ROUNDS), ("items", NO_ITEM_PLAN), ("own-launch", PLAN.SSN_PLAN_ENS_OWN_LAUNCH)]


@pytest.mark.parametrize("plan,flags", PI_PLANS)
def test_f64_driven_oscillators_on_every_plan(Simulator, plan, flags):
    """Member 1 through a 5 ms synapse, member 2 ``[8:40]`` directly.  The filter runs on the 1-wide source here and on the
    weighted 64-wide output in the graph walk (-10 * lowpass(s) against lowpass(-10 * s)): the two differ by rounding, which can
    move a spike of member 1 across a step boundary.  Differing raster samples of member 1, of 19 200: expected 0, measured 0 on
    every plan (MI355X); allowed at most 0.1 % = 19."""
    model, probes, want = driven_pathint()
    with Simulator(None, model=model, dtype="f64", block_steps=96, flags=flags) as sim:
        sim.run_steps(STEPS)
        no_block_kernel(sim.counters())
        got = {k: np.array(sim.data[p]) for k, p in probes.items()}
    err = float(np.max(H.cosine_error(got["decoded"][20:], want["decoded"][20:])))
    differing = int((got["filtered"] != want["filtered"]).sum())
    print("%s: decoded cosine error %.3e; filtered member: %d of %d raster samples differ; slice member: %d" % (
        plan, err, differing, want["filtered"].size, int((got["slice"] != want["slice"]).sum())))
    np.testing.assert_array_equal(got["slice"], want["slice"])
    assert err < 1e-9
    assert differing <= 0.001 * want["filtered"].size


# ---- 2b. drives decoded from ensembles ----------------------------------------------------------------------------------------
_DECODED = {}


def decoded_drives():
    """K = 3, n = 60: member 0 driven without a synapse by the decoded value of a plain ensemble (stepped before the array within
    the timestep), member 2 through a 5 ms synapse by the decoded value of member 1 of the same array."""
    if not _DECODED:
        K, n = 3, 60
        with nengo.Network(seed=12) as net:
            stim = nengo.Node(lambda t: [0.8 * np.sin(7 * t + 0.4 * i) for i in range(K)])
            gate = nengo.Node(window(100, 200))
            ctl = nengo.Ensemble(80, 1, seed=13, **RATES)
            ea = nengo.EnsembleArray(n, K, seed=5, **RATES)
            nengo.Connection(gate, ctl, synapse=None)
            nengo.Connection(stim, ea.input, synapse=0.005)
            nengo.Connection(ctl, ea.ea_ensembles[0].neurons, transform=np.ones((n, 1)) * -3, synapse=None, seed=41)
            nengo.Connection(ea.ea_ensembles[1], ea.ea_ensembles[2].neurons, transform=np.ones((n, 1)) * -1.5, synapse=0.005, seed=42)
            probes = {"out": nengo.Probe(ea.output, synapse=0.01), "m0": nengo.Probe(ea.ea_ensembles[0].neurons),
                      "m2": nengo.Probe(ea.ea_ensembles[2].neurons)}
        model = build(net)
        walk = GraphWalkSimulator(net, model)
        walk.run_steps(STEPS)
        want = {k: np.array(walk.probe_data(p)) for k, p in probes.items()}
        on, off = (want["m0"][120:200] != 0).sum(), (want["m0"][220:300] != 0).sum()
        print("graph walk: member 0 spikes %d under the decoded drive, %d after it; member 2: %d" % (on, off, (want["m2"] != 0).sum()))
        assert on < 0.5 * off and (want["m2"] != 0).sum() > 100
        _DECODED.update(model=model, probes=probes, want=want)
    return _DECODED["model"], _DECODED["probes"], _DECODED["want"]


@pytest.mark.parametrize("plan,flags", [("default", 0), ("rounds", PLAN.SSN_PLAN_NO_FUSED_CORE), ("items", NO_ITEM_PLAN)])
def test_f64_drives_decoded_from_ensembles(Simulator, plan, flags):
    """The drive scalars are decoded sums here, which the device and the graph walk add up in different orders: they agree to
    rounding, not bit for bit, and w * (D . a) in the column against (w * D) . a in the graph walk rounds differently too.  As
    for the filtered oscillator, such a difference can move a spike across a step boundary: differing raster samples of the two
    driven members, of 18 000 each: expected 0, measured 0 on the three plans (MI355X), allowed at most 0.1 % = 18; the decoded output under the 1e-9 bar."""
    model, probes, want = decoded_drives()
    with Simulator(None, model=model, dtype="f64", block_steps=96, flags=flags) as sim:
        sim.run_steps(STEPS)
        no_block_kernel(sim.counters())
        got = {k: np.array(sim.data[p]) for k, p in probes.items()}
    err = float(np.max(H.cosine_error(got["out"][20:], want["out"][20:])))
    differing = {k: int((got[k] != want[k]).sum()) for k in ("m0", "m2")}
    print("%s: decoded cosine error %.3e; raster samples that differ: member 0 %d, member 2 %d of %d" % (
        plan, err, differing["m0"], differing["m2"], want["m0"].size))
    assert err < 1e-9
    assert differing["m0"] <= 0.001 * want["m0"].size and differing["m2"] <= 0.001 * want["m2"].size


# ---- 3. shapes ----------------------------------------------------------------------------------------------------------------
_SHAPES = {}


def shaped_array(n, din, m, neuron):
    """K = 3; members 0 and 2 get ``m`` columns each from per-member connections, member 1 none (all its slots are -1).  Column 0
    has weights in [-12, -10], the others in [-3, 0]; every column is on alone for 20 timesteps (one exact product decides the
    spikes), then all together for 60 (column 0 silences the member)."""
    key = (n, din, m, neuron)
    if key not in _SHAPES:
        K = 3
        rng = np.random.RandomState(n + 10 * din + m)
        nt = nengo.LIF() if neuron == "lif" else nengo.LIFRate(amplitude=0.5)

        def gates(t):
            s = int(round(t / DT))
            return [1.0 if (40 + 30 * j < s <= 60 + 30 * j) or (200 < s <= 260) else 0.0 for j in range(m)]
        with nengo.Network(seed=6) as net:
            stim = nengo.Node(lambda t: [0.7 * np.sin(9 * t + 0.5 * i) for i in range(K * din)])
            gate = nengo.Node(gates)
            ea = nengo.EnsembleArray(n, K, ens_dimensions=din, seed=8, neuron_type=nt, **RATES)
            nengo.Connection(stim, ea.input, synapse=0.005)
            for i in (0, 2):
                W = np.concatenate([rng.uniform(-12, -10, size=(n, 1)), rng.uniform(-3, 0, size=(n, m - 1))], axis=1)
                nengo.Connection(gate, ea.ea_ensembles[i].neurons, transform=W, synapse=None, seed=30 + i)
            probes = {"out": nengo.Probe(ea.output, synapse=0.01), "driven": nengo.Probe(ea.ea_ensembles[2].neurons),
                      "free": nengo.Probe(ea.ea_ensembles[1].neurons[1:n - 1])}
        model = build(net)
        eo = [o for o in model.ops if o["kind"] == "ensarray"][0]
        src = model.buffers[eo["drive"]["src"]]
        assert eo["drive"]["m"] == m and (src[1] == -1).all() and (src[0] >= 0).all() and (src[2] >= 0).all()
        walk = GraphWalkSimulator(net, model)
        walk.run_steps(STEPS)
        want = {k: np.array(walk.probe_data(p)) for k, p in probes.items()}
        assert not want["driven"][200:260].any() and want["driven"][:40].any() and want["free"][200:260].any()
        _SHAPES[key] = (model, probes, want)
    return _SHAPES[key]


SHAPES = [(60, 1, 1, "lif"), (60, 4, 2, "lif"), (60, 4, 4, "lif"), (1030, 1, 4, "lif"), (1030, 4, 1, "lif"), (1030, 1, 2, "lif"),
          (60, 4, 4, "lifrate"), (1030, 1, 2, "lifrate")]


@pytest.mark.parametrize("n,din,m,neuron,sweeps", [s + (None,) for s in SHAPES] + [s + (8,) for s in SHAPES if s[0] == 1030])
def test_shapes_f64_exact_and_f32_under_the_bar(Simulator, monkeypatch, n, din, m, neuron, sweeps):
    """LIF members: rasters equal to the graph walk's.  LIFRate members: rates to ``rtol = 1e-9``, as in
    ``test_gpu_neuron_taps.py::test_f64_lifrate_members`` - the device's ``log1p`` is not NumPy's to the last bit, so a rate is not
    a bit-for-bit quantity on either side; a rate that is 0 on one side (current at or below threshold) is 0 on the other.
    ``sweeps`` = 8: one workgroup steps a whole ensemble of 1030 neurons in two (f32) or three (f64) 256-thread sweeps - the
    prefetch of the next sweep's weights; default: one sweep per workgroup, two or three workgroups per ensemble."""
    model, probes, want = shaped_array(n, din, m, neuron)
    monkeypatch.delenv("SSN_ENS_SWEEPS", raising=False)
    if sweeps is not None:
        monkeypatch.setenv("SSN_ENS_SWEEPS", str(sweeps))
    got = {}
    for dtype in ("f64", "f32"):
        with Simulator(None, model=model, dtype=dtype, block_steps=96) as sim:
            sim.run_steps(STEPS)
            no_block_kernel(sim.counters())
            got[dtype] = {k: np.array(sim.data[p], dtype=np.float64) for k, p in probes.items()}
    g = got["f64"]
    if neuron == "lif":
        print("n=%d din=%d m=%d: raster mismatches driven %d free %d" % (n, din, m, int((g["driven"] != want["driven"]).sum()),
                                                                          int((g["free"] != want["free"]).sum())))
        np.testing.assert_array_equal(g["driven"], want["driven"])
        np.testing.assert_array_equal(g["free"], want["free"])
    else:
        np.testing.assert_allclose(g["driven"], want["driven"], rtol=1e-9, atol=0)
        np.testing.assert_allclose(g["free"], want["free"], rtol=1e-9, atol=0)
    assert not g["driven"][200:260].any() and not got["f32"]["driven"][200:260].any()
    assert float(np.max(H.cosine_error(g["out"][20:], want["out"][20:]))) < 1e-9
    err32 = float(np.max(H.cosine_error(got["f32"]["out"][20:], g["out"][20:])))
    print("n=%d din=%d m=%d %s: f32 against f64 cosine error %.3e" % (n, din, m, neuron, err32))
    assert err32 < 1e-3


# ---- 4. AdditiveInputGatedMemory ----------------------------------------------------------------------------------------------
def test_f64_additive_input_gated_memory(Simulator):
    net = gated_memory(AdditiveInputGatedMemory, nengo.EnsembleArray, d=4, n=50)
    model = build(net)
    walk = GraphWalkSimulator(net, model)
    walk.run_steps(900)
    want = walk.probe_data(net.p)
    with Simulator(None, model=model, dtype="f64", block_steps=96) as sim:
        sim.run_steps(900)
        no_block_kernel(sim.counters())
        got = np.array(sim.data[net.p])
    err = float(np.max(H.cosine_error(got[20:600], want[20:600])))
    print("working memory: cosine error %.3e over the loaded and held phases, max abs %.3e over the run" % (err, np.abs(got - want).max()))
    assert err < 1e-9
    np.testing.assert_allclose(got, want, atol=1e-9, rtol=0)           # (after the reset the value is 0: no direction to compare)
    check_memory_behaviour(got)


# ---- 5. a drive that adds nothing; taps beside drives -------------------------------------------------------------------------
def zero_drive_net(variant):
    n, K = 60, 4
    with nengo.Network(seed=9) as net:
        stim = nengo.Node(lambda t: [0.8 * np.sin(7 * t + 0.4 * i) for i in range(K * 3)])
        zero = nengo.Node(lambda t: [0.0, 0.0])
        ea = nengo.EnsembleArray(n, K, ens_dimensions=3, seed=5, **RATES)
        nengo.Connection(stim, ea.input, synapse=0.005)
        W = np.random.RandomState(2).uniform(-10, 0, size=(K * n, 2))
        if variant in ("zero source", "zero source, tapped"):
            nengo.Connection(zero, ea.add_neuron_input(), transform=W, synapse=None, seed=1)
        elif variant == "zero transform":
            nengo.Connection(stim[:2], ea.add_neuron_input(), transform=0.0 * W, synapse=None, seed=1)
        net.p = nengo.Probe(ea.output, synapse=0.01, seed=2)
        if variant == "zero source, tapped":
            net.tap = nengo.Probe(ea.ea_ensembles[1].neurons[3:50], seed=3)
    return net


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_a_zero_drive_changes_no_bit(Simulator, dtype):
    """A source that is identically zero against a zero transform, against no connection at all (the plain kernel, kept off the
    whole-block kernel so that both sum their decoders in the same order), and against the same run with a tap."""
    outs = {}
    for variant in ("zero source", "zero transform", "none", "zero source, tapped"):
        net = zero_drive_net(variant)
        with Simulator(None, model=build(net), dtype=dtype, block_steps=96, flags=PLAN.SSN_PLAN_NO_BLOCK_KERNEL) as sim:
            sim.run_steps(STEPS)
            no_block_kernel(sim.counters())
            outs[variant] = np.array(sim.data[net.p])
            if variant == "zero source, tapped":
                assert np.array(sim.data[net.tap]).any()
    assert np.abs(outs["none"]).max() > 0.1
    for variant in ("zero transform", "none", "zero source, tapped"):
        np.testing.assert_array_equal(outs[variant], outs["zero source"])


def test_tapped_and_driven_equals_driven(Simulator):
    model, probes, want = gated_array("sparse")
    only = build_without_taps()
    with Simulator(None, model=only[0], dtype="f32", block_steps=96) as sim:
        sim.run_steps(STEPS)
        plain = np.array(sim.data[only[1]])
    with Simulator(None, model=model, dtype="f32", block_steps=96) as sim:
        sim.run_steps(STEPS)
        tapped = np.array(sim.data[probes["out"]])
    assert np.abs(plain).max() > 0.05
    np.testing.assert_array_equal(tapped, plain)


def build_without_taps():
    """``gated_array("sparse")`` without its two neuron probes."""
    K, n = 5, 60
    with nengo.Network(seed=3) as net:
        stim = nengo.Node(lambda t: [0.8 * np.sin(7 * t + 0.4 * i) for i in range(K * 3)])
        gate = nengo.Node(window(100, 200))
        ea = nengo.EnsembleArray(n, K, ens_dimensions=3, seed=5, **RATES)
        nengo.Connection(stim, ea.input, synapse=0.005)
        out = ea.add_output("f", lambda x: [x[0], x[1], x[2], x[0] * x[1], x[2] ** 2])
        nengo.Connection(gate, ea.add_neuron_input(), transform=np.ones((K * n, 1)) * -10, synapse=None)
        p = nengo.Probe(out, synapse=0.01)
    return build(net), p


# ---- 6. ABI -------------------------------------------------------------------------------------------------------------------
def _drive_records(desc):
    at = [i for i in range(desc.n_buffers) if desc.buffers[i].kind == _lib.SSN_BUF_DRIVES]
    assert len(at) == 1 and desc.buffers[at[0]].count == 1
    return C.cast(desc.buffers[at[0]].data, C.POINTER(_lib.DriveDesc)), at[0]


def test_split_block_with_a_drive_is_refused(Simulator):
    model, probes, want = gated_array("sparse")
    with pytest.raises(nengo.BuildError, match="SSN_EUNSUPPORTED.*SSN_PLAN_SPLIT_BLOCK"):
        Simulator(None, model=model, dtype="f32", flags=PLAN.SSN_PLAN_SPLIT_BLOCK)


@pytest.mark.parametrize("what,value,message", [
    ("op", 0, "not an ensemble array"), ("op", 9999, "not an ensemble array"), ("m", 0, "columns"), ("m", 5, "columns"),
    ("w_buf", "dst_idx", "w_buf must be a real buffer"), ("src_buf", "enc", "src_buf must be an int32 buffer"),
    ("w_count", None, "w_buf must be a real buffer"), ("src_count", None, "src_buf must be an int32 buffer"),
    ("src", -2, "outside"), ("src", 10 ** 6, "outside"), ("twice", None, "already has a drive record"),
    ("two buffers", None, "at most one buffer")])
def test_ssn_create_validates_drives(Simulator, what, value, message):
    """Every record names a core ensemble array once, 1 <= m <= 4, a real buffer of K * m * n weights, an int32 buffer of K * m
    sources, each -1 or inside the signal vector; the records sit in one buffer, in front of the taps."""
    model, probes, want = gated_array("sparse")
    lib = _lib.load()
    desc, keep, _ = PLAN.pack_model(model, "f64")
    assert desc.n_buffers == len(model.buffers) + 2 and desc.buffers[desc.n_buffers - 1].kind == _lib.SSN_BUF_TAPS
    rec, at = _drive_records(desc)
    eo = [o for o in model.ops if o["kind"] == "ensarray"][0]
    if what == "op" and value == 0:
        assert model.ops[0]["kind"] != "ensarray"
    if what in ("op", "m"):
        setattr(rec[0], what, value)
    elif what in ("w_buf", "src_buf"):
        setattr(rec[0], what, eo[value])
    elif what == "w_count":
        desc.buffers[rec[0].w_buf].count -= 1
    elif what == "src_count":
        desc.buffers[rec[0].src_buf].count -= 1
    elif what == "src":
        src = np.ascontiguousarray(model.buffers[eo["drive"]["src"]], dtype=np.int32).copy()
        src[2, 0] = value
        keep.append(src)
        desc.buffers[rec[0].src_buf].data = src.ctypes.data
    elif what == "twice":
        two = (_lib.DriveDesc * 2)(rec[0], rec[0])
        keep.append(two)
        desc.buffers[at].data, desc.buffers[at].count = C.addressof(two), 2
    elif what == "two buffers":
        desc.buffers[0].kind = _lib.SSN_BUF_DRIVES
    h = C.c_void_p()
    assert lib.ssn_create(C.byref(desc), C.byref(h)) == -1, _lib.last_error()
    print(_lib.last_error())
    assert message in _lib.last_error()
