"""Neuron probes on EnsembleArray members on the device: the taps of every ensemble kernel.

* f64, exact against ``oracle.graphwalk`` (``test_neuron_taps.py`` proves that reference against the stepper's state): the
  whole-block kernel, the per-timestep fused kernel, the round grid and the one-launch-per-operator plan; LIFRate members; a
  small SLAMNetwork (an oscillator and a product ensemble of a circular convolution).
* f32, exact by construction on the open-loop model of ``lif_open_loop.py``: its integer decoder rows (count, checksum, one
  neuron's train) are sums over the same spikes the taps report, so they agree in any summation order - all seven variants of
  the whole-block kernel, the per-timestep kernel, two block lengths.
* a run with taps equals the run without them in every other probe, bit for bit.

Every case asserts through ``counters()`` which kernel ran."""
import numpy as np
import pytest

import sspslam_amd.frontend as nengo
from sspslam_amd import harness as H
from sspslam_amd import simulator as PLAN
from sspslam_amd import _lib
from sspslam_amd.builder import build
from oracle import OracleSimulator
from oracle.graphwalk import GraphWalkSimulator

import lif_open_loop as L
from helpers import small_pathint
from test_gpu_lif_open_loop import F32_VARIANTS, assert_kernel, forced

pytestmark = pytest.mark.gpu

DT = 0.001


@pytest.fixture(scope="module")
def Simulator():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from sspslam_amd.simulator import Simulator
    return Simulator


# ---- f64, exact against the graph walk ---------------------------------------------------------------------------------
_PATHINT = {}


def tapped_pathint(ssp_dim, n, steps=300):
    """(model, probes, graph-walk rows per probe, stepper rows of the decoded probe): built and stepped once per shape."""
    key = (ssp_dim, n)
    if key not in _PATHINT:
        pm = small_pathint(ssp_dim=ssp_dim, n=n, T=10.0, limit=0.2)
        ens = pm.pathintegrator.oscillators.ea_ensembles
        with pm.model:
            probes = {"all": nengo.Probe(ens[1].neurons, synapse=None),
                      "mid": nengo.Probe(ens[2].neurons[5:37], synapse=None, sample_every=7 * DT),
                      "end": nengo.Probe(ens[-1].neurons[n - 3:n], synapse=0.01)}
        model = build(pm.model)
        walk = GraphWalkSimulator(pm.model, model)
        walk.run_steps(steps)
        ref = OracleSimulator(model)
        ref.run_steps(steps)
        decoded = ref.probe_data([i for i, p in enumerate(model.probes) if p["probe"] is pm.probe][0])
        want = {name: np.array(walk.probe_data(p)) for name, p in probes.items()}
        assert want["all"].shape == (steps, n) and want["mid"].shape == (steps // 7, 32) and want["end"].shape == (steps, 3)
        counts = {name: int((w != 0).sum()) for name, w in want.items()}
        print("graph walk d=%d n=%d: nonzero samples %s" % (ssp_dim, n, counts))
        assert counts["all"] > steps and counts["mid"] > 10, counts
        _PATHINT[key] = (pm, model, probes, want, decoded)
    return _PATHINT[key]


NO_ITEM_PLAN = PLAN.SSN_PLAN_NO_FUSED_CORE | PLAN.SSN_PLAN_NO_ROUNDS
F64_PLANS = [("block", 0), ("per-timestep", PLAN.SSN_PLAN_NO_BLOCK_KERNEL), ("rounds", PLAN.SSN_PLAN_NO_FUSED_CORE),
             ("no-rounds", PLAN.SSN_PLAN_NO_ROUNDS), ("items", NO_ITEM_PLAN)]


@pytest.mark.parametrize("plan,flags", F64_PLANS)
@pytest.mark.parametrize("ssp_dim,n", [(7, 64), (55, 60)])
def test_f64_taps_equal_the_graph_walk(Simulator, ssp_dim, n, plan, flags):
    """Member 1 ``[:]``, member 2 ``[5:37]`` every 7 steps, the last member ``[n-3:n]`` through a 10 ms probe synapse; 300 steps in
    blocks of 96; a reset and the same run again."""
    steps = 300
    pm, model, probes, want, decoded = tapped_pathint(ssp_dim, n, steps)
    with Simulator(None, model=model, dtype="f64", block_steps=96, flags=flags) as sim:
        runs = []
        for _ in range(2):
            sim.run_steps(steps)
            c = sim.counters()
            if plan in ("block", "no-rounds"):
                assert c["launches_per_step"] == 0 and c["block_tpb"] == 1024, c
            else:
                assert c["launches_per_step"] >= 1 and c["block_tpb"] == 0, c
            runs.append({name: np.array(sim.data[p]) for name, p in list(probes.items()) + [("decoded", pm.probe)]})
            sim.reset()
    got = runs[0]
    for name in ("all", "mid"):
        mism = int((got[name] != want[name]).sum())
        print("%s d=%d n=%d %s: %d spikes, %d mismatches" % (plan, ssp_dim, n, name, int((want[name] != 0).sum()), mism))
    np.testing.assert_array_equal(got["all"], want["all"])
    np.testing.assert_array_equal(got["mid"], want["mid"])
    np.testing.assert_allclose(got["end"], want["end"], atol=1e-9, rtol=0)
    err = float(np.max(H.cosine_error(got["decoded"][20:], decoded[20:])))
    print("decoded probe: max cosine error vs the stepper %.3e" % err)
    assert err < 1e-9
    for name in got:
        np.testing.assert_array_equal(runs[1][name], got[name])


@pytest.mark.parametrize("flags", [0, NO_ITEM_PLAN])
def test_f64_lifrate_members(Simulator, flags):
    """An array of LIFRate members (the generic body of the array kernel): the tap is amplitude * rate, rtol 1e-9."""
    steps = 120
    with nengo.Network(seed=4) as net:
        stim = nengo.Node(lambda t: [0.8 * np.sin(9 * t), 0.6 * np.cos(5 * t), 0.5, -0.4 * np.sin(3 * t), 0.9 * np.cos(11 * t)])
        ea = nengo.EnsembleArray(45, 5, neuron_type=nengo.LIFRate(amplitude=0.5))
        nengo.Connection(stim, ea.input, synapse=0.005)
        p_out = nengo.Probe(ea.output, synapse=0.01)
        p_a = nengo.Probe(ea.ea_ensembles[0].neurons)
        p_b = nengo.Probe(ea.ea_ensembles[3].neurons[7:40], sample_every=3 * DT)
    model = build(net)
    walk = GraphWalkSimulator(net, model)
    walk.run_steps(steps)
    with Simulator(None, model=model, dtype="f64", flags=flags) as sim:
        sim.run_steps(steps)
        for p in (p_a, p_b):
            a, b = np.array(sim.data[p]), walk.probe_data(p)
            assert a.shape == b.shape and b.max() > 10.0
            np.testing.assert_allclose(a, b, rtol=1e-9, atol=0)
        np.testing.assert_allclose(np.array(sim.data[p_out]), walk.probe_data(p_out), atol=1e-9, rtol=0)


@pytest.mark.parametrize("flags", [0, PLAN.SSN_PLAN_ENS_OWN_LAUNCH])
def test_f64_slam_oscillator_and_product_member(Simulator, flags):
    """SLAMNetwork at the shape of ``test_slam_lowering_equals_the_graph_walk``, 200 steps: an oscillator ``[:40]`` and all neurons of
    a product ensemble of a circular convolution (15 neurons, one input, one decoded row: the array that normally takes the
    wave-per-ensemble body of the round grid - with a tap it takes the general one, or its own launch)."""
    steps = 200
    s = H.make_ssp_space(2, 55)
    path, vels = H.make_random_path(20.0, limit=0.1, seed=0)
    sm = H.make_slam_model(s, path, vels, n_landmarks=10, pi_n_neurons=60, mem_n_neurons=120, circonv_n_neurons=30,
                           view_rad=0.6)
    with sm.model:
        p_osc = nengo.Probe(sm.slam.pathintegrator.oscillators.ea_ensembles[3].neurons[:40], synapse=None)
        p_prod = nengo.Probe(sm.slam.position_estimate.product.sq1.ea_ensembles[17].neurons, synapse=None)
    model = build(sm.model)
    walk = GraphWalkSimulator(sm.model, model)
    walk.run_steps(steps)
    ref = OracleSimulator(model)
    ref.run_steps(steps)
    want_out = ref.probe_data([i for i, p in enumerate(model.probes) if p["probe"] is sm.probe][0])
    with Simulator(None, model=model, dtype="f64", flags=flags) as sim:
        sim.run_steps(steps)
        assert sim.counters()["launches_per_step"] >= 1
        for p in (p_osc, p_prod):
            a, b = np.array(sim.data[p]), walk.probe_data(p)
            print(p, "spikes", int((b != 0).sum()), "mismatches", int((a != b).sum()))
            assert a.shape == b.shape and (b != 0).sum() > 20
            np.testing.assert_array_equal(a, b)
        np.testing.assert_allclose(np.array(sim.data[sm.probe]), want_out, atol=1e-9, rtol=0)


@pytest.mark.parametrize("flags", [0, NO_ITEM_PLAN])
def test_f64_tap_on_the_second_of_two_arrays(Simulator, flags):
    """Two arrays of K = 2 members of 64 neurons, the tap on the second one only (taps belong to an operator by its index in the
    model, and the first array has none to be mistaken for); 20 steps, spike for spike."""
    steps = 20
    with nengo.Network(seed=14) as net:
        stim = nengo.Node(lambda t: [0.8 * np.sin(40 * t), 0.6 * np.cos(30 * t)])
        first = nengo.EnsembleArray(64, 2, seed=15)
        second = nengo.EnsembleArray(64, 2, seed=16)
        nengo.Connection(stim, first.input, synapse=0.005)
        nengo.Connection(stim, second.input, synapse=0.005)
        p_first = nengo.Probe(first.output, synapse=0.01)
        p_tap = nengo.Probe(second.ea_ensembles[1].neurons, synapse=None)
        p_out = nengo.Probe(second.output, synapse=0.01)
    model = build(net)
    assert ["taps" in o for o in model.ops if o["kind"] == "ensarray"] == [False, True]
    walk = GraphWalkSimulator(net, model)
    walk.run_steps(steps)
    want = np.array(walk.probe_data(p_tap))
    assert want.shape == (steps, 64) and (want != 0).sum() > 50
    with Simulator(None, model=model, dtype="f64", flags=flags) as sim:
        sim.run_steps(steps)
        got = np.array(sim.data[p_tap])
        print("flags %d: %d spikes, %d mismatches" % (flags, int((want != 0).sum()), int((got != want).sum())))
        np.testing.assert_array_equal(got, want)
        for p in (p_first, p_out):
            np.testing.assert_allclose(np.array(sim.data[p]), walk.probe_data(p), atol=1e-9, rtol=0)


# ---- f32, exact by construction --------------------------------------------------------------------------------------
def open_loop_with_taps(monkeypatch, n, slices):
    """``lif_open_loop.open_loop_pathint(n, ssp_dim=7)`` with neuron probes on the members ``slices`` names, added before its
    build.  -> (ol, {member: probe key}).  ``open_loop_pathint`` deep-copies the built model, probe objects included, so the keys
    are those of the copy (as ``ol.probe_key()`` is): found by their place in ``model.probes``."""
    real = L.build_model
    index = {}

    def build_with_probes(net, **kw):
        (osc,) = [sub for sub in net.all_networks if getattr(sub, "ea_ensembles", None)]
        with net:
            added = {k: nengo.Probe(osc.ea_ensembles[k].neurons[sl], synapse=None, sample_every=7 * DT)
                     for k, sl in slices.items()}
        model = real(net, **kw)
        for k, probe in added.items():
            (index[k],) = [i for i, p in enumerate(model.probes) if p["probe"] is probe]
        return model

    monkeypatch.setattr(L, "build_model", build_with_probes)
    ol = L.open_loop_pathint(n, ssp_dim=7)
    monkeypatch.setattr(L, "build_model", real)
    assert ol.K == 4 and sorted(index) == sorted(slices)
    keys = {k: ol.probe_key(i) for k, i in index.items()}
    for k, i in index.items():
        assert ol.model.probes[i]["every"] == 7 and "src" in ol.model.probes[i], ol.model.probes[i]
    return ol, keys


def run_open_loop(Simulator, ol, probes, variant, block, steps=1000, **sim_kw):
    with forced(variant), Simulator(None, model=ol.model, dtype="f32", **sim_kw) as sim:
        sim.run_steps(steps)
        assert_kernel(sim.counters(), variant, block)
        obs = L.observed(ol, sim.data[ol.probe_key()])                       # [steps, K, 3]: count, checksum, train
        taps = {k: np.array(sim.data[p], dtype=np.float64) for k, p in probes.items()}
    return obs, taps


def check_open_loop_taps(Simulator, monkeypatch, n, variant, block=True, steps=1000, **sim_kw):
    amp = 1.0 / DT
    part = slice(3, n - 5)
    ol, probes = open_loop_with_taps(monkeypatch, n, {1: slice(None), 2: slice(None), 3: part})
    obs, taps = run_open_loop(Simulator, ol, probes, variant, block, steps, **sim_kw)
    at = np.arange(7, steps + 1, 7) - 1                       # rows of the every-step probe at the sampled steps
    weights = (np.arange(n) % L.CHECKSUM_MOD) + 1.0
    for k in (1, 2):
        t = taps[k]
        assert t.shape == (len(at), n)
        assert np.isin(t, (0.0, amp)).all()
        spk = t / amp                                         # tap * dt / amplitude: the spike indicator
        print("n %d %s member %d: %d spikes in %d samples" % (n, variant, k, int(spk.sum()), len(at)))
        assert spk.sum() > 0
        np.testing.assert_array_equal(spk.sum(axis=1), obs[at, k, L.COUNT])
        np.testing.assert_array_equal(spk @ weights, obs[at, k, L.CHECKSUM])
        np.testing.assert_array_equal(spk[:, ol.hot[k]], obs[at, k, L.TRAIN])
    # the partial slice against the same columns of a full tap from a second run
    ol2, probes2 = open_loop_with_taps(monkeypatch, n, {3: slice(None)})
    obs2, taps2 = run_open_loop(Simulator, ol2, probes2, variant, block, steps, **sim_kw)
    np.testing.assert_array_equal(obs2, obs)
    assert taps[3].shape == (len(at), n - 8) and np.isin(taps[3], (0.0, amp)).all() and taps[3].sum() > 0
    np.testing.assert_array_equal(taps[3], taps2[3][:, part])
    np.testing.assert_array_equal(taps2[3].sum(axis=1) / amp, obs[at, 3, L.COUNT])


@pytest.mark.parametrize("variant,n", [(v, cap) for v, cap, _ in F32_VARIANTS] + [(v, rag) for v, _, rag in F32_VARIANTS])
def test_f32_block_variant_taps(Simulator, monkeypatch, variant, n):
    check_open_loop_taps(Simulator, monkeypatch, n, variant)


def test_f32_per_timestep_kernel_taps(Simulator, monkeypatch):
    check_open_loop_taps(Simulator, monkeypatch, 12000, None, block=False, flags=PLAN.SSN_PLAN_NO_BLOCK_KERNEL)


@pytest.mark.parametrize("block_steps", [96, 1000])
def test_f32_block_lengths(Simulator, monkeypatch, block_steps):
    check_open_loop_taps(Simulator, monkeypatch, 5111, "512,10,0", block_steps=block_steps)


# ---- tapped equals untapped ----------------------------------------------------------------------------------------------
def _with_and_without_taps(pm, n, **build_kw):
    plain = build(pm.model, **build_kw)
    ens = pm.pathintegrator.oscillators.ea_ensembles
    with pm.model:
        ps = [nengo.Probe(ens[0].neurons, synapse=None), nengo.Probe(ens[2].neurons[1:n - 2], synapse=None, sample_every=5 * DT)]
    return plain, build(pm.model, **build_kw), ps


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("flags", [0, PLAN.SSN_PLAN_NO_BLOCK_KERNEL, PLAN.SSN_PLAN_NO_FUSED_CORE])
def test_tapped_run_equals_untapped_run_bit_for_bit(Simulator, dtype, flags):
    steps = 300
    pm = small_pathint(ssp_dim=7, n=64, T=10.0, limit=0.2)
    plain, tapped, ps = _with_and_without_taps(pm, 64)
    outs = []
    for model in (plain, tapped):
        with Simulator(None, model=model, dtype=dtype, block_steps=96, flags=flags) as sim:
            sim.run_steps(steps)
            outs.append(np.array(sim.data[pm.probe]))
            if model is tapped:
                assert all(np.array(sim.data[p]).any() for p in ps)
    assert np.abs(outs[0]).max() > 0.05
    np.testing.assert_array_equal(outs[0], outs[1])


def test_tapped_run_equals_untapped_run_headline_variant(Simulator):
    """(512, 20, LDS) forced at n = 10 223, 200 steps, f32."""
    n, steps = 10223, 200
    pm = small_pathint(ssp_dim=7, n=n, T=10.0, limit=0.2)
    plain, tapped, ps = _with_and_without_taps(pm, n, n_eval_points=300)
    outs = []
    for model in (plain, tapped):
        with forced("512,20,3"), Simulator(None, model=model, dtype="f32") as sim:
            sim.run_steps(steps)
            assert_kernel(sim.counters(), "512,20,3", True)
            outs.append(np.array(sim.data[pm.probe]))
            if model is tapped:
                assert all(np.array(sim.data[p]).any() for p in ps)
    assert np.abs(outs[0]).max() > 0.05
    np.testing.assert_array_equal(outs[0], outs[1])


# ---- ABI -----------------------------------------------------------------------------------------------------------------
def test_split_block_with_taps_is_refused(Simulator):
    pm, model, probes, want, decoded = tapped_pathint(7, 64)
    with pytest.raises(nengo.BuildError, match="SSN_EUNSUPPORTED.*SSN_PLAN_SPLIT_BLOCK"):
        Simulator(None, model=model, dtype="f32", flags=PLAN.SSN_PLAN_SPLIT_BLOCK)


def _tap_records(desc):
    import ctypes as C
    last = desc.buffers[desc.n_buffers - 1]
    assert last.kind == _lib.SSN_BUF_TAPS and last.count == desc.n_taps
    return C.cast(last.data, C.POINTER(_lib.TapDesc))


@pytest.mark.parametrize("field,value", [("count", 65), ("first", -1), ("k", 99), ("dst", -5), ("op", 0)])
def test_ssn_create_validates_taps(Simulator, field, value):
    """Ranges inside n and K, dst inside the signal vector, an ensemble-array operator; no overlap between two taps; the records
    where the descriptor says they are."""
    import ctypes as C
    pm, model, probes, want, decoded = tapped_pathint(7, 64)
    lib = _lib.load()
    desc, keep, _ = PLAN.pack_model(model, "f64")
    assert desc.n_taps == 3 and desc.n_buffers == len(model.buffers) + 1
    if field == "op":
        assert model.ops[0]["kind"] != "ensarray"
    setattr(_tap_records(desc)[1], field, value)
    h = C.c_void_p()
    assert lib.ssn_create(C.byref(desc), C.byref(h)) == -1, _lib.last_error()
    desc, keep, _ = PLAN.pack_model(model, "f64")
    _tap_records(desc)[2].dst = _tap_records(desc)[0].dst + 1
    assert lib.ssn_create(C.byref(desc), C.byref(h)) == -1 and "overlap" in _lib.last_error()
    desc, keep, _ = PLAN.pack_model(model, "f64")
    desc.n_taps = 2
    assert lib.ssn_create(C.byref(desc), C.byref(h)) == -1 and "SSN_BUF_TAPS" in _lib.last_error()
