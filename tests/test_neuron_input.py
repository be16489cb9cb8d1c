"""Direct neuron input of EnsembleArray members on the CPU: ``EnsembleArray.add_neuron_input()``, the drive columns the builder
lowers such connections to, every refusal by name, and ``networks.AdditiveInputGatedMemory``.  The device side is
``test_gpu_neuron_input.py``; ``oracle.graphwalk`` (J = bias + scaled_encoders . x + direct neuron input, for array members too)
is the reference of both.  ``oracle.OracleSimulator`` is frozen and does not know drive columns."""
import hashlib

import numpy as np
import pytest

import sspslam_amd.frontend as nengo
from sspslam_amd.builder import build, op_access
from sspslam_amd.networks import AdditiveInputGatedMemory
from oracle.graphwalk import GraphWalkSimulator

from helpers import small_pathint

DT = 0.001


def ens_op(model):
    ops = [o for o in model.ops if o["kind"] == "ensarray"]
    assert len(ops) == 1
    return ops[0]


# ---- front end -----------------------------------------------------------------------------------------------------------------
def test_add_neuron_input_declares_a_node_and_one_link_per_member():
    with nengo.Network() as net:
        ea = nengo.EnsembleArray(10, 3)
        assert ea.neuron_input is None
        before = len(ea.connections)
        ni = ea.add_neuron_input()
        assert ni is ea.neuron_input and ni.size_in == 30 and ni.size_out == 30 and ni.label == "neuron_input" and ni.output is None
        links = ea.connections[before:]
        assert len(links) == 3
        for i, c in enumerate(links):
            assert c.synapse is None and c.pre.obj is ni and list(c.pre.indices) == list(range(10 * i, 10 * i + 10))
            assert c.post is ea.ea_ensembles[i].neurons
        assert ea.add_neuron_input() is ni and len(ea.connections) == before + 3 and ea.nodes.count(ni) == 1
    assert net.all_nodes.count(ni) == 1


# ---- builder -------------------------------------------------------------------------------------------------------------------
def driven_array(synapse=None):
    """3 members of 10 neurons: a two-column connection into the whole array through ``neuron_input`` and a one-column connection
    into ``member[1].neurons[2:6]`` (optionally filtered)."""
    rng = np.random.RandomState(5)
    with nengo.Network(seed=1) as net:
        stim = nengo.Node(lambda t: [0.5 * np.sin(6 * t)] * 3)
        gate = nengo.Node(lambda t: [1.0 if 0.1 < t <= 0.2 else 0.0, 0.25])
        ea = nengo.EnsembleArray(10, 3, seed=2)
        nengo.Connection(stim, ea.input, synapse=None)
        net.T2 = rng.uniform(-2, 0, size=(30, 2))
        net.T1 = rng.uniform(-3, -1, size=(4, 1))
        net.c2 = nengo.Connection(gate, ea.add_neuron_input(), transform=net.T2, synapse=None)
        net.c1 = nengo.Connection(gate[0], ea.ea_ensembles[1].neurons[2:6], transform=net.T1, synapse=synapse)
        net.p = nengo.Probe(ea.output, synapse=0.01)
        net.pn = nengo.Probe(ea.ea_ensembles[1].neurons)
    net.ea, net.gate = ea, gate
    return net


def test_drive_columns_of_the_array_operator():
    net = driven_array()
    model = build(net)
    eo = ens_op(model)
    d = eo["drive"]
    w, src = model.buffers[d["w"]], model.buffers[d["src"]]
    assert d["m"] == 3 and w.shape == (3, 3, 10) and src.shape == (3, 2 + 1) and src.dtype == np.int32
    g = model.sig[("node_out", id(net.gate))]
    assert g[1] == 2
    # columns in connection order: the two of the array-wide connection, then the member connection's one (member 1 only)
    np.testing.assert_array_equal(src, [[g[0], g[0] + 1, -1], [g[0], g[0] + 1, g[0]], [g[0], g[0] + 1, -1]])
    for k in range(3):
        np.testing.assert_array_equal(w[k, :2], net.T2[10 * k:10 * k + 10].T)
    assert not w[0, 2].any() and not w[2, 2].any()                    # unused slots: zero weights
    want = np.zeros(10)
    want[2:6] = net.T1[:, 0]
    np.testing.assert_array_equal(w[1, 2], want)                      # zero outside the sliced target
    # the sources are reads of the operator; the neuron_input node has no signal; nothing K * n wide is a signal
    reads = op_access(eo, model)[2]
    assert ("s", g[0], g[0] + 1) in reads and ("s", g[0] + 1, g[0] + 2) in reads
    assert ("node_out", id(net.ea.neuron_input)) not in model.sig and ("node_in", id(net.ea.neuron_input)) not in model.sig
    assert model.sig_size < 30 + 20
    # every such connection has built parameters (GraphWalkSimulator, sim.data[conn])
    np.testing.assert_array_equal(model.params[net.c2].weights, net.T2)
    np.testing.assert_array_equal(model.params[net.c1].weights, net.T1)
    for c in net.ea.connections:
        assert c in model.params


def test_filtered_drive_filters_its_source():
    net = driven_array(synapse=0.005)
    model = build(net)
    eo = ens_op(model)
    src = model.buffers[eo["drive"]["src"]]
    g = model.sig[("node_out", id(net.gate))]
    lows = [o for o in model.ops if o["kind"] == "lowpass" and o["src"] == g[0] and o["len"] == 1]
    assert len(lows) == 1 and lows[0]["a"] == np.exp(-DT / 0.005) and lows[0]["gain"] == 1.0
    state = lows[0]["dst"]
    s_lo = model.arena_base["S"]
    assert s_lo <= state < s_lo + model.arena_size["S"]               # the filter state lives in the S arena, m_c = 1 wide
    np.testing.assert_array_equal(src[:, 2], [-1, state, -1])
    # the array reads the state before the filter updates it: the one-step delay of a filtered connection
    kinds = [(o["kind"], o.get("dst")) for o in model.ops]
    assert kinds.index(("ensarray", None)) < kinds.index(("lowpass", state))


def test_graph_walk_steps_a_driven_array():
    net = driven_array(synapse=0.005)
    model = build(net)
    walk = GraphWalkSimulator(net, model)
    walk.run_steps(300)
    rows = walk.probe_data(net.pn)
    assert rows.shape == (300, 10) and np.isfinite(walk.probe_data(net.p)).all()


def decoded_drive_net(own_synapse=0.005):
    """A drive decoded from a plain ensemble (no synapse) into member 0, and one decoded from member 1 into member 2."""
    with nengo.Network(seed=4) as net:
        stim = nengo.Node(lambda t: [0.5 * np.sin(6 * t)] * 3)
        net.ctl = nengo.Ensemble(40, 1, seed=6)
        ea = nengo.EnsembleArray(10, 3, seed=2, label="arr")
        nengo.Connection(stim, ea.input, synapse=None)
        nengo.Connection(stim[0], net.ctl, synapse=None)
        net.c_ctl = nengo.Connection(net.ctl, ea.ea_ensembles[0].neurons, transform=-2 * np.ones((10, 1)), synapse=None, seed=7)
        net.c_own = nengo.Connection(ea.ea_ensembles[1], ea.ea_ensembles[2].neurons, transform=-2 * np.ones((10, 1)),
                                     synapse=own_synapse, seed=8)
        net.p = nengo.Probe(ea.output, synapse=0.01)
    return net


def test_a_drive_decoded_from_an_ensemble():
    """The column reads the decoded value (W arena); the transform stays in the column, ``params[c].weights`` is the full product.
    Without a synapse the source ensemble is stepped before the array within the timestep; a member of the same array may only be
    a source through a synapse, whose state the array reads before the filter updates it."""
    net = decoded_drive_net()
    model = build(net)
    eo = ens_op(model)
    src = model.buffers[eo["drive"]["src"]]
    assert eo["drive"]["m"] == 1 and src[1, 0] == -1
    w_lo, s_lo = model.arena_base["W"], model.arena_base["S"]
    assert w_lo <= src[0, 0] < w_lo + model.arena_size["W"] and s_lo <= src[2, 0] < s_lo + model.arena_size["S"]
    writers = [o for o in model.ops if any(lo <= src[0, 0] < hi for _, lo, hi in op_access(o, model)[0] + op_access(o, model)[1])]
    assert writers and all(o["kind"] != "ensarray" and o["level"] < eo["level"] for o in writers)
    low = [o for o in model.ops if o["kind"] == "lowpass" and o["dst"] == src[2, 0]]
    assert len(low) == 1 and low[0]["len"] == 1 and low[0]["src"] in model.buffers[eo["dst_idx"]][1]
    assert model.params[net.c_ctl].weights.shape == (10, 40) and model.params[net.c_own].weights.shape == (10, 10)
    walk = GraphWalkSimulator(net, model)
    walk.run_steps(100)
    assert np.isfinite(walk.probe_data(net.p)).all()


def test_a_network_without_neuron_input_lowers_as_before():
    """``small_pathint(ssp_dim=7, n=64)`` as the parent commit built it: 26 operators in this order, 152 signals, 12 buffers whose
    bytes hash to e8f6a06898eb6b2f..., boundaries pre->core [(0, 12)] and core->post [(92, 103)] (recorded from the parent)."""
    model = build(small_pathint(ssp_dim=7, n=64).model)
    assert [o["kind"] for o in model.ops] == [
        "fill", "fill", "table", "table", "axpy", "axpy", "axpy", "axpy", "axpy", "matvec", "matvec", "axpy", "lowpass", "lowpass",
        "axpy", "axpy", "ensarray", "lowpass", "fill", "fill", "axpy", "axpy", "axpy", "lowpass", "matvec", "lowpass"]
    assert model.sig_size == 152
    assert [b.shape for b in model.buffers] == [(12, 7), (3, 2), (3, 2), (3, 2), (7, 12), (4, 3, 64), (4, 64), (4, 4, 64), (4, 64),
                                                (4, 64), (4, 4), (9, 2)]
    h = hashlib.sha256()
    for b in model.buffers:
        h.update(np.ascontiguousarray(b).tobytes())
    assert h.hexdigest()[:16] == "e8f6a06898eb6b2f"
    assert model.stage_info["pre_to_core"] == [(0, 12)] and model.stage_info["core_to_post"] == [(92, 103)]
    assert "drive" not in ens_op(model)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _array(n_cols=1, width=None):
    net = nengo.Network(seed=3)
    with net:
        net.src = nengo.Node(lambda t: [0.0] * (width or n_cols))
        net.ea = nengo.EnsembleArray(10, 3, label="arr")
        nengo.Probe(net.ea.output)
    return net


def test_five_columns_are_refused():
    net = _array()
    with net:
        for _ in range(5):
            nengo.Connection(net.src, net.ea.ea_ensembles[2].neurons, transform=-np.ones((10, 1)), synapse=None)
    with pytest.raises(nengo.BuildError, match=r"'arr'.*5 neuron-input columns"):
        build(net)
    wide = _array(5)
    with wide:
        nengo.Connection(wide.src, wide.ea.add_neuron_input(), transform=-np.ones((30, 5)), synapse=None)
    with pytest.raises(nengo.BuildError, match=r"'arr'.*5 neuron-input columns"):
        build(wide)


def test_an_n_wide_identity_source_is_refused():
    net = _array(width=10)
    with net:
        nengo.Connection(net.src, net.ea.ea_ensembles[0].neurons, synapse=None)
    with pytest.raises(nengo.BuildError, match="not a column form"):
        build(net)


def test_an_unsynapsed_drive_decoded_from_the_same_array_is_refused():
    """The array operator would read, in one launch, a signal that another of its workgroups writes."""
    with pytest.raises(nengo.BuildError, match=r"without a synapse decoded from a member of the same EnsembleArray 'arr'"):
        build(decoded_drive_net(own_synapse=None))


def test_a_connection_out_of_neuron_input_is_refused():
    net = _array()
    with net:
        ni = net.ea.add_neuron_input()
        nengo.Connection(net.src, ni, transform=-np.ones((30, 1)), synapse=None)
        sink = nengo.Node(size_in=30)
        nengo.Connection(ni, sink, synapse=None)
        nengo.Probe(sink)
    with pytest.raises(nengo.BuildError, match="connection out of the neuron_input node"):
        build(net)


def test_a_probe_on_neuron_input_is_refused():
    net = _array()
    with net:
        ni = net.ea.add_neuron_input()
        nengo.Connection(net.src, ni, transform=-np.ones((30, 1)), synapse=None)
        nengo.Probe(ni)
    with pytest.raises(nengo.BuildError, match="probing the neuron_input node"):
        build(net)


@pytest.mark.parametrize("kw,name", [(dict(vco_shard=(0, 2)), "vco_shard"), (dict(neuron_shard=(0, 2)), "neuron_shard")])
def test_sharded_builds_with_a_driven_array_are_refused(kw, name):
    net = _array()
    with net:
        nengo.Connection(net.src, net.ea.add_neuron_input(), transform=-np.ones((30, 1)), synapse=None)
    with pytest.raises(nengo.BuildError, match=r"neuron input.*'arr'.*sharding.*" + name):
        build(net, **kw)


# ---- AdditiveInputGatedMemory --------------------------------------------------------------------------------------------------
STIM = [0.2, -0.15, 0.1, -0.2]


def gated_memory(cls, ea_cls, d=4, n=50):
    with nengo.Network(seed=7) as net:
        stim = nengo.Node(lambda t: STIM[:d])
        gate = nengo.Node(lambda t: [0.0 if t <= 0.3 else 1.0])
        reset = nengo.Node(lambda t: [1.0 if t > 0.6 else 0.0])
        inp = ea_cls(n, d, label="inp", seed=11)
        nengo.Connection(stim, inp.input, synapse=None)
        # (rates of at most 100 Hz keep bias + |encoders| below 3.04 = the current of a 100 Hz LIF neuron: the class's reset
        #  weight of -3 then silences the memory)
        wm = cls(inp.output, [inp], n, d, seed=12, max_rates=nengo.Uniform(50, 100))
        nengo.Connection(gate, wm.gate, synapse=None)
        nengo.Connection(reset, wm.reset, synapse=None)
        net.p = nengo.Probe(wm.output, synapse=0.01)
    net.wm, net.inp = wm, inp
    return net


def check_memory_behaviour(out):
    """Gate open for 300 ms: the integrator (tau 0.1) adds up its input, about 3 x of it; gate closed for 300 ms: what the
    difference synapse (tau 0.1) still holds drains into the memory for a while, then the value stands - compared between 200 and
    290 ms after the gate closed; reset for 300 ms: with its neurons silent the value decays as exp(-t / 0.1), to 5 % after 290 ms."""
    target = np.array(STIM)
    loaded, held0, held, cleared = out[290], out[500], out[590], out[890]
    print("memory: loaded %s held %s -> %s cleared %s" % (np.round(loaded, 3), np.round(held0, 3), np.round(held, 3), np.round(cleared, 3)))
    cos = np.dot(loaded, target) / (np.linalg.norm(target) * np.linalg.norm(loaded))
    assert cos > 0.9 and np.linalg.norm(loaded) > np.linalg.norm(target)     # gate open: the memory follows (integrates) its input
    assert np.linalg.norm(held - held0) < 0.15 * np.linalg.norm(held0) and np.linalg.norm(held) > np.linalg.norm(target)   # closed: it holds
    assert np.linalg.norm(cleared) < 0.15 * np.linalg.norm(held)             # reset: empty


def census(net):
    return (len(net.all_nodes), len(net.all_ensembles), len(net.all_connections),
            sorted((n.label or "", n.size_in) for n in net.all_nodes))


def test_additive_input_gated_memory_census_build_and_walk():
    d, n = 4, 50
    net = gated_memory(AdditiveInputGatedMemory, nengo.EnsembleArray, d, n)
    wm = net.wm
    assert isinstance(wm.mem, nengo.EnsembleArray) and wm.output is wm.mem.output
    assert wm.gate.size_in == 1 and wm.reset.size_in == 1 and wm.mem.neuron_input.size_in == n * d
    assert net.inp.neuron_input is not None and net.inp.neuron_input.size_in == n * d
    # the class's own objects: mem (input, output, neuron_input + d members) + gate + reset; connections: mem's 2 d + d member
    # links, feedback, difference, one gate connection per gated array, reset
    assert len(wm.all_nodes) == 5 and len(wm.all_ensembles) == d
    assert len(wm.all_connections) == 3 * d + 4
    model = build(net)
    drives = {o["label"]: o["drive"] for o in model.ops if o["kind"] == "ensarray"}
    assert set(drives) == {"inp", "mem"} and all(v["m"] == 1 for v in drives.values())
    np.testing.assert_array_equal(model.buffers[drives["inp"]["w"]], np.full((d, 1, n), -10.0))
    np.testing.assert_array_equal(model.buffers[drives["mem"]["w"]], np.full((d, 1, n), -3.0))
    walk = GraphWalkSimulator(net, model)
    walk.run_steps(900)
    out = walk.probe_data(net.p)
    check_memory_behaviour(out)


def test_reference_working_memory_class_on_our_stack(golden):
    """The reference's own ``AdditiveInputGatedMemory``, loaded from a checkout with zero edits and this object model registered as
    ``import nengo``, builds to the same census, operators and buffers as ours: what it built is recorded in
    ``tests/golden/neuron_input_dropin.npz`` (``tests/golden/make_neuron_input_golden.py``, which also compares the two live)."""
    ours = gated_memory(AdditiveInputGatedMemory, nengo.EnsembleArray)
    model = build(ours)
    with golden("neuron_input_dropin.npz") as z:
        n_nodes, n_ens, n_conn, nodes = census(ours)
        np.testing.assert_array_equal(z["census"], [n_nodes, n_ens, n_conn])
        assert [str(v) for v in z["node_labels"]] == [lb for lb, _ in nodes]
        np.testing.assert_array_equal(z["node_size_in"], [sz for _, sz in nodes])
        assert [str(v) for v in z["op_kinds"]] == [o["kind"] for o in model.ops]
        assert int(z["sig_size"]) == model.sig_size and int(z["n_buffers"]) == len(model.buffers)
        for i, b in enumerate(model.buffers):
            np.testing.assert_array_equal(z[f"buffer_{i}"], np.asarray(b))
