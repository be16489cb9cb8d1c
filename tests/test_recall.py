"""Map recall without a GPU: the instrument of tests/recall_checks.py passes the NumPy-f32 restatement of the kernels and fails each
wrong device; MapProbe lowers, is refused by name where the kernels do not reach, and enters the cache key with its keys and mode; the
C ABI fails loudly without a device; harness.map_over_time is the per-sample host decode.

Worst err / B of the restatement over the three shapes and both modes: 1.5e-2."""
import ctypes as C

import numpy as np
import pytest

import recall_checks as rc

MODES = ("reference", "network")


@pytest.fixture(scope="module", params=rc.SHAPES, ids=str)
def state(request):
    return rc.synthetic_state(*request.param)


def args_of(st, mode):
    return st["keys"], st["E"], st["W"], st["gain"], st["bias"], rc.LIF, mode


# -- the instrument -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_f32_restatement_passes(state, mode):
    worst = rc.check(rc.emulate_f32(*args_of(state, mode)), *args_of(state, mode), rc.U32, "NumPy f32")
    assert worst <= 0.1      # (measured: at most 1.5e-2 - a restatement near the bound would say the bound prices nothing)
    rc.check(rc.recall_f64(*args_of(state, mode)), *args_of(state, mode), rc.U64, "NumPy f64")


@pytest.mark.parametrize("fault", rc.FAULTS)
@pytest.mark.parametrize("mode", MODES)
def test_wrong_devices_fail(state, mode, fault):
    q = rc.emulate_f32(*args_of(state, mode), fault=fault, W_prev=state["W_prev"])
    with pytest.raises(AssertionError, match="exceeds B"):
        rc.check(q, *args_of(state, mode), rc.U32, fault)


def test_rate_populations_and_condition():
    st = rc.synthetic_state(*rc.SHAPES[1])
    relu = dict(type="relu", tau_rc=0.0, tau_ref=0.0, amplitude=1.0)
    for neuron in (dict(rc.LIF, type="lifrate"), relu):
        a = st["keys"], st["E"], st["W"], st["gain"], st["bias"], neuron, "network"
        rc.check(rc.emulate_f32(*a), *a, rc.U32, neuron["type"])
    # inputs whose recall cancels violate the condition, and the instrument says so instead of passing a loose bound
    W = st["W"] * np.where(np.arange(st["W"].shape[1]) % 2, 1.0, -1.0)[None, :] * 1e3
    a = st["keys"], st["E"] * 40.0, W, st["gain"], st["bias"], rc.LIF, "reference"
    q, B = rc.bound(*a, rc.U32)
    if rc.condition(q, B) > rc.CONDITION:
        with pytest.raises(AssertionError, match="choose another seed"):
            rc.check(q, *a, rc.U32, "cancelling")


# -- MapProbe on the CPU ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    from sspslam_amd.builder import build
    net, o = rc.memory_network(*rc.SHAPES[0])
    return net, o, build(net)


def test_map_probe_lowers_beside_the_buffer_probes(small):
    net, o, model = small
    mem = o["memory"]
    assert len(model.map_probes) == 2 and all("src" in p or "buf" in p for p in model.probes)
    be, bc = model.params[mem.memory], model.params[mem.conn_out]
    for mode in MODES:
        entry = [p for p in model.map_probes if p["probe"] is o["map_probes"][mode]][0]
        spec = entry["recall"]
        assert entry["every"] == rc.EVERY and entry["shape"] == (rc.N_KEYS, rc.SHAPES[0][2])
        assert (spec["enc"], spec["dec"], spec["n"], spec["d_key"], spec["d_val"]) == (be.encoder_buffer, bc.learned_buffer) + rc.SHAPES[0]
        np.testing.assert_array_equal(spec["scale"], be.gain if mode == "reference" else np.ones(rc.SHAPES[0][0]))
        np.testing.assert_array_equal(spec["bias"], be.bias)
        np.testing.assert_array_equal(spec["keys"], o["keys"])
        assert spec["neuron"]["type"] == "lif"
    # the NumPy oracle steps the same model: a MapProbe adds no operator and no signal
    from sspslam_amd.builder import build
    from oracle import OracleSimulator
    net2, o2 = rc.memory_network(*rc.SHAPES[0], map_modes=())
    plain = build(net2)
    assert [op["kind"] for op in plain.ops] == [op["kind"] for op in model.ops] and plain.sig_size == model.sig_size
    ref = OracleSimulator(model)
    ref.run_steps(60)
    # ... and its learned state meets the instrument's condition with the host definition as the device
    E, W = np.array(ref.buf[be.encoder_buffer]), np.array(ref.buf[bc.learned_buffer])
    assert np.any(W != 0) and np.any(E != be.scaled_encoders)
    from sspslam_amd import frontend as nengo
    x = o["keys"] @ E.T
    host = nengo.LIF().rates(x, be.gain, be.bias) @ W.T                  # harness.map_recall_learned's arithmetic
    rc.check(host, o["keys"], E, W, be.gain, be.bias, be.neuron, "reference", rc.U64, "host definition")


def test_refusals_by_name():
    from sspslam_amd import MapProbe
    from sspslam_amd import frontend as nengo
    from sspslam_amd.builder import build, recall_spec
    from sspslam_amd.networks.associativememory import AssociativeMemory
    keys = rc.unit_rows(np.random.RandomState(0), 4, 7)
    with nengo.Network(seed=1) as net:
        key_in = nengo.Node(lambda t: keys[0])
        mem = AssociativeMemory(100, 7, 5, 0.1, seed=1)
        nengo.Connection(key_in, mem.key_input, synapse=None)
        plain = nengo.Connection(mem.memory, mem.recall, synapse=0.01, transform=np.zeros((5, 7)))
        ea = nengo.EnsembleArray(50, 3)
        other = nengo.Ensemble(60, 7)
        nengo.Connection(key_in, other, synapse=None)
        with pytest.raises(nengo.ValidationError, match="keys of shape"):
            MapProbe(mem, np.zeros((4, 8)))
        with pytest.raises(nengo.ValidationError, match="no learned buffer"):
            MapProbe((mem.memory, plain), keys)
        with pytest.raises(nengo.ValidationError, match="not a connection out of"):
            MapProbe((other, mem.conn_out), keys)
        with pytest.raises(nengo.ValidationError, match="not a connection out of"):
            MapProbe((ea.ea_ensembles[0], mem.conn_out), keys)
        with pytest.raises(nengo.ValidationError, match="mode"):
            MapProbe(mem, keys, mode="twice")
        with pytest.raises(nengo.ValidationError, match="AssociativeMemory or a pair"):
            MapProbe(mem.memory, keys)
        nengo.Probe(mem.recall, synapse=0.01)
    model = build(net)
    with pytest.raises(nengo.BuildError, match="keys of shape"):
        recall_spec(model, mem, np.zeros((4, 8)))
    with pytest.raises(nengo.BuildError, match="mode"):
        recall_spec(model, mem, keys, mode="twice")
    assert recall_spec(model, (mem.conn_in, mem.conn_out), keys, "network")["scale"].max() == 1.0
    # populations the kernels do not cover carry the reason from the build
    model.params[mem.memory].recall_refusal = "is neuron-sharded"
    with pytest.raises(nengo.BuildError, match="neuron-sharded"):
        recall_spec(model, mem, keys)
    model.params[mem.memory].recall_refusal = None
    assert model.params[ea.ea_ensembles[0]].recall_refusal == "is an EnsembleArray member"
    # a neuron-sharded or replicated build refuses the probe itself
    for kw, word in ((dict(neuron_shard=(0, 2)), "neuron-sharded"), (dict(neuron_shard=(0, 2), replicate=[mem.memory]), "replicated")):
        with nengo.Network(seed=1) as net2:
            k2 = nengo.Node(lambda t: keys[0])
            mem2 = AssociativeMemory(100, 7, 5, 0.1, seed=1)
            nengo.Connection(k2, mem2.key_input, synapse=None)
            nengo.Probe(mem2.recall, synapse=0.01)
            MapProbe(mem2, keys)
        if "replicate" in kw:
            kw["replicate"] = [mem2.memory]
        with pytest.raises(nengo.BuildError, match=word):
            build(net2, **kw)


def test_cache_key_follows_keys_and_mode():
    from sspslam_amd import MapProbe, modelcache

    def digest(keys, mode, with_probe=True):
        net, o = rc.memory_network(*rc.SHAPES[0], map_modes=())
        if with_probe:
            with net:
                MapProbe(o["memory"], keys, sample_every=0.05, mode=mode)
        return modelcache.fingerprint(net)

    keys = rc.unit_rows(np.random.RandomState(2), 6, 7)
    base = digest(keys, "reference")
    assert base == digest(keys.copy(), "reference")
    moved = keys.copy()
    moved[3, 2] += 1e-9
    assert len({base, digest(moved, "reference"), digest(keys, "network"), digest(keys[:5], "reference"), digest(keys, "reference", False)}) == 5


def test_cached_model_keeps_the_map_probe(tmp_path, monkeypatch):
    from sspslam_amd import modelcache
    monkeypatch.setenv("SSN_CACHE_DIR", str(tmp_path))
    net, o = rc.memory_network(*rc.SHAPES[0])
    first = modelcache.cached_build(net, cache=True)
    again = modelcache.cached_build(net, cache=True)
    assert first.stats["cache"].startswith("miss") and again.stats["cache"] == "hit"
    assert [p["probe"] for p in again.map_probes] == [p["probe"] for p in first.map_probes]
    for a, b in zip(first.map_probes, again.map_probes):
        np.testing.assert_array_equal(a["recall"]["keys"], b["recall"]["keys"])
        np.testing.assert_array_equal(a["recall"]["scale"], b["recall"]["scale"])
        assert a["recall"]["mode"] == b["recall"]["mode"] and a["every"] == b["every"]


# -- the C ABI without a device -------------------------------------------------------------------------------------------------------
def test_abi_fails_loudly_without_a_device():
    from sspslam_amd import _lib
    lib = _lib.load()
    out = np.zeros(8)
    info = _lib.RecallInfo()
    assert lib.ssn_recall_run(None, out.ctypes.data) == -1 and b"null handle" in lib.ssn_last_error()
    assert lib.ssn_recall_set_keys(None, out.ctypes.data, 1) == -1
    assert lib.ssn_recall_get_info(None, C.byref(info)) == -1
    lib.ssn_recall_destroy(None)
    h = C.c_void_p()
    scale, bias, keys = np.ones(100), np.zeros(100), np.zeros((2, 7))
    call = lambda n_keys, handle: lib.ssn_recall_create(None, 0, 1, 100, 7, 5, scale.ctypes.data, bias.ctypes.data, 0, 0.02, 0.002, 1.0,      # noqa: E731
                                                        keys.ctypes.data, n_keys, 0, handle)
    assert call(2, None) == -1 and b"null handle" in lib.ssn_last_error()
    assert call(0, C.byref(h)) == -1 and b"key rows" in lib.ssn_last_error()
    if lib.ssn_device_count() == 0:
        assert call(2, C.byref(h)) == -2 and b"no HIP device available (there is no CPU fallback)" in lib.ssn_last_error()
    else:
        assert call(2, C.byref(h)) == -1 and b"null simulator" in lib.ssn_last_error()
    assert not h.value
    assert C.sizeof(_lib.RecallInfo) == 12 * 8 + 8


# -- harness.map_over_time ------------------------------------------------------------------------------------------------------------
def test_map_over_time_is_the_per_sample_host_decode():
    from sspslam_amd import frontend as nengo
    from sspslam_amd import harness as H
    from sspslam_amd.sspspace import SPSpace
    space = H.make_ssp_space(2, ssp_dim=13)
    d, n, L = space.ssp_dim, 60, 4
    rng = np.random.RandomState(4)
    lm_space = SPSpace(L, d, seed=1)
    locs = rng.uniform(-0.8, 0.8, (L, 2))
    gain, bias = rc.lif_gain_bias(rng.uniform(200, 400, n), np.full(n, 0.1))
    built = type("B", (), dict(gain=gain, bias=bias))()
    frames, want = [], []
    for s in range(3):
        E = rc.unit_rows(rng, n, d) * gain[:, None]
        E[:L] = np.asarray(lm_space.vectors) * gain[:L, None]
        W = 1e-3 * rng.standard_normal((d, n)) * 0.01
        W[:, :L] += 1e-3 * space.encode(locs + 0.05 * s).T
        recalled, est = H.map_recall_learned(space, lm_space, built, nengo.LIF(), E, W, num_samples=40)
        frames.append(recalled)
        want.append(est)
    got = H.map_over_time(space, np.array(frames), num_samples=40)
    assert got.shape == (3, L, 2)
    np.testing.assert_array_equal(got, np.array(want))
    assert H.map_over_time(space, np.zeros((0, L, d))).shape == (0, L, 2)
    with pytest.raises(ValueError):
        H.map_over_time(space, np.zeros((L, d)))
