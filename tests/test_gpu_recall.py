"""Map recall on the GPU (csrc/ssn_recall.hip behind MapProbe and Simulator.recall), held to the instrument of
tests/recall_checks.py: every sample of a MapProbe within B of the float64 recall computed from the samples of the two buffer probes of
the same run - which also proves that a map sample is taken where a buffer-probe sample is.

Worst err / B measured on the MI355X (printed by every test): DESIGN.md 3.13."""
import os
import subprocess
import sys

import numpy as np
import pytest

import recall_checks as rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("reference", "network")


@pytest.fixture(scope="module")
def Simulator():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from sspslam_amd.simulator import Simulator
    return Simulator


_built = {}


def built(shape, neuron="lif", voja=True):
    """(model, objects) of the memory network of a shape, built once per module."""
    key = (shape, neuron, voja)
    if key not in _built:
        from sspslam_amd import frontend as nengo
        from sspslam_amd.builder import build
        nt = {"lif": None, "lifrate": nengo.LIFRate(), "relu": nengo.RectifiedLinear()}[neuron]
        net, o = rc.memory_network(*shape, neuron_type=nt, voja=voja)
        _built[key] = (build(net), o)
    return _built[key]


def matrices(sim, model, o, i=None):
    """(E, W, built ensemble): sample i of the two buffer probes, or (i is None) the state read back now."""
    mem = o["memory"]
    be, bc = model.params[mem.memory], model.params[mem.conn_out]
    if i is None:
        return sim.read_buffer(be.encoder_buffer), sim.read_buffer(bc.learned_buffer), be
    E = sim.data[o["e_probe"]][i] if o["e_probe"] is not None else be.scaled_encoders
    return E, sim.data[o["w_probe"]][i], be


def check_samples(sim, model, o, u, label):
    n_samples = rc.STEPS // rc.EVERY
    worst = 0.0
    for mode in MODES:
        frames = sim.data[o["map_probes"][mode]]
        assert frames.shape == (n_samples, rc.N_KEYS, model.params[o["memory"].conn_out].weights.shape[0]) and frames.dtype == np.float64
        assert not frames.flags.writeable
        for i in range(n_samples):
            E, W, be = matrices(sim, model, o, i)
            worst = max(worst, rc.check(frames[i], o["keys"], E, W, be.gain, be.bias, be.neuron, mode, u, f"{label} sample {i}"))
    np.testing.assert_allclose(sim.trange(sample_every=rc.EVERY * sim.dt), sim.dt * rc.EVERY * np.arange(1, n_samples + 1))
    return worst


@pytest.mark.parametrize("shape", rc.SHAPES)
def test_f64_samples_match_the_buffer_probes(Simulator, shape):
    model, o = built(shape)
    with Simulator(None, model=model, dtype="f64") as sim:
        sim.run_steps(rc.STEPS)
        check_samples(sim, model, o, rc.U64, f"f64 {shape}")


@pytest.mark.parametrize("plan", ["default", "no_spmv"])
@pytest.mark.parametrize("shape", rc.SHAPES)
def test_f32_samples_match_the_buffer_probes_in_both_layouts(Simulator, shape, plan):
    from sspslam_amd.simulator import SSN_PLAN_NO_SPMV
    model, o = built(shape)
    with Simulator(None, model=model, dtype="f32", flags=SSN_PLAN_NO_SPMV if plan == "no_spmv" else 0) as sim:
        sim.run_steps(rc.STEPS)
        check_samples(sim, model, o, rc.U32, f"f32 {plan} {shape}")
        info = sim.recall_info(o["map_probes"]["reference"])
        # the plan keeps the decoders of a LIF population of 128 neurons or more neuron-major unless SSN_PLAN_NO_SPMV forbids it
        assert info["dec_neuron_major"] == int(plan == "default" and shape[0] >= 128), info
        assert (info["n"], info["d_key"], info["d_val"], info["n_keys"]) == shape + (rc.N_KEYS,) and info["last_launches"] >= 3
        assert sim.recall_seconds > 0 and sim.recall_kernel_ms > 0


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("shape", rc.SHAPES)
def test_recall_on_demand_for_any_number_of_keys(Simulator, shape, dtype):
    model, o = built(shape)
    mem = o["memory"]
    with Simulator(None, model=model, dtype=dtype) as sim:
        sim.run_steps(rc.STEPS)
        E, W, be = matrices(sim, model, o)
        for L in (1, 10, 33, 65, 130):
            keys = rc.recall_keys(o["keys"], L)
            for mode in MODES:
                q = sim.recall(mem, keys, mode=mode)
                rc.check(q, keys, E, W, be.gain, be.bias, be.neuron, mode, rc.U32 if dtype == "f32" else rc.U64, f"recall {dtype} {shape} L = {L}")
        # the pair form names the same memory; a later run is seen by the next call
        keys = rc.recall_keys(o["keys"], 10)
        np.testing.assert_array_equal(sim.recall((mem.conn_in, mem.conn_out), keys), sim.recall(mem, keys))
        np.testing.assert_array_equal(sim.recall((mem.memory, mem.conn_out), keys), sim.recall(mem, keys))
        before = sim.recall(mem, keys)
        sim.run_steps(20)
        E, W, be = matrices(sim, model, o)
        after = sim.recall(mem, keys)
        assert not np.array_equal(before, after)
        rc.check(after, keys, E, W, be.gain, be.bias, be.neuron, "reference", rc.U32 if dtype == "f32" else rc.U64, f"recall {dtype} {shape} after 20 more steps")


@pytest.mark.parametrize("plan", ["default", "no_spmv"])
def test_same_bits_for_two_scratch_sizes_and_two_calls(Simulator, plan):
    from sspslam_amd.simulator import SSN_PLAN_NO_SPMV
    shape = rc.SHAPES[2]
    model, o = built(shape)
    mem = o["memory"]
    with Simulator(None, model=model, dtype="f32", flags=SSN_PLAN_NO_SPMV if plan == "no_spmv" else 0) as sim:
        sim.run_steps(rc.STEPS)
        for L in (10, 65):
            keys = rc.recall_keys(o["keys"], L)
            full = sim.recall(mem, keys)
            info = sim.recall_info(mem)
            assert info["n_chunks"] == 5 and info["chunks_per_pass"] == 5, info
            for scratch in (info["min_scratch_bytes"], 2 * info["min_scratch_bytes"]):
                small = sim.recall(mem, keys, scratch_bytes=scratch)
                assert sim.recall_info(mem, scratch_bytes=scratch)["chunks_per_pass"] == scratch // info["min_scratch_bytes"]
                assert small.tobytes() == full.tobytes(), (L, scratch)
            assert sim.recall(mem, keys).tobytes() == full.tobytes()
        from sspslam_amd.frontend import SimulationError
        with pytest.raises(SimulationError, match="scratch"):
            sim.recall(mem, keys, scratch_bytes=1024)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("neuron", ["lifrate", "relu"])
def test_rate_populations(Simulator, neuron, dtype):
    shape = rc.SHAPES[1]
    model, o = built(shape, neuron=neuron)
    assert model.params[o["memory"].memory].neuron["type"] == neuron
    with Simulator(None, model=model, dtype=dtype) as sim:
        sim.run_steps(rc.STEPS)
        check_samples(sim, model, o, rc.U32 if dtype == "f32" else rc.U64, f"{neuron} {dtype} {shape}")


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_voja_off_uses_the_built_encoders(Simulator, dtype):
    shape = rc.SHAPES[0]
    model, o = built(shape, voja=False)
    with Simulator(None, model=model, dtype=dtype) as sim:
        sim.run_steps(rc.STEPS)
        check_samples(sim, model, o, rc.U32 if dtype == "f32" else rc.U64, f"voja off {dtype} {shape}")


def test_pipelined_run_gives_the_same_samples(Simulator):
    """A run longer than 2 PIPELINE_CHUNK is cut into chunks whose inputs are tabulated beside the device; the map samples cut it
    further, as buffer probes do.  Same samples as the same run in one prepared piece."""
    shape = rc.SHAPES[0]
    model, o = built(shape)
    mp = o["map_probes"]["reference"]
    with Simulator(None, model=model, dtype="f32") as sim:
        steps = 2 * sim.PIPELINE_CHUNK + 150
        sim.run_steps(steps)
        piped = np.array(sim.data[mp])
        w_piped = np.array(sim.data[o["w_probe"]])
    with Simulator(None, model=model, dtype="f32") as sim:
        sim.prepare(steps)
        sim.run_steps(steps)
        whole = np.array(sim.data[mp])
        np.testing.assert_array_equal(np.array(sim.data[o["w_probe"]]), w_piped)
    assert piped.shape == (steps // rc.EVERY, rc.N_KEYS, shape[2])
    np.testing.assert_array_equal(piped, whole)


def test_reset_drops_the_samples(Simulator):
    shape = rc.SHAPES[0]
    model, o = built(shape)
    mp = o["map_probes"]["network"]
    with Simulator(None, model=model, dtype="f32") as sim:
        sim.run_steps(rc.STEPS)
        first = np.array(sim.data[mp])
        assert first.shape[0] == rc.STEPS // rc.EVERY
        sim.reset()
        assert sim.data[mp].shape == (0, rc.N_KEYS, shape[2])
        sim.run_steps(rc.STEPS)
        np.testing.assert_array_equal(np.array(sim.data[mp]), first)


def test_abi_refuses_wrong_shapes_and_null_handles(Simulator):
    import ctypes as C
    from sspslam_amd import _lib
    from sspslam_amd.builder import recall_spec
    from sspslam_amd.frontend import SimulationError
    from sspslam_amd.simulator import DeviceRecall
    shape = rc.SHAPES[0]
    model, o = built(shape)
    lib = _lib.load()
    out = np.zeros(4)
    assert lib.ssn_recall_run(None, out.ctypes.data) == -1 and lib.ssn_recall_set_keys(None, out.ctypes.data, 1) == -1
    assert lib.ssn_recall_get_info(None, C.byref(_lib.RecallInfo())) == -1
    with Simulator(None, model=model, dtype="f32") as sim:
        spec = recall_spec(model, o["memory"], o["keys"])
        for wrong in (dict(n=spec["n"] + 1), dict(d_key=spec["d_key"] + 1), dict(d_val=spec["d_val"] + 1), dict(enc=spec["dec"]), dict(dec=spec["enc"]),
                      dict(keys=np.zeros((0, spec["d_key"])))):
            with pytest.raises(SimulationError, match="SSN_EINVAL"):
                DeviceRecall(sim, dict(spec, **wrong))
        h = C.c_void_p()
        rcode = lib.ssn_recall_create(None, spec["enc"], spec["dec"], spec["n"], spec["d_key"], spec["d_val"], spec["scale"].ctypes.data, spec["bias"].ctypes.data,
                                      0, 0.02, 0.002, 1.0, spec["keys"].ctypes.data, spec["keys"].shape[0], 0, C.byref(h))
        assert rcode == -1 and b"null simulator" in lib.ssn_last_error()


def test_run_slam_example_writes_the_map_over_time(tmp_path):
    """examples/run_slam.py --map-every: a MapProbe on the landmark SPs, decoded on the GPU, saved next to the reference's fields."""
    cmd = [sys.executable, os.path.join(ROOT, "examples", "run_slam.py"), "--map-every", "0.05", "--T", "0.3", "--decode-backend", "hip", "--save",
           "--save-dir", str(tmp_path), "--ssp-dim", "55", "--pi-n-neurons", "100", "--mem-n-neurons", "300", "--limit", "4.0"]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    print(done.stdout[-3000:], done.stderr[-3000:])
    assert done.returncode == 0
    assert "map recall" in done.stdout
    files = [f for f in os.listdir(tmp_path) if f.endswith(".npz")]
    assert len(files) == 1, files
    data = np.load(os.path.join(tmp_path, files[0]), allow_pickle=False)
    n_lm = data["obj_locs"].shape[0]
    assert data["landmark_loc_over_time"].shape == (6, n_lm, 2) and data["landmark_loc_over_time_ts"].shape == (6,)
    np.testing.assert_allclose(data["landmark_loc_over_time_ts"], 0.05 * np.arange(1, 7))
    assert data["landmark_loc_est"].shape == (n_lm, 2) and data["landmark_ssps_est"].shape == (n_lm, 55)
