#!/usr/bin/env python3
"""Capture the fixtures of tests/test_reference_dropin.py from a checkout of the reference (sspslam).

The reference's OWN network classes are loaded file by file with this repo's object model registered as
``import nengo`` (``frontend.install_as_nengo``), built by our builder and stepped by the NumPy oracle; what
they produce - built-model census, buffers, probe trajectories - is written to ``reference_dropin.npz``, with
the inputs the reference's objects fed them (phase matrix, vocabulary, object-vector-cell encoders, the input
functions tabulated per timestep).  The recorded trajectory the reference ships (``example_paths/
twoRooms_path.npy``, the rows ``--path-data`` reads) goes to ``recorded_path.npz``.  Nothing from the
reference's source is copied: the fixtures hold inputs and outputs only.

    python tests/golden/make_dropin_golden.py PATH_TO_REFERENCE_CHECKOUT
"""
import hashlib
import importlib.util
import os
import sys
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DT = 0.001
D = 55
PI_STEPS = 150
SLAM_STEPS = 120
PATH_ROWS = 49999          # harness.load_path's default cut (run_pathint.py --path-data)


def load_reference(ref):
    import sspslam_amd.frontend as fe
    fe.install_as_nengo(force=True)

    def load(modname, relpath):
        spec = importlib.util.spec_from_file_location(modname, os.path.join(ref, relpath))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[modname] = mod
        spec.loader.exec_module(mod)
        return mod
    # register the packages by hand: sspslam/utils/__init__.py wants LaTeX fonts and nengo_loihi
    for pkg in ("sspslam", "sspslam.utils", "sspslam.networks"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    utils = load("sspslam.utils.utils", "sspslam/utils/utils.py")
    sys.modules["sspslam.utils"].sparsity_to_x_intercept = utils.sparsity_to_x_intercept
    sys.modules["sspslam.utils"].Rd_sampling = utils.Rd_sampling
    out = types.SimpleNamespace(utils=utils)
    out.ssp = load("sspslam.sspspace", "sspslam/sspspace.py")
    out.pi = load("sspslam.networks.pathintegration", "sspslam/networks/pathintegration.py")
    out.bind = load("sspslam.networks.binding", "sspslam/networks/binding.py")
    out.am = load("sspslam.networks.associativememory", "sspslam/networks/associativememory.py")
    nets = sys.modules["sspslam.networks"]
    nets.PathIntegration, nets.CircularConvolution = out.pi.PathIntegration, out.bind.CircularConvolution
    nets.Product, nets.AssociativeMemory = out.bind.Product, out.am.AssociativeMemory
    out.slam = load("sspslam.networks.slam", "sspslam/networks/slam.py")
    import nengo
    out.nengo = nengo
    return out


def pathint(ref, g):
    """run_pathint.py:128-143 with the reference's PathIntegration class, d = 55, 60 neurons per VCO."""
    from sspslam_amd import harness as H
    from sspslam_amd.builder import build
    from oracle import OracleSimulator
    nengo = ref.nengo
    space_ref = ref.ssp.HexagonalSSPSpace(2, ssp_dim=D, domain_bounds=np.tile([-1.0, 1.0], (2, 1)), length_scale=0.2)
    path, vels = H.make_random_path(10.0, limit=0.2, seed=0)
    real_ssp = space_ref.encode(path)
    scale_fac = 1.0 / np.max(np.abs(space_ref.phase_matrix @ vels.T))
    vs = vels * scale_fac
    model = nengo.Network(seed=0)
    with model:
        vel_input = nengo.Node(lambda t: vs[int((t - DT) / DT)], label="vel_input")
        init_state = nengo.Node(lambda t: real_ssp[int((t - DT) / DT)] if t < 0.05 else np.zeros(space_ref.ssp_dim))
        pint = ref.pi.PathIntegration(space_ref, 60, 0.05, scaling_factor=scale_fac, stable=True, solver_weights=False)
        nengo.Connection(vel_input, pint.velocity_input, synapse=None)
        nengo.Connection(init_state, pint.input, synapse=None)
        nengo.Probe(pint.output, synapse=0.05)
    bm = build(model)
    sim = OracleSimulator(bm)
    sim.run_steps(PI_STEPS)
    g["phase_matrix"] = np.asarray(space_ref.phase_matrix, dtype=float)
    g["pi_n_ops"] = np.array(bm.stats["n_ops"])
    g["pi_n_neurons"] = np.array(bm.stats["n_neurons"])
    g["pi_probe"] = sim.probe_data(0)


def slam(ref, g):
    """run_slam.py:155-195 with the reference's SLAMNetwork (and its CircularConvolution, Product, AssociativeMemory,
    PathIntegration) and the reference's input functions on the reference's SSP space, d = 55, 5 landmarks."""
    from sspslam_amd import harness as H
    from sspslam_amd.builder import build
    from oracle import OracleSimulator
    nengo = ref.nengo
    space_ref = ref.ssp.HexagonalSSPSpace(2, ssp_dim=D, domain_bounds=np.tile([-1.0, 1.0], (2, 1)), length_scale=0.2)
    path, vels = H.make_random_path(10.0, limit=0.2, seed=0)
    obj_locs = 0.9 * 2 * (ref.utils.Rd_sampling(5, 2, seed=0) - 0.5)
    vec_to_lm = obj_locs[None, :, :] - path[:, None, :]
    lm_space = ref.ssp.SPSpace(5, D, seed=0)
    real_ssp = space_ref.encode(path)
    vf, scale, inview, idf, spf, vecf, vecsspf = ref.slam.get_slam_input_functions2(space_ref, lm_space, vels, vec_to_lm, 0.6)
    # the network classes get OUR space objects on the reference's phase matrix and vocabulary - the ones the test
    # rebuilds - so that both classes see the same clean-up grid bit for bit (its argmax amplifies a 1e-16 difference;
    # the matrix in C order, as the fixture stores it: the encoding's product rounds differently on a Fortran-order one)
    from sspslam_amd.sspspace import SPSpace, SSPSpace
    space = SSPSpace(2, D, np.ascontiguousarray(space_ref.phase_matrix), domain_bounds=np.tile([-1.0, 1.0], (2, 1)), length_scale=0.2)
    lm_own = SPSpace(5, D, vectors=lm_space.vectors)
    init_f = (lambda t: real_ssp[int((t - DT) / DT)] if t < 0.05 else np.zeros(D))
    model = nengo.Network(seed=0)
    with model:
        vel_input = nengo.Node(vf, label="vel_input")
        init_state = nengo.Node(init_f, label="init_state")
        landmark_vec = nengo.Node(vecsspf, label="lm_vec")
        landmark_id = nengo.Node(spf, label="lm_id")
        is_landmark = nengo.Node(inview, label="lm_in_view")
        sl = ref.slam.SLAMNetwork(space, lm_own, 0.6, 5, 30, 60, 20, tau_pi=0.05, update_thres=0.2, vel_scaling_factor=scale,
                                  shift_rate=0.2, voja_learning_rate=1e-4, pes_learning_rate=5e-3, clean_up_method="grid",
                                  gc_n_neurons=0, encoders=None, voja=True, seed=0, intercept=0.1)
        nengo.Connection(vel_input, sl.velocity_input, synapse=None)
        nengo.Connection(init_state, sl.pathintegrator.input, synapse=None)
        nengo.Connection(landmark_vec, sl.landmark_vec_ssp, synapse=None)
        nengo.Connection(landmark_id, sl.landmark_id_input, synapse=None)
        nengo.Connection(is_landmark, sl.no_landmark_in_view, synapse=None)
        nengo.Probe(sl.pathintegrator.output, synapse=0.05)
    # the two Python function nodes with inputs of the reference's class carry no `native` hint (ZERO edits to it)
    assert sl.gridcells.native is None and sl.update_state.native is None
    bm = build(model)
    sim = OracleSimulator(bm)
    sim.run_steps(SLAM_STEPS)
    # the inputs, one row per timestep k = 0 .. SLAM_STEPS + 8 at t = k dt (the node functions read at those times)
    ts = np.arange(SLAM_STEPS + 9) * DT
    for name, f in (("vel", vf), ("init", init_f), ("lm_vec", vecsspf), ("lm_id", spf), ("in_view", inview)):
        g["slam_in_" + name] = np.stack([np.atleast_1d(np.asarray(f(t), dtype=float)) for t in ts])
    g["slam_vel_scale"] = np.array(float(scale))
    g["slam_lm_vectors"] = np.asarray(lm_space.vectors, dtype=float)
    # drawn from the global, unseeded NumPy generator by the reference (slam.py:206): the fixture pins one draw
    g["slam_ovc_encoders"] = np.asarray(sl.ovc_ens.encoders, dtype=float)
    g["slam_n_connections"] = np.array(len(model.all_connections))
    g["slam_n_ensembles"] = np.array(len(model.all_ensembles))
    g["slam_op_kinds"] = np.array([o["kind"] for o in bm.ops])
    gate = next(o for o in bm.ops if o["kind"] == "gate")
    g["slam_gate"] = np.array([gate["d"], gate["thres"], gate["rate"]], dtype=float)
    cl = next(o for o in bm.ops if o["kind"] == "cleanup")
    # the clean-up table (10^4 grid rows x d) is compared bit for bit: its digest stands for it
    w = np.ascontiguousarray(bm.buffers[cl["w"]], dtype=np.float64)
    g["slam_cleanup_w_index"] = np.array(cl["w"])
    g["slam_cleanup_w_shape"] = np.array(w.shape)
    g["slam_cleanup_w_sha256"] = np.array(hashlib.sha256(w.tobytes()).hexdigest())
    g["slam_n_buffers"] = np.array(len(bm.buffers))
    for i, b in enumerate(bm.buffers):
        if i != cl["w"]:
            g[f"slam_buffer_{i}"] = np.asarray(b)
    g["slam_probe"] = sim.probe_data(0)


def main(ref):
    g = {}
    pathint(load_reference(ref), g)
    slam(load_reference(ref), g)
    np.savez_compressed(os.path.join(OUT, "reference_dropin.npz"), **g)
    raw = np.load(os.path.join(ref, "example_paths", "twoRooms_path.npy"))
    np.savez_compressed(os.path.join(OUT, "recorded_path.npz"), twoRooms_path=raw[:PATH_ROWS])
    for fn in ("reference_dropin.npz", "recorded_path.npz"):
        print(f"  {fn:28s} {os.path.getsize(os.path.join(OUT, fn)) / 1024:8.1f} KiB")


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "sspslam")):
        sys.exit(__doc__)
    main(sys.argv[1])
