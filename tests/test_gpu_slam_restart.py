"""The f32 SLAM step against ONE float64 step from the device's own state, every operator (tests/slam_restart.py derives the bounds and
the decision rules; tests/test_slam_restart.py proves the instrument on the CPU).  Between the restart points the device advances with
one ordinary ``run_steps`` call per gap (the step graphs); a restart step is a launch of one timestep.  The time-batched stages run
in blocks of 64 timesteps counted from the start of each ``run_steps`` call: a restart point 65 after the one before it follows a
call of exactly 64 timesteps, so it reads the carry row that a whole block left; the other points follow ragged blocks.

Every case asserts which plan ran: kernel names of a profiled run, counters, and for what is a body of k_round the planner's own
listing (SSN_DEBUG_PLAN, read from stderr).  The figures are printed before they are asserted (run with -s)."""
import re
import contextlib
import os
import time

import numpy as np
import pytest

import sspslam_amd.frontend as nengo
from sspslam_amd import harness as H
from sspslam_amd import simulator as PLAN
from sspslam_amd.builder import build

import slam_restart as R

pytestmark = pytest.mark.gpu

BLOCK = 64
OLD = PLAN.SSN_PLAN_NO_ROUNDS | PLAN.SSN_PLAN_NO_ITEM_BATCH


@pytest.fixture(scope="module")
def Simulator():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from sspslam_amd.simulator import Simulator
    return Simulator


@pytest.fixture(scope="module")
def small():
    return R.small_slam()


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


# positions in ``enum RoundKind`` (csrc/ssn_launch.hpp) and ``enum MicroKind``, as the plan listing prints them
RK_PES, RK_VOJA, RK_GRID_LHS, RK_GRID_DOT, M_LOWPASS = 8, 9, 14, 15, 4


def plan_listing(err):
    """The single-timestep round plan of an SSN_DEBUG_PLAN listing -> ({body kind: {(gx, gy)}}, [(micro kind, len, dst, src)])."""
    bodies, micros = {}, []
    for line in err.splitlines():
        if line.startswith("[ssn]   round"):
            for k, gx, gy in re.findall(r" (\d+)\[(\d+)x(\d+)\]", line):
                bodies.setdefault(int(k), set()).add((int(gx), int(gy)))
        m = re.match(r"\[ssn\]\s+micro (\d+)/(\d+) dst (-?\d+) src (-?\d+)", line)
        if m:
            micros.append(tuple(int(g) for g in m.groups()))
    return bodies, micros


def planned(Simulator, capfd, model, flags=0, env=None):
    """A simulator built under SSN_DEBUG_PLAN -> (sim, bodies, micros).  The environment is set around ``Simulator(...)`` only."""
    out = capfd.readouterr()
    print(out.out, end="")
    with environment(SSN_DEBUG_PLAN="1", **(env or {})):
        sim = Simulator(None, model=model, dtype="f32", flags=flags, block_steps=BLOCK)
    bodies, micros = plan_listing(capfd.readouterr().err)
    return sim, bodies, micros


def restart_run(sim, model, points, steps, label, profile_steps=32):
    """-> (summary, counters, kernel names); closes ``sim``."""
    t0 = time.time()
    with sim:
        s = R.run_points(model, sim, points)
        if steps > sim.n_steps:
            sim.run_steps(steps - sim.n_steps)
        c = sim.counters()
        assert c["n_steps"] == steps
        sim.run_steps(profile_steps, profile=2)
        names = set(sim.kernel_times())
    print(R.describe(s, label))
    print("%s kernels %s launches per step %d wall %.1f s" % (label, sorted(names), c["launches_per_step"], time.time() - t0))
    return s, c, names


def simulator(Simulator, model, flags=0, env=None):
    with environment(**(env or {})):
        return Simulator(None, model=model, dtype="f32", flags=flags, block_steps=BLOCK)


def assert_passes(s, kinds, learning=True, gate_open=False):
    assert not s["failures"], R.describe(s)
    assert s["worst"] <= 1.0, R.describe(s)
    assert s["skipped"] <= 1 and s["ok"], R.describe(s)
    assert set(kinds) <= set(s["kind"]), (kinds, sorted(s["kind"]))
    if learning:
        assert s["live"]["pes"] > 0 and s["live"]["pes_inc"] > 0 and s["live"]["voja"] > 0 and s["live"]["voja_rows"] > 0, s["live"]
    if gate_open:
        assert 0 < s["live"]["gate_open"], s["live"]


SLAM_KINDS = ("lowpass", "neurons", "ensarray", "pes", "voja", "gate", "cleanup")
# 129 and 194 follow a call of exactly 64 timesteps (one whole block), the others ragged blocks; the gate is closed up to 194, open from 200
SMALL_POINTS = (60, 64, 129, 194, 200, 250, 320, 399)


@pytest.mark.parametrize("flags,name", [(0, "default"), (OLD, "one launch per operator"), (PLAN.SSN_PLAN_NO_FFT, "dense transforms")])
def test_small_slam_on_three_plans(Simulator, small, flags, name):
    """d = 55, 15 200 neurons, 400 steps: the round plan (k_round), the round-1 plan - k_pes, k_voja, k_matvec, k_neurons and
    k_spmv_partial as launches of their own -, and the dense transform matrices instead of the FFT."""
    model = small[1]
    assert {o["kind"] for o in model.ops} >= {"cleanup", "gate", "pes", "voja", "neurons", "ensarray", "matvec", "lowpass", "lincomb"}
    s, c, names = restart_run(simulator(Simulator, model, flags), model, SMALL_POINTS, 400, "small SLAM, %s" % name)
    n_dft = sum(1 for o in model.ops if o["kind"] == "matvec" and o.get("dft"))
    if flags == OLD:
        assert {"k_pes", "k_voja", "k_matvec", "k_neurons", "k_spmv_partial"} <= names and "k_round" not in names, sorted(names)
    else:
        assert "k_round" in names, sorted(names)
    assert c["fft_transforms"] == (0 if flags == PLAN.SSN_PLAN_NO_FFT else n_dft), c
    assert_passes(s, SLAM_KINDS, gate_open=True)


def test_small_slam_factored_cleanup_in_the_round_grid(Simulator, small, capfd):
    """SSN_GRID_DOT_MIN_MB=0: the 10^4 x 55 table goes through its factor tables as bodies of the round grid (RK_GRID_LHS, RK_GRID_DOT),
    nn = 100 (six 16-row blocks and 4 rows), k2 = 56.  The route is a body of k_round, so it has no kernel name of its own: the
    planner's listing must hold both bodies, and must not hold them in the default plan."""
    model = small[1]
    cl = [o for o in model.ops if o["kind"] == "cleanup"][0]
    assert (cl["grid_rows"], cl["grid_cols"], cl["grid_k2"]) == (100, 100, 56) and cl["rows"] < 65536 and cl["grid_k2"] * 4 <= 48 * 1024 and "g_dft" in cl
    sim, bodies, _ = planned(Simulator, capfd, model)
    with sim:
        default = sim.counters()
    assert bodies and RK_GRID_LHS not in bodies and RK_GRID_DOT not in bodies, bodies
    sim, bodies, _ = planned(Simulator, capfd, model, env={"SSN_GRID_DOT_MIN_MB": "0"})
    assert RK_GRID_LHS in bodies and RK_GRID_DOT in bodies, bodies
    assert os.environ.get("SSN_GRID_DOT_MIN_MB") is None
    s, c, names = restart_run(sim, model, SMALL_POINTS, 400, "small SLAM, factored clean-up")
    assert "k_round" in names and c["device_bytes"] > default["device_bytes"], (c, default)
    assert_passes(s, SLAM_KINDS, gate_open=True)
    assert "sig %d:%d cleanup" % (cl["dst"], cl["dst"] + cl["cols"]) in s["region"], sorted(s["region"])


def test_slam_at_ssp_dim_1015(Simulator, capfd):
    """The benchmark's operator shapes (the model of test_slam_at_ssp_dim_1015_matches_oracle): the factored clean-up by default,
    FFTs with a radix-29 pass inside the round grid, PES and Voja on 1015 columns and 1200 rows (37 blocks of 32 and 16), the folded
    activity filter.  Memory spikes are rare at this size (one or two rows of the Voja matrix in a step): the points are steps at
    which the float64 oracle's run has some; 119 follows a call of exactly 64 timesteps."""
    space = H.make_ssp_space(2, 1015)
    path, vels = H.make_random_path(20.0, limit=0.1, seed=0)
    sm = R.with_decision_probes(H.make_slam_model(space, path, vels, n_landmarks=10, pi_n_neurons=100, mem_n_neurons=1200,
                                                  circonv_n_neurons=20, view_rad=0.6, weights_sample_every=None))
    model = build(sm.model)
    assert sorted(o["dft"] for o in model.ops if o["kind"] == "matvec" and o.get("dft")) == [1, 2, 2, 3, 5, 5]
    pes = [o for o in model.ops if o["kind"] == "pes"][0]
    voja = [o for o in model.ops if o["kind"] == "voja"][0]
    assert (pes["rows"], pes["cols"], voja["rows"], voja["cols"]) == (1015, 1200, 1200, 1015)
    cl = [o for o in model.ops if o["kind"] == "cleanup"][0]
    # the planner's conditions for the factored route in the round grid, and its listing
    assert cl["rows"] * cl["cols"] * 4 >= 16 << 20 and "g_dft" in cl and cl["rows"] < 65536 and cl["grid_k2"] * 4 <= 48 * 1024
    sim, bodies, micros = planned(Simulator, capfd, model)
    assert RK_GRID_LHS in bodies and RK_GRID_DOT in bodies, bodies
    assert bodies[RK_PES] == {(1, (1200 + 31) // 32)} and RK_VOJA in bodies, bodies        # neuron-major: 1015 columns, 1200 rows
    assert not [m for m in micros if m[0] == M_LOWPASS and m[2] < pes["act"] + pes["cols"] and pes["act"] < m[2] + m[1]], "the activity filter is folded"
    s, c, names = restart_run(sim, model, (42, 45, 49, 52, 54, 119), 120, "SLAM d = 1015")
    assert "k_round" in names and c["fft_transforms"] == 6 and c["fft_bluestein"] == 0, (sorted(names), c)
    assert_passes(s, SLAM_KINDS)


@pytest.mark.parametrize("flags,split", [(0, None), (0, "2"), (OLD, None)])
def test_slam_3d_grid_product(Simulator, flags, split):
    """The 3-D model of test_slam_3d_matches_oracle (d = 33, 10^6-row grid): the left operand (a body of the round grid by default,
    k_grid_lhs as a launch of its own in the round-1 plan), k_gemm_nt_mfma_f32 (with K-split partials under SSN_GRID_SPLIT=2) and
    k_argmax_partial.  The clean-up returns the float64 row on every step that is not marginal.  (60 steps: no whole block.)"""
    space = H.make_ssp_space(3, ssp_dim=33, rng=np.random.default_rng(3))
    path, vels = H.make_random_path(10.0, limit=0.5, seed=2, domain_dim=3)
    sm = R.with_decision_probes(H.make_slam_model(space, path, vels, n_landmarks=20, pi_n_neurons=100, mem_n_neurons=200,
                                                  circonv_n_neurons=50, view_rad=0.6, weights_sample_every=None))
    model = build(sm.model)
    cl = [o for o in model.ops if o["kind"] == "cleanup"][0]
    assert (cl["rows"], cl["grid_rows"], cl["grid_cols"], cl["grid_k2"]) == (100 ** 3, 100, 100 ** 2, 34)
    s, c, names = restart_run(simulator(Simulator, model, flags, {"SSN_GRID_SPLIT": split}), model, (20, 33, 47, 59), 60,
                              "SLAM 3-D, flags %d split %s" % (flags, split))
    if split:       # the split was in force: a second vector of 10^6 partial similarities (the default plan has one part at k2 = 34),
        with simulator(Simulator, model, flags) as sim:      # and a little more for the partials of the argmax stage
            more = c["device_bytes"] - sim.counters()["device_bytes"]
        assert cl["rows"] * 4 <= more < cl["rows"] * 4 + (64 << 10), more
    assert {"k_gemm_nt_mfma_f32", "k_argmax_partial", "k_grid_lhs" if flags == OLD else "k_round"} <= names, sorted(names)
    assert_passes(s, ("cleanup", "lowpass", "neurons", "ensarray"), learning=False)
    assert "sig %d:%d cleanup" % (cl["dst"], cl["dst"] + cl["cols"]) in s["region"], sorted(s["region"])


def learning_network(n=1100, d=12, d_out=5):
    """A Voja + PES memory population driven by nodes: learning is live at every step.  n is just over one 1024-column tile of the
    PES kernel and no multiple of the Voja kernel's rows per wave or per workgroup."""
    rng = np.random.RandomState(5)
    wk, pk = rng.uniform(3.0, 9.0, size=d), rng.uniform(0, 6.28, size=d)
    we, pe = rng.uniform(2.0, 7.0, size=d_out), rng.uniform(0, 6.28, size=d_out)
    with nengo.Network(seed=5) as net:
        key = nengo.Node(lambda t: 0.5 * np.sin(wk * t + pk))
        err_src = nengo.Node(lambda t: 0.4 * np.cos(we * t + pe))
        mem = nengo.Ensemble(n, d, intercepts=nengo.Uniform(-0.2, 0.6))
        out = nengo.Node(size_in=d_out)
        nengo.Connection(key, mem, synapse=None, learning_rule_type=nengo.Voja(learning_rate=1e-3, post_synapse=None))
        learned = nengo.Connection(mem, out, synapse=0.005, transform=np.zeros((d_out, d)),
                                   learning_rule_type=nengo.PES(learning_rate=1e-4))
        err = nengo.Node(size_in=d_out)
        nengo.Connection(out, err, synapse=None)
        nengo.Connection(err_src, err, transform=-1.0, synapse=None)
        nengo.Connection(err, learned.learning_rule, synapse=None)
        nengo.Probe(out, synapse=0.01)
    return build(net)


LEARNING_POINTS = (10, 30, 63, 128, 193, 195, 197, 199)      # 128 and 193 follow a call of exactly 64 timesteps


def overlapping_filters(micros, lo, n):
    return [m for m in micros if m[0] == M_LOWPASS and m[2] < lo + n and lo < m[2] + m[1]]


def test_learning_network_neuron_major(Simulator, capfd):
    """The default plan keeps the 5 x 1100 decoders neuron-major (they multiply a spike vector), so the PES body sees 1100 rows and 5
    columns: one column tile, 34 blocks of 32 rows and one of 12, with the activity filter folded into it (lp_dst) - bit-equal to the
    run with the fold switched off.  Voja on 1100 rows: a partly filled last wave.  Both rules live at every restart point."""
    model = learning_network()
    pes = [o for o in model.ops if o["kind"] == "pes"][0]
    voja = [o for o in model.ops if o["kind"] == "voja"][0]
    assert (pes["rows"], pes["cols"], voja["rows"]) == (5, 1100, 1100) and 1100 % 32 == 12
    sim, bodies, micros = planned(Simulator, capfd, model)
    assert bodies[RK_PES] == {(1, 35)} and RK_VOJA in bodies, bodies
    assert not overlapping_filters(micros, pes["act"], pes["cols"]), micros
    s, c, names = restart_run(sim, model, LEARNING_POINTS, 200, "learning network, neuron-major")
    assert_passes(s, ("pes", "voja", "neurons", "lowpass"))
    assert s["live"]["pes"] == len(LEARNING_POINTS) and s["live"]["voja"] == len(LEARNING_POINTS), s["live"]
    states = []
    for fold in (None, "0"):
        sim, bodies, micros = planned(Simulator, capfd, model, env={"SSN_PES_FOLD": fold})
        assert bool(overlapping_filters(micros, pes["act"], pes["cols"])) == (fold == "0"), (fold, micros)
        with sim:
            sim.run_steps(150)
            states.append(R.read_state(model, sim))
    np.testing.assert_array_equal(states[0][0], states[1][0])
    for i in states[0][1]:
        np.testing.assert_array_equal(states[0][1][i], states[1][1][i], err_msg=model.buffer_meta[i]["name"])


def test_learning_network_over_two_column_tiles(Simulator, capfd):
    """SSN_PLAN_NO_SPMV keeps the 5 x 1100 matrix row-major: the PES body sees 5 rows and 1100 columns, two 1024-column tiles (the
    second holds 76), and the fold is not planned there (the activity filter stays an operator of its own)."""
    model = learning_network()
    pes = [o for o in model.ops if o["kind"] == "pes"][0]
    sim, bodies, micros = planned(Simulator, capfd, model, flags=PLAN.SSN_PLAN_NO_SPMV)
    assert bodies[RK_PES] == {(2, 1)}, bodies
    assert overlapping_filters(micros, pes["act"], pes["cols"]), micros
    s, c, names = restart_run(sim, model, LEARNING_POINTS, 200, "learning network, row-major")
    assert_passes(s, ("pes", "voja", "neurons", "lowpass"))
    assert s["live"]["pes"] == len(LEARNING_POINTS) and s["live"]["voja"] == len(LEARNING_POINTS), s["live"]


@pytest.mark.parametrize("block,steps", [(64, 128), (256, 256)])
def test_single_step_launches_equal_the_step_graph(Simulator, small, block, steps):
    """One ``run_steps(steps)`` call (whole blocks of the pipelined step graph) and ``steps`` calls of run_steps(1) (the launches the
    restart checks look at) leave the same bits in every state buffer, learned buffer and carried signal of the per-timestep core.
    The filters of the time-batched stages are scans along time whose arithmetic depends on the block length:
    kb_lowpass in blocks of 64, kb_lowpass_chunked from 256 on, the length at which the benchmark's default blocks run.  The probed
    output of such a filter is held at EVERY step of both runs to a float64 filter under the low-pass bound of tests/slam_restart.py,
    accumulated along the run.  The float64 filter is fed the inputs of the single-step run; those of the long run cannot be read
    step by step: they are compared at its last step, and they are a function of the core's state, which is bit-equal at the end."""
    sm, model = small
    c = R.carried(model)
    batched = [o for o in model.ops if o["kind"] == "lowpass" and o["stage"] != 1]
    assert len(batched) == 1 and batched[0]["stage"] == 2 and batched[0]["dst"] == model.probes[0]["src"] and model.probes[0]["probe"] is sm.probe
    o = batched[0]
    y, b = np.array(model.sig_init[o["dst"]:o["dst"] + o["len"]], dtype=np.float64), np.zeros(o["len"])
    want, bound = [], []
    states, outputs = [], []
    for chunk in (steps, 1):
        with Simulator(None, model=model, dtype="f32", block_steps=block) as sim:
            for _ in range(steps // chunk):
                sim.run_steps(chunk)
                if chunk == 1:          # the float64 filter of the inputs this device saw, with its bound
                    x = sim.read_signal(o["src"], o["len"])
                    t1, t2 = o["a"] * y, (1.0 - o["a"]) * o["gain"] * x
                    b = abs(o["a"]) * b + 3 * R.U * (np.abs(t1) + np.abs(t2))
                    y = t1 + t2
                    want.append(y)
                    bound.append(b + 2 * R.U * np.abs(y))
            states.append(R.read_state(model, sim))
            outputs.append(np.array(sim.data[sm.probe]))
    want, bound = np.array(want), np.array(bound)
    sl = slice(o["dst"], o["dst"] + o["len"])
    np.testing.assert_array_equal(states[0][0][o["src"]:o["src"] + o["len"]], states[1][0][o["src"]:o["src"] + o["len"]])
    for out, name in zip(outputs, ("one call", "single steps")):
        assert out.shape == want.shape, (out.shape, want.shape)
        ratio = R._ratio(np.abs(out - want), bound)          # (0 where the two are equal: the first rows are all zero)
        print("block %d, batched filter %d:%d, %s: worst |device - float64| / bound over %d steps %.3f; %d of %d elements differ between the runs at the end"
              % (block, sl.start, sl.stop, name, steps, ratio.max(), int((states[0][0][sl] != states[1][0][sl]).sum()), o["len"]))
        assert ratio.max() <= 1.0, (name, ratio.max())
    exact = c.mask.copy()
    exact[sl] = False
    for lo, hi in R._ranges(exact):
        np.testing.assert_array_equal(states[0][0][lo:hi], states[1][0][lo:hi], err_msg="signals %d:%d" % (lo, hi))
    for i in c.buffers:
        np.testing.assert_array_equal(states[0][1][i], states[1][1][i], err_msg=model.buffer_meta[i]["name"])
