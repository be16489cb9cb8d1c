"""The pipelined tail of k_ens_block's f32 time loop (csrc/ssn_block.hpp): the next timestep's input row is read from LDS in
front of the wave reduction, and the state half of the LIF step of some neuron groups is computed one timestep ahead, in
the waits of the cross-wave sum.  What that adds to the kernel sits at the edges of a launch and of its 32-timestep
chunks: the row prefetch at a chunk's last timestep (chunks of fewer than 32, of exactly 32 timesteps, launches of one
timestep), and the hoisted state half at the first and at the last timestep of a launch.

The block length only cuts the same recurrence into launches.  The runs at different block lengths are nevertheless not
equal bit for bit, and were not before the pipelined tail existed: the time-batched stages beside the kernel round
differently at different batch lengths (measured with the kernel of the commit before, block_steps = 1 against 64: 294 - 543
of 910 probe values differ, by at most 6e-8 - 1.1e-5).  So every block length is compared with the per-timestep kernel
(flags = SSN_PLAN_NO_BLOCK_KERNEL) under the suite's 1e-3 cosine bar for f32 runs; the differences from the block_steps = 64
run are printed."""
import os

import numpy as np
import pytest

import sspslam_amd.frontend as nengo
from sspslam_amd import harness as H
from sspslam_amd import simulator as PLAN
from sspslam_amd.modelcache import cached_build as build

from helpers import small_pathint

pytestmark = pytest.mark.gpu

STEPS = 130
BLOCKS = (1, 2, 31, 32, 33, 65)


@pytest.fixture(scope="module")
def Simulator():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from sspslam_amd.simulator import Simulator
    return Simulator


def run(Simulator, model, probes, block_steps, variant):
    os.environ.pop("SSN_BLOCK_VARIANT", None)
    if variant:
        os.environ["SSN_BLOCK_VARIANT"] = variant
    try:
        with Simulator(None, model=model, dtype="f32", block_steps=block_steps) as sim:
            sim.run_steps(STEPS)
            c = sim.counters()
            assert c["launches_per_step"] == 0, c                      # the whole-block kernel steps the oscillators
            if variant:
                assert "%d,%d,%d" % (c["block_tpb"], c["block_npt"], c["block_enc_lds"]) == variant, c
            return [np.array(sim.data[p]) for p in probes]
    finally:
        os.environ.pop("SSN_BLOCK_VARIANT", None)


# (neurons per oscillator, forced kernel variant, five decoded rows): the two variants with the pipelined tail and the
# hoisted state halves / the prefetch alone, two variants that keep the plain loop, the planner's own choice at a small
# size, and a model whose probe keeps the oscillators' fifth decoded row (DOUT = 5)
CASES = [(5200, "512,20,3", False), (5200, "768,14,3", False), (2500, "512,10,0", False), (2500, "1024,6,0", False),
         (700, None, False), (5200, "512,20,3", True), (2500, "512,10,0", True)]


@pytest.mark.parametrize("n,variant,five_rows", CASES)
def test_block_length_does_not_change_the_run(Simulator, n, variant, five_rows):
    pm = small_pathint(ssp_dim=19, n=n, T=10.0, limit=0.2)
    probes = [pm.probe]
    if five_rows:
        with pm.model:
            probes.append(nengo.Probe(pm.pathintegrator.oscillators.output, synapse=None))
    model = build(pm.model, n_eval_points=300)
    with Simulator(None, model=model, dtype="f32", flags=PLAN.SSN_PLAN_NO_BLOCK_KERNEL, block_steps=64) as sim:
        sim.run_steps(STEPS)
        assert sim.counters()["launches_per_step"] > 0
        want = [np.array(sim.data[p]) for p in probes]
    assert all(w.shape[0] == STEPS and np.isfinite(w).all() for w in want)
    assert np.abs(want[0][20:]).max() > 0.01                           # (a run in which something happens)
    at64 = run(Simulator, model, probes, 64, variant)
    for bs in BLOCKS + (64,):
        got = run(Simulator, model, probes, bs, variant) if bs != 64 else at64
        for g, w, g64 in zip(got, want, at64):
            ce = float(H.cosine_error(g[20:], w[20:]).max())
            print("n %d variant %s five rows %s block_steps %d: max cosine error vs the per-timestep kernel %.3e (bar 1e-3); "
                  "%d of %d values differ from block_steps 64, max |diff| %.3e"
                  % (n, variant, five_rows, bs, ce, int(np.count_nonzero(g != g64)), g.size, float(np.abs(g - g64).max())))
            assert g.shape == w.shape and np.isfinite(g).all()
            assert ce < 1e-3, (n, variant, five_rows, bs, ce)
