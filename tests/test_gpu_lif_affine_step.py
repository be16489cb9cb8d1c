"""The f32 whole-block kernel's affine LIF step (csrc/ssn_block.hpp; tests/test_lif_affine_step.py is its CPU restatement) on the
GPU, with the open-loop instrument of tests/lif_open_loop.py (checks A, B, C; bars: the reference's float32 yardstick plus that
module's documented terms) at the smallest shapes that reach the code: (512, 10) in registers, (512, 20, LDS) with the hoisted
state halves and the interleaved row sum, (768, 14, LDS) without a hoist; launches of 1, 2 and 33 timesteps, so that the
conversion between the HBM word and the loop word happens at every step, every other step and across a 32-step chunk edge; a
model whose refractory scale is below what the planner admits; four decoded rows.

Every case asserts through ``counters()`` which kernel ran.  The figures are printed before they are asserted (run with -s)."""
import contextlib
import functools
import os

import numpy as np
import pytest

import sspslam_amd.frontend as nengo
from oracle import OracleSimulator

import lif_open_loop as L

pytestmark = pytest.mark.gpu

STEPS, T0 = 130, 77
MS = (1, 2, 33)


@pytest.fixture(scope="module")
def Simulator():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from sspslam_amd.simulator import Simulator
    return Simulator


@contextlib.contextmanager
def forced(variant):
    os.environ.pop("SSN_BLOCK_VARIANT", None)
    os.environ["SSN_BLOCK_VARIANT"] = variant
    try:
        yield
    finally:
        os.environ.pop("SSN_BLOCK_VARIANT", None)


@functools.lru_cache(maxsize=None)
def case(n, tau_rc, tau_ref):
    """(open-loop model, float64 run, float32 yardstick, float64 oracle at T0): computed once per model, shared, never changed."""
    if tau_ref * 200.0 < 1.0:
        ol = L.open_loop_pathint(n, ssp_dim=7, neuron_type=nengo.LIF(tau_rc=tau_rc, tau_ref=tau_ref))
    else:
        # (no ensemble with the default maximum rates can be built at such a tau_ref: the constant is changed in the built
        #  model - gains and biases stay those of LIF(tau_rc, 0.002), the input currents are what they were)
        ol = L.open_loop_pathint(n, ssp_dim=7, neuron_type=nengo.LIF(tau_rc=tau_rc, tau_ref=0.002))
        ol.model = L.with_lif_constants(ol.model, tau_ref_scale=tau_ref / 0.002)
        ol.ens = next(o for o in ol.model.ops if o["kind"] == "ensarray")
        ol.tau_ref = ol.ens["neuron"]["tau_ref"]
        assert abs(ol.tau_ref - tau_ref) < 1e-12
    assert ol.ens["dout"] == 5
    ref64 = L.reference_run(ol, STEPS)
    yard = L.reference_run(ol, STEPS, np.float32)
    at_T0 = OracleSimulator(ol.model)
    at_T0.run_steps(T0)
    ref64.setflags(write=False)
    yard.setflags(write=False)
    return ol, ref64, yard, at_T0


def assert_kernel(c, variant, block):
    if block:
        assert c["launches_per_step"] == 0, c
        assert "%d,%d,%d" % (c["block_tpb"], c["block_npt"], c["block_enc_lds"]) == variant, c
    else:
        assert c["launches_per_step"] > 0 and c["block_tpb"] == 0, c


def run_checks(Simulator, n, tau_rc, tau_ref, variant, block=True, label="", **sim_kw):
    ol, ref64, yard, at_T0 = case(n, tau_rc, tau_ref)
    with forced(variant), Simulator(None, model=ol.model, dtype="f32", **sim_kw) as sim:
        sim.run_steps(STEPS)
        c = sim.counters()
        assert_kernel(c, variant, block)
        assert c["n_steps"] == STEPS
        dev = L.observed(ol, sim.data[ol.probe_key()])
        ok_c, info_c = L.check_exact(ol, dev, STEPS)
        print("%s C %s" % (label, info_c))
        ok_a, info_a = L.check_drift(ol, dev, ref64, yard)
        print("%s A D %s yardstick %s bar %s spikes %s" % (label, info_a["D"], info_a["D_yardstick"], info_a["bar"], info_a["spikes_f64"]))
        results = []
        for m in MS:
            sim.reset()
            results.append(L.check_restart(ol, sim, at_T0, T0, m))
            print("%s B %s" % (label, results[-1][1]))
        assert_kernel(sim.counters(), variant, block)
    assert ok_c, info_c
    assert ok_a, info_a
    for ok_b, info_b in results:
        assert ok_b, info_b


# (variant, neurons per VCO: no multiple of the workgroup size, a last group that is partly empty, more than one wave per SIMD)
SHAPES = [("512,10,0", 2500), ("512,20,3", 5200), ("768,14,3", 5200)]


@pytest.mark.parametrize("block_steps", [1, 2, 33])
@pytest.mark.parametrize("tau_rc,tau_ref", [(0.02, 0.002), (0.02, 0.001)])
@pytest.mark.parametrize("variant,n", SHAPES)
def test_affine_step_on_the_block_kernel(Simulator, variant, n, tau_rc, tau_ref, block_steps):
    run_checks(Simulator, n, tau_rc, tau_ref, variant, block_steps=block_steps,
               label="f32 %s n %d LIF(%g, %g) block_steps %d" % (variant, n, tau_rc, tau_ref, block_steps))


def test_refractory_scale_below_four_runs_the_per_timestep_kernel(Simulator):
    """LIF(0.02, 0.0137): kappa = 1 - the planner keeps the model off the block kernel; the per-timestep kernel passes the same checks."""
    run_checks(Simulator, 2500, 0.02, 0.0137, "512,10,0", block=False, label="f32 LIF(0.02, 0.0137)")


def test_five_decoded_rows_at_the_headline_variant(Simulator):
    """The raw probe makes the array decode five rows (asserted in ``case``): (512, 20, LDS) at the default block length, one
    launch of 130 timesteps (four chunks of 32 and one of 2)."""
    run_checks(Simulator, 5200, 0.02, 0.002, "512,20,3", label="f32 512,20,3 dout 5 one launch")


def test_four_decoded_rows_at_the_headline_variant(Simulator):
    """DOUT = 4 (no unfiltered probe; the instantiation the benchmark runs): count and checksum read with ``read_signal`` after
    launches of ONE timestep for checks A and C, check B at the usual launch lengths."""
    n = 5200
    ol = L.open_loop_pathint(n, ssp_dim=7, raw_probe=False)
    assert ol.ens["dout"] == 4
    lo, hi = int(ol.sig.min()), int(ol.sig.max()) + 1
    refs = []
    for dtype in (np.float64, np.float32):
        o = OracleSimulator(ol.model, dtype=dtype)
        rows = []
        for _ in range(STEPS):
            o.step()
            rows.append(np.array(o.sig[ol.sig], dtype=np.float64))
        refs.append(np.array(rows))
    at_T0 = OracleSimulator(ol.model)
    at_T0.run_steps(T0)
    with forced("512,20,3"), Simulator(None, model=ol.model, dtype="f32") as sim:
        rows = []
        for _ in range(STEPS):
            sim.run_steps(1)
            rows.append(sim.read_signal(lo, hi - lo)[ol.sig - lo])
        dev = np.array(rows)
        assert_kernel(sim.counters(), "512,20,3", True)
        ok_c, info_c = L.check_exact(ol, dev, STEPS)
        print("dout 4 C", info_c)
        ok_a, info_a = L.check_drift(ol, dev, refs[0], refs[1])
        print("dout 4 A", info_a)
        results = []
        for m in MS:
            sim.reset()
            results.append(L.check_restart(ol, sim, at_T0, T0, m))
            print("dout 4 B", results[-1][1])
        assert_kernel(sim.counters(), "512,20,3", True)
    assert ok_c, info_c
    assert ok_a, info_a
    for ok_b, info_b in results:
        assert ok_b, info_b
