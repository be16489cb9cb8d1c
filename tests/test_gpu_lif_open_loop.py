"""The LIF kernels against a float64 LIF step, spike by spike, on the open-loop model of tests/lif_open_loop.py (its docstring
derives the bars; tests/test_lif_open_loop.py proves the instrument on the CPU): every f32 variant of the whole-block kernel at
its capacity and at a ragged size, the headline variant at the benchmark's size and at other block lengths and with four decoded
rows, LIF constants at the edges of what the planner admits, the per-timestep f32 kernel and the f64 block variants.

Every case asserts through ``counters()`` which kernel ran.  The figures are printed before they are asserted (run with -s)."""
import contextlib
import os
import time

import numpy as np
import pytest

import sspslam_amd.frontend as nengo
from sspslam_amd import simulator as PLAN
from oracle import OracleSimulator

import lif_open_loop as L

pytestmark = pytest.mark.gpu

STEPS, T0 = 1000, 77
MS = (1, 2, 33, 65)


@pytest.fixture(scope="module")
def Simulator():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from sspslam_amd.simulator import Simulator
    return Simulator


@contextlib.contextmanager
def forced(variant):
    os.environ.pop("SSN_BLOCK_VARIANT", None)
    if variant:
        os.environ["SSN_BLOCK_VARIANT"] = variant
    try:
        yield
    finally:
        os.environ.pop("SSN_BLOCK_VARIANT", None)


def assert_kernel(c, variant, block):
    """The kernel under test really ran: the whole-block kernel in the forced variant, or the per-timestep kernel."""
    if block:
        assert c["launches_per_step"] == 0, c
        if variant:
            assert "%d,%d,%d" % (c["block_tpb"], c["block_npt"], c["block_enc_lds"]) == variant, c
    else:
        assert c["launches_per_step"] > 0 and c["block_tpb"] == 0, c


def run_checks(Simulator, ol, variant, dtype="f32", block=True, exact=False, ms=MS, label="", **sim_kw):
    """Checks C and A over STEPS steps from reset, then check B at T0 for every m (each from a reset)."""
    t0 = time.time()
    ref64 = L.reference_run(ol, STEPS)
    yard = ref64 if exact else L.reference_run(ol, STEPS, np.float32)
    at_T0 = OracleSimulator(ol.model)
    at_T0.run_steps(T0)
    if not exact:                      # the yardstick's own restart deviations, printed beside the device's
        for m in (1, 33):
            print("%s B yardstick %s" % (label, L.check_restart(ol, L.OracleRun(ol.model, np.float32), at_T0, T0, m)[1]))
    t_ref = time.time() - t0
    with forced(variant), Simulator(None, model=ol.model, dtype=dtype, **sim_kw) as sim:
        sim.run_steps(STEPS)
        c = sim.counters()
        assert_kernel(c, variant, block)
        assert c["n_steps"] == STEPS
        dev = L.observed(ol, sim.data[ol.probe_key()])
        ok_c, info_c = L.check_exact(ol, dev, STEPS)
        print("%s C %s" % (label, info_c))
        ok_a, info_a = L.check_drift(ol, dev, ref64, yard, exact=exact)
        print("%s A D %s yardstick %s bar %s first step %s spikes %s" % (label, info_a["D"], info_a["D_yardstick"], info_a["bar"],
                                                                        info_a["first_step_of_D"], info_a["spikes_f64"]))
        results = []
        for m in ms:
            sim.reset()
            ok_b, info_b = L.check_restart(ol, sim, at_T0, T0, m, exact_tol=1e-12 if exact else None)
            print("%s B %s" % (label, info_b))
            results.append((ok_b, info_b))
        assert_kernel(sim.counters(), variant, block)
    print("%s wall %.1f s (references %.1f s)" % (label, time.time() - t0, t_ref))
    assert ok_c, info_c
    assert ok_a, info_a
    for ok_b, info_b in results:
        assert ok_b, info_b
    return dev


# (variant, capacity tpb * npt, a ragged size below it: odd, no multiple of 4 or of npt)
F32_VARIANTS = [("1024,2,0", 2048, 1999), ("1024,4,0", 4096, 4093), ("512,6,0", 3072, 3067), ("1024,6,0", 6144, 6139),
                ("512,10,0", 5120, 5111), ("512,20,3", 10240, 10223), ("768,14,3", 10752, 10739)]


@pytest.mark.parametrize("variant,n", [(v, cap) for v, cap, _ in F32_VARIANTS] + [(v, rag) for v, _, rag in F32_VARIANTS])
def test_f32_block_variant(Simulator, variant, n):
    """All seven f32 variants of k_ens_block, 1000 steps at the default block length (31 chunks of 32 timesteps and one of 8),
    launches of 1, 2, 33 and 65 timesteps from step 77 (the hoisted halves' first and last steps, a chunk edge)."""
    tpb, npt, _ = (int(s) for s in variant.split(","))
    assert n <= tpb * npt and (n == tpb * npt or (n % 2 == 1 and n % npt != 0))
    ol = L.open_loop_pathint(n, ssp_dim=7)
    run_checks(Simulator, ol, variant, label="f32 %s n %d" % (variant, n))


def test_headline_variant_at_the_benchmark_size(Simulator):
    """(512, 20, LDS) at n = 10 000 on the planner's own choice; and a reset followed by the same run: bit-equal."""
    ol = L.open_loop_pathint(10000, ssp_dim=7)
    dev = run_checks(Simulator, ol, None, label="f32 headline n 10000")
    with forced(None), Simulator(None, model=ol.model, dtype="f32") as sim:
        outs = []
        for _ in range(2):
            sim.run_steps(STEPS)
            c = sim.counters()
            assert (c["launches_per_step"], c["block_tpb"], c["block_npt"], c["block_enc_lds"]) == (0, 512, 20, 3), c
            outs.append((np.array(sim.data[ol.probe_key()]), sim.read_buffer(ol.ens["v"]), sim.read_buffer(ol.ens["r"])))
            sim.reset()
            assert sim.n_steps == 0 and not sim.read_buffer(ol.ens["v"]).any() and not sim.read_buffer(ol.ens["r"]).any()
    for a, b in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(L.observed(ol, outs[0][0]), dev)


@pytest.mark.parametrize("block_steps", [33, 100])
def test_headline_variant_other_block_lengths(Simulator, block_steps):
    """Launches of 33 (a chunk and one timestep) and of 100 timesteps (three chunks and one of 4)."""
    ol = L.open_loop_pathint(10000, ssp_dim=7)
    run_checks(Simulator, ol, "512,20,3", label="f32 headline block_steps %d" % block_steps, block_steps=block_steps)


def test_headline_variant_with_four_decoded_rows(Simulator):
    """DOUT = 4: without the unfiltered probe the array decodes four rows, two of them observed (count, checksum).  No unfiltered probe
    reaches them without becoming a fifth row (a probe of the array's output makes its third dimension live; behind the read-out
    matrix only a low-pass filtered signal exists), so they are read with ``read_signal`` after every launch: launches of ONE timestep
    for checks A and C over 300 steps - every step the first and the last of its launch - and check B at the usual launch lengths."""
    n, steps = 10000, 300
    ol = L.open_loop_pathint(n, ssp_dim=7, raw_probe=False)
    assert ol.ens["dout"] == 4
    lo, hi = int(ol.sig.min()), int(ol.sig.max()) + 1
    refs = []
    for dtype in (np.float64, np.float32):
        o = OracleSimulator(ol.model, dtype=dtype)
        rows = []
        for _ in range(steps):
            o.step()
            rows.append(np.array(o.sig[ol.sig], dtype=np.float64))
        refs.append(np.array(rows))
    at_T0 = OracleSimulator(ol.model)
    at_T0.run_steps(T0)
    with forced("512,20,3"), Simulator(None, model=ol.model, dtype="f32") as sim:
        rows = []
        for _ in range(steps):
            sim.run_steps(1)
            rows.append(sim.read_signal(lo, hi - lo)[ol.sig - lo])
        dev = np.array(rows)
        assert_kernel(sim.counters(), "512,20,3", True)
        ok_c, info_c = L.check_exact(ol, dev, steps)
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


@pytest.mark.parametrize("tau_rc,tau_ref,block", [(0.02, 0.001, True), (0.02, 2.0 ** -9, True), (0.05, 0.0022, True),
                                                  (0.03, 0.0005, False), (0.006, 0.002, False)])
def test_lif_constants_through_the_f32_kernels(Simulator, tau_rc, tau_ref, block):
    """tau_ref = dt; tau_ref = 2^-9 (K tau_ref = 1 exactly); (0.05, 0.0022); and two sets the branch-free step does not cover
    (tau_ref < dt; dt / tau_rc > 1 / 20), which must fall back to the per-timestep kernel and pass the same checks."""
    ol = L.open_loop_pathint(2500, ssp_dim=7, neuron_type=nengo.LIF(tau_rc=tau_rc, tau_ref=tau_ref))
    run_checks(Simulator, ol, "512,10,0", block=block, label="f32 LIF(%g, %g)" % (tau_rc, tau_ref))


def test_per_timestep_f32_kernel_above_the_block_capacity(Simulator):
    """k_ensarray (flags = SSN_PLAN_NO_BLOCK_KERNEL) at n = 12 000: the path of populations no block variant holds."""
    ol = L.open_loop_pathint(12000, ssp_dim=7)
    run_checks(Simulator, ol, None, block=False, label="f32 per-timestep n 12000", flags=PLAN.SSN_PLAN_NO_BLOCK_KERNEL)


@pytest.mark.parametrize("variant,n", [("1024,1,0", 1024), ("1024,2,0", 2039), ("1024,4,0", 4093)])
def test_f64_block_variant_equals_the_oracle(Simulator, variant, n):
    """The f64 variants restate the oracle's step operation for operation: counts, checksums and trains equal, the state within 1e-12."""
    ol = L.open_loop_pathint(n, ssp_dim=7)
    run_checks(Simulator, ol, variant, dtype="f64", exact=True, label="f64 %s n %d" % (variant, n))
