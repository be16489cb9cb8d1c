"""The open-loop LIF instrument (tests/lif_open_loop.py) proved on the CPU before it is pointed at a kernel
(tests/test_gpu_lif_open_loop.py): the observed decoder rows give f32 sums that do not depend on the summation order, the
yardstick (the oracle in np.float32) passes checks A, B and C against the float64 oracle at the default LIF constants and at
the parameter edges the planner admits, and every mutated reference is rejected."""
import functools

import numpy as np
import pytest

import sspslam_amd.frontend as nengo
from oracle import OracleSimulator

import lif_open_loop as L

STEPS, T0 = 1000, 77
MS = (1, 2, 33, 65)


@functools.lru_cache(maxsize=None)
def case(n, tau_rc=None, tau_ref=None):
    """(open-loop model, float64 run, yardstick run, float64 oracle at step T0)"""
    lif = None if tau_rc is None else nengo.LIF(tau_rc=tau_rc, tau_ref=tau_ref)
    ol = L.open_loop_pathint(n, ssp_dim=7, neuron_type=lif)
    ref64 = L.reference_run(ol, STEPS)
    yard = L.reference_run(ol, STEPS, np.float32)
    at_T0 = OracleSimulator(ol.model)
    at_T0.run_steps(T0)
    return ol, ref64, yard, at_T0


def test_observed_rows_sum_to_the_same_f32_value_in_any_order():
    """n = 10 240 neurons, 40 % of them firing: count, checksum and one-hot sums in float32, summed in shuffled orders, in chunks of
    every workgroup shape of the block kernel (waves of 64, groups of 2 - 20 per thread) and pairwise (np.sum) - all equal to the integer sum."""
    rng = np.random.RandomState(0)
    n = 10240
    w = np.stack([np.ones(n), (np.arange(n) % L.CHECKSUM_MOD) + 1.0, np.eye(1, n, 777)[0]]).astype(np.float32)
    for trial in range(5):
        spk = (rng.rand(n) < 0.4).astype(np.float32)
        spk[777] = 1.0
        exact = (w.astype(np.int64) * spk.astype(np.int64)).sum(axis=1)
        assert exact[1] < 2 ** 24 and exact[1] <= 16 * 0.5 * n
        terms = w * spk
        sums = [terms.sum(axis=1, dtype=np.float32)]
        for _ in range(3):
            p = rng.permutation(n)
            acc = np.zeros(3, dtype=np.float32)
            for i in p:                                         # one serial chain in a random order
                acc = acc + terms[:, i]
            sums.append(acc)
        for chunk in (2, 20, 64, 128, 1024):
            part = terms.reshape(3, -1, chunk).sum(axis=2, dtype=np.float32)         # per thread / wave / workgroup partial sums
            acc = np.zeros(3, dtype=np.float32)
            for j in rng.permutation(part.shape[1]):
                acc = acc + part[:, j]
            sums.append(acc)
        for s in sums:
            assert s.dtype == np.float32 and np.array_equal(s.astype(np.int64), exact), (s, exact)


CASES = [(700, None, None), (5200, None, None), (700, 0.02, 0.001), (700, 0.02, 2.0 ** -9), (700, 0.05, 0.0022)]


@pytest.mark.parametrize("n,tau_rc,tau_ref", CASES)
def test_yardstick_passes_every_check(n, tau_rc, tau_ref):
    """default LIF at n = 700 and n = 5200; tau_ref = dt; tau_ref = 2^-9 (K tau_ref = 1 exactly in the block kernel's time unit);
    (tau_rc, tau_ref) = (0.05, 0.0022).  The yardstick's own D is part of check A's bar, so what A asserts of it here is that the
    documented-error allowance is not negative and the cumulative count differs by a few spikes at most (measured: 1 - 2)."""
    ol, ref64, yard, at_T0 = case(n, tau_rc, tau_ref)
    ok, info = L.check_exact(ol, yard, STEPS)
    print("C yardstick", info)
    assert ok, info
    ok, info = L.check_exact(ol, ref64, STEPS)
    assert ok, info
    ok, info = L.check_drift(ol, yard, ref64, yard)
    print("A yardstick", info)
    assert ok, info
    assert np.array(info["D_yardstick"])[:, L.COUNT].max() <= 4, info                 # (the reference's own f32 error stays a few spikes)
    assert min(info["spikes_f64"]) > 20 * n                                           # (a run in which every VCO is busy)
    for m in MS:
        ok, info = L.check_restart(ol, L.OracleRun(ol.model, np.float32), at_T0, T0, m)
        print("B yardstick", info)
        assert ok, info
        assert info["disagree"] <= max(1, int(0.00005 * info["neurons"]) + 1), info    # (the yardstick: 0.005 % or below)


def test_exact_float64_run_passes_with_zero_bars():
    ol, ref64, yard, at_T0 = case(700)
    again = L.reference_run(ol, STEPS)
    ok, info = L.check_drift(ol, again, ref64, yard, exact=True)
    assert ok, info
    ok, info = L.check_restart(ol, L.OracleRun(ol.model), at_T0, T0, 33, exact_tol=1e-12)
    assert ok and info["max_dV"] == 0.0, info


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("which,scale", [("tau_ref", 1.0005), ("tau_rc", 1.0002)])
def test_mutated_lif_constant_fails_check_a(which, scale, dtype):
    """A refractory period longer by 1 us, a membrane time constant longer by 4 us: the cumulative spike count leaves the bar."""
    ol, ref64, yard, _ = case(5200)
    mutant = L.with_lif_constants(ol.model, **{which + "_scale": scale})
    got = L.reference_run(ol, STEPS, dtype, model=mutant)
    ok, info = L.check_exact(ol, got, STEPS)
    assert ok, info                                                                    # (still a well-formed run: only A sees it)
    ok, info = L.check_drift(ol, got, ref64, yard)
    print(which, scale, dtype.__name__, "D", np.array(info["D"])[:, L.COUNT], "bar", np.array(info["bar"])[:, L.COUNT])
    assert not ok, info
    assert (np.array(info["D"])[1:, L.COUNT] > 5 * np.array(info["bar"])[1:, L.COUNT]).all(), info


def test_dropped_spikes_of_a_slice_fail_check_a():
    """The spikes of neurons 64 .. 127 left out of the decode at every 32nd step (a chunk's last timestep)."""
    ol, ref64, yard, _ = case(700)
    got = L.reference_run(ol, STEPS, np.float32, drop=(slice(64, 128), 32))
    ok, info = L.check_drift(ol, got, ref64, yard)
    assert not ok, info
    assert (np.array(info["D"])[:, L.COUNT] > np.array(info["bar"])[:, L.COUNT]).all(), info


def test_a_tail_neuron_that_never_fires_fails_check_a():
    """The last neuron of a ragged n (the one-hot neuron is near the tail) silent: the count drifts by its spikes, the train is empty."""
    ol, ref64, yard, _ = case(700)
    hot = int(ol.hot[1])
    got = L.reference_run(ol, STEPS, np.float32, drop=(slice(hot, hot + 1), 1))
    ok, info = L.check_drift(ol, got, ref64, yard)
    assert not ok and np.array(info["D"])[1, L.TRAIN] > 1, info


def test_swapped_restart_state_fails_check_b():
    ol, _, _, at_T0 = case(700)

    def swap(V, R):
        k = 1
        i, j = int(np.argmax(V[k])), int(np.argmax(R[k]))           # an integrating neuron and a refractory one
        assert V[k, i] > 0.5 and R[k, j] > 0 and V[k, j] == 0
        V[k, [i, j]] = V[k, [j, i]]
        R[k, [i, j]] = R[k, [j, i]]
        return V, R

    for m in (1, 33):
        ok, info = L.check_restart(ol, L.OracleRun(ol.model, np.float32), at_T0, T0, m, mutate=swap)
        print(info)
        assert not ok and info["disagree_not_marginal"] >= 1, info


def test_malformed_samples_fail_check_c():
    ol, ref64, _, _ = case(700)
    ok, _ = L.check_exact(ol, ref64[:-1], STEPS)                      # a missing sample
    assert not ok
    for k, (row, value) in enumerate([(L.COUNT, 0.5), (L.COUNT, ol.n + 1.0), (L.CHECKSUM, -1.0), (L.TRAIN, 2.0)]):
        bad = ref64.copy()
        bad[500 + k, 1, row] = value
        ok, info = L.check_exact(ol, bad, STEPS)
        assert not ok, (row, value, info)
    bad = ref64.copy()
    bad[31, 2] = 0.0                                                   # a decode dropped at a chunk's last timestep: A sees it
    ok, info = L.check_drift(ol, bad, ref64, ref64)
    assert not ok, info
