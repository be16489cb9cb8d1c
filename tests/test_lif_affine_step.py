"""The f32 whole-block kernel's LIF step (csrc/ssn_block.hpp: refractory word affine in the spike's overshoot, no polynomial)
restated in NumPy float32 and held against the float64 step ``oracle.stepper.lif_step`` on the open-loop model of
tests/lif_open_loop.py - before the kernel is run anywhere.

The restatement is the kernel's eleven packed operations, one by one: every FMA is a float64 product and sum rounded once to
float32 (the product of two float32 is exact in float64), the clamp is the VOP3P one ([0, 1], NaN -> 0), the constants are made
by the kernel's rules (in double, rounded to float32), and the state word goes through the HBM form (s >= 0: V; s < 0:
-(R - dt)) with float32 ``expm1`` / ``log1p`` either at every step (launches of one timestep) or never (one long launch).

Conditions: the bound of ``lif_open_loop.restart_reference`` is propagated beside the float64 run from reset over all steps
with that module's ``BLOCK_TERMS``; a neuron whose float64 run has a decision inside its own bound is marginal.  Spike counts
per neuron are equal for every neuron that is not marginal, and the final states pass ``compare_states``.  Two mutants - the
spike-time constant ``A`` off by one part in 1e-4, the refractory decay ``q`` replaced by 1 - must fail."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import sspslam_amd.frontend as nengo
from oracle import OracleSimulator
from oracle.stepper import lif_step

import lif_open_loop as L

N, STEPS = 5000, 300                         # 4 VCOs x 5000 = 20 000 neurons
F = np.float32
# (tau_rc, tau_ref) -> kappa: every constant set the existing tests expect on the block kernel
SETS = {(0.02, 0.002): 8, (0.02, 0.001): 16, (0.02, 2.0 ** -9): 8, (0.05, 0.0022): 16}


def affine_constants(dt, tau_rc, tau_ref):
    """The kernel's constants (lif_const_affine): double arithmetic, each rounded to float32 once."""
    h = dt / tau_rc
    q, E1, C1 = math.exp(-h), -math.expm1(-h), math.exp((tau_ref - dt) / tau_rc)
    kappa = 2.0 ** 20
    while kappa * (C1 - q) > 1.0:
        kappa *= 0.5
    a = F(1.0 / (kappa * E1))
    c = F(a + F(1.0))
    if float(c) < float(a) + 1.0:
        c = np.nextafter(c, F(np.inf))
    m1 = 1.0 + kappa * E1
    return {"kappa": kappa, "q": F(q), "nqm1": F(-q * m1), "E1": F(E1), "A": F(kappa * (C1 - q)), "nB": F(-kappa * C1 * E1), "na": F(-a),
            "c": c, "kq": F(kappa * q), "rkq": F(1.0 / (kappa * q)), "tau_rc": F(tau_rc), "rtau_rc": F(1.0 / tau_rc),
            "exact": {"q": q, "E1": E1, "C1": C1}}


def fma(x, y, z):
    return (np.asarray(x, np.float64) * np.asarray(y, np.float64) + np.asarray(z, np.float64)).astype(F)


def clamp(x):
    x = np.asarray(x, F)
    return np.where(np.isnan(x), F(0), np.minimum(np.maximum(x, F(0)), F(1))).astype(F)


BIG = F(2.0 ** 100)


def affine_step(w, JE, k):
    """One timestep on the loop words ``w`` with the pre-scaled input ``JE = E1 (J - 1)`` -> (w', spike indicator)."""
    with np.errstate(all="ignore"):
        W0 = clamp(w)
        dl = clamp(fma(w, k["na"], k["c"]))
        nmt = clamp(fma(w, k["q"], k["nqm1"]))
        t = fma(W0, k["E1"], JE)
        U = fma(t, dl, -W0)
        spk = clamp(U * BIG)
        rc = (F(1) / JE).astype(F)
        Wn = clamp(fma(spk, BIG, -U))
        u = (U * rc).astype(F)
        nu = clamp(fma(u, k["nB"], k["A"]))
        return fma(spk, nu, (Wn + nmt).astype(F)), spk


def word_in(s, k):
    """HBM word -> loop word (lif_word_in)."""
    rho = np.where(s < 0, -s, F(0)).astype(F)
    return np.where(s < 0, fma(k["kq"], np.expm1((rho * k["rtau_rc"]).astype(F)).astype(F), F(1)), (F(1) - s).astype(F)).astype(F)


def word_out(w, k):
    """loop word -> HBM word (lif_word_out)."""
    x = np.where(w > 1, ((w - F(1)).astype(F) * k["rkq"]).astype(F), F(0)).astype(F)
    return np.where(w > 1, -(k["tau_rc"] * np.log1p(x).astype(F)).astype(F), (F(1) - w).astype(F)).astype(F)


@functools.lru_cache(maxsize=None)
def case(tau_rc, tau_ref):
    """(open-loop model, inputs x [STEPS, K, 3] of the float64 oracle, float64 spike counts per neuron, the float64 run from reset
    with its propagated bound: V, R, bV, bR, marginal).  Computed once per constant set and left unchanged."""
    ol = L.open_loop_pathint(N, ssp_dim=7, neuron_type=nengo.LIF(tau_rc=tau_rc, tau_ref=tau_ref))
    ens = ol.ens
    o = OracleSimulator(ol.model)
    bias, enc = np.array(o.buf[ens["bias"]]), np.array(o.buf[ens["enc"]])
    V, R = np.zeros((ol.K, N)), np.zeros((ol.K, N))
    counts = np.zeros((ol.K, N), dtype=np.int64)
    X = np.zeros((STEPS, ol.K, 3))
    for t in range(STEPS):
        o.step()
        X[t] = o.sig[ens["x"]:ens["x"] + ol.K * 3].reshape(ol.K, 3)
        J = bias + np.einsum("kdn,kd->kn", enc, X[t])
        counts += lif_step(J, V, R, ol.dt, tau_rc, tau_ref, ens["neuron"]["min_voltage"])
    assert np.array_equal(V, o.buf[ens["v"]]) and np.array_equal(R, o.buf[ens["r"]])       # the oracle's own step, restated
    zero = np.zeros((ol.K, N))
    ref = L.restart_reference(ol, OracleSimulator(ol.model), zero, zero, STEPS)
    assert np.array_equal(ref[0], V)
    for arr in (X, counts, bias, enc) + tuple(ref):
        arr.setflags(write=False)
    return ol, X, counts, bias, enc, ref


def run_affine(ol, X, bias, enc, every_step, mutate=None):
    """The float32 restatement from reset -> (V, R as read back from the HBM words, spike counts per neuron)."""
    k = affine_constants(ol.dt, ol.tau_rc, ol.tau_ref)
    if mutate:
        k = mutate(dict(k))
    # inputs as the kernel holds them: bias registers (bias - 1) E1, encoder entries times E1 (each product rounded once)
    bE = ((bias.astype(F) - F(1)).astype(F) * k["E1"]).astype(F)
    eE = (enc.astype(F) * k["E1"]).astype(F)
    s = np.zeros((ol.K, N), F)
    w = word_in(s, k)
    counts = np.zeros((ol.K, N), dtype=np.int64)
    for t in range(X.shape[0]):
        x = X[t].astype(F)
        JE = bE
        for d in range(3):
            JE = fma(eE[:, d, :], x[:, d, None], JE)
        w, spk = affine_step(w, JE, k)
        assert np.isin(spk, (0, 1)).all() and np.isfinite(w).all() and (w >= 0).all() and (w <= 2).all()
        counts += spk.astype(np.int64)
        if every_step:
            w = word_in(word_out(w, k), k)
    s = word_out(w, k).astype(np.float64)
    return np.where(s >= 0, s, 0.0), np.where(s < 0, -s + ol.dt, 0.0), counts


def judge(ol, counts64, ref, V, R, counts):
    V_ref, R_ref, bV, bR, marginal = ref
    ok, info = L.compare_states(ol, V, R, V_ref, R_ref, bV, bR, marginal)
    diff = counts != counts64
    info["spikes_f64"] = int(counts64.sum())
    info["count_differences"] = int(diff.sum())
    info["count_differences_not_marginal"] = int((diff & ~marginal).sum())
    return ok and info["count_differences_not_marginal"] == 0, info


@pytest.mark.parametrize("every_step", [True, False], ids=["hbm-every-step", "hbm-never"])
@pytest.mark.parametrize("tau_rc,tau_ref", list(SETS))
def test_affine_step_against_the_float64_step(tau_rc, tau_ref, every_step):
    ol, X, counts64, bias, enc, ref = case(tau_rc, tau_ref)
    V, R, counts = run_affine(ol, X, bias, enc, every_step)
    ok, info = judge(ol, counts64, ref, V, R, counts)
    print("LIF(%g, %g) %s: %s" % (tau_rc, tau_ref, "HBM form every step" if every_step else "one launch", info))
    assert info["spikes_f64"] > 10 * ol.K * N
    assert ok, info


def _a_off(k):
    k["A"] = F(float(k["A"]) * (1.0 + 1e-4))
    return k


def _q_one(k):
    m1 = 1.0 + k["kappa"] * k["exact"]["E1"]
    k["q"], k["nqm1"] = F(1.0), F(-m1)
    return k


@pytest.mark.parametrize("mutate", [_a_off, _q_one], ids=["A-off-1e-4", "q-is-1"])
def test_mutants_fail(mutate):
    ol, X, counts64, bias, enc, ref = case(0.02, 0.002)
    V, R, counts = run_affine(ol, X, bias, enc, False, mutate=mutate)
    ok, info = judge(ol, counts64, ref, V, R, counts)
    print(mutate.__name__, info)
    assert not ok, info


@pytest.mark.parametrize("tau_rc,tau_ref", list(SETS) + [(0.02, 0.0137)])
def test_constants(tau_rc, tau_ref):
    """kappa is the largest power of two with kappa (C1 - q) <= 1; c - a >= 1 in exact arithmetic (a full step is exactly 1);
    the qualifying sets have kappa >= 4, LIF(0.02, 0.0137) has kappa 1 and stays on the per-timestep kernel."""
    k = affine_constants(0.001, tau_rc, tau_ref)
    e = k["exact"]
    kappa = k["kappa"]
    assert math.log2(kappa) == int(math.log2(kappa))
    assert kappa * (e["C1"] - e["q"]) <= 1.0 < 2 * kappa * (e["C1"] - e["q"])
    assert kappa == SETS.get((tau_rc, tau_ref), 1)
    assert (kappa >= 4) == ((tau_rc, tau_ref) in SETS)
    assert Fraction(float(k["c"])) + Fraction(float(k["na"])) >= 1
    assert float(k["c"]) - 1.0 + float(k["na"]) <= 2.0 ** -22 * float(k["c"])          # ... and no more than an ulp above it
    assert 0.0 < float(k["A"]) <= 1.0 and float(k["A"]) + float(k["nB"]) * 1.0 >= -1e-7      # nu of u = E1 (u' = 1): kappa (C1 q - q) >= 0
    # an integrating word (w <= 1) takes a full step, a word at the edge of the refractory range none
    w = np.array([0.0, 0.5, 1.0], F)
    assert (clamp(fma(w, k["na"], k["c"])) == 1).all()
    if tau_ref > 0.001:                                   # (C1 > 1: em = 1 - C1 < 0)
        assert clamp(fma(F(1.0) + k["A"], k["na"], k["c"])) == 0
