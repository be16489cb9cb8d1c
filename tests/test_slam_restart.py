"""The one-step restart instrument (tests/slam_restart.py) on the CPU: the NumPy f32 oracle as the device passes, its bounds are
tight, and every wrong device fails.  The GPU file (tests/test_gpu_slam_restart.py) drives the same code with the kernels."""
import types

import numpy as np
import pytest

import slam_restart as R

POINTS = (60, 64, 100, 127, 150, 200, 250, 300, 320, 350, 380, 399)
CLOSED, OPEN = 127, 200                                                   # the gate is closed at the first, open at the second


@pytest.fixture(scope="module")
def model():
    return R.small_slam()[1]


@pytest.fixture(scope="module")
def passing(model):
    dev = R.OracleDevice(model)
    reports = []
    for p in POINTS:
        dev.run_steps(p - dev.n_steps)
        reports.append(R.check_restart_step(model, dev))
    return reports


def op_of(model, kind, **match):
    found = [(j, o) for j, o in enumerate(model.ops) if o["kind"] == kind and all(o.get(k) == v for k, v in match.items())]
    assert found, (kind, match)
    return found[0]


def test_carried_set_of_a_three_operator_model():
    """table -> [0, 2); axpy copies it to [2, 4), which the low-pass filter reads in the same step (dead at its end); the filter's own
    state [4, 6) is read before it is rewritten: carried.  The state buffer is included, the parameter buffer is not."""
    m = types.SimpleNamespace(sig_size=8, probes=[], buffers=[np.zeros(3), np.zeros(3)],
                              buffer_meta=[dict(name="w", role="param"), dict(name="v", role="state")],
                              ops=[dict(kind="table", dst=0, width=2, table=0),
                                   dict(kind="axpy", dst=2, src=0, len=2, alpha=0.5, mode="set"),
                                   dict(kind="lowpass", dst=4, src=2, len=2, a=0.9, gain=1.0)])
    c = R.carried(m)
    assert c.signals == [(4, 6)] and c.buffers == [1] and c.probes == []
    assert not c.mask[2:4].any() and not c.mask[0:2].any() and c.mask[4:6].all() and not c.mask[6:].any()
    assert list(c.writer[:6]) == [0, 0, 1, 1, 2, 2]
    m.probes = [dict(src=2, width=2, every=1, probe=None)]           # a probe makes the intermediate part of the comparison
    c = R.carried(m)
    assert c.probes == [(2, 4)] and c.mask[2:4].all() and c.signals == [(4, 6)]


def test_the_small_slam_carries_filters_states_and_the_decision_probes(model):
    c = R.carried(model)
    kinds = {model.ops[j]["kind"] for j in np.unique(c.writer[c.mask])}
    assert {"lowpass", "cleanup", "gate"} <= kinds
    roles = {model.buffer_meta[i]["role"] for i in c.buffers}
    assert roles == {"state", "learned"} and len(c.buffers) == 20
    dead = [o for o in model.ops if o["kind"] == "neurons"][0]        # spikes are consumed inside the step
    assert not c.mask[dead["out"]:dead["out"] + dead["n"]].any()


def test_numpy_f32_device_passes_with_learning_and_the_gate_live(passing):
    s = R.summarize(passing, max_skips=0)
    print(R.describe(s, "NumPy f32"))
    assert s["ok"] and s["skipped"] == 0 and not s["failures"], R.describe(s)
    assert s["worst"] <= 1.0
    assert s["live"]["pes"] == len(POINTS) and s["live"]["voja"] == len(POINTS) and s["live"]["pes_inc"] > 0 and s["live"]["voja_rows"] > 0
    by_step = {r["step"] - 1: r for r in passing}
    assert by_step[OPEN]["live"]["gate_open"] and not by_step[CLOSED]["live"]["gate_open"]
    assert {"lowpass", "neurons", "ensarray", "pes", "voja", "gate", "cleanup"} <= set(s["kind"])


def test_bounds_are_tight(passing):
    """bound / |NumPy f32 - float64|, median over the compared elements the f32 run did not get exactly, per operator kind: at most 64
    (the clean-up's region holds table rows: either equal or a decision)."""
    s = R.summarize(passing)
    print("tightness", s["tightness"])
    assert set(s["tightness"]) >= {"lowpass", "neurons", "ensarray", "pes", "voja", "gate"}
    for kind, t in s["tightness"].items():
        assert t <= 64.0, (kind, t, s["tightness"])


# ---- mutants: every wrong device fails ---------------------------------------------------------------------------------------
def run_mutant(model, wrap=None, after_step=None, points=(CLOSED, OPEN)):
    dev = R.OracleDevice(model, wrap=wrap, after_step=after_step)
    return R.run_points(model, dev, points)


def altered(**kw):
    return lambda dev, o, apply: apply(dict(o, **kw))


def mutants(model):
    jp, pes = op_of(model, "pes")
    jv, voja = op_of(model, "voja")
    jg, gate = op_of(model, "gate")
    jc, cl = op_of(model, "cleanup")
    jl, lp = op_of(model, "lowpass", dst=model.probes[0]["src"])
    jm, mv = [(j, o) for j, o in enumerate(model.ops) if o["kind"] == "matvec" and o["mode"] == "set" and not o.get("dft") and o["stage"] == 1][0]
    je, ens = op_of(model, "ensarray", label="pathint_vco")
    err_copy = [o for o in model.ops if o["kind"] == "axpy" and o["mode"] == "set" and o["dst"] == pes["err"] and o["len"] == pes["rows"]][0]
    out = {}
    out["pes kappa x (1 + 2e-3)"] = {jp: altered(kappa=pes["kappa"] * (1 + 2e-3))}

    def pes_ragged(dev, o, apply):
        lo = (o["rows"] - 1) // 32 * 32
        keep = dev.o.buf[o["w"]][lo:].copy()
        apply(o)
        dev.o.buf[o["w"]][lo:] = keep
    assert pes["rows"] % 32
    out["pes ragged last 32-row block untouched"] = {jp: pes_ragged}

    def with_signal(offset_of, value_of):
        def fn(dev, o, apply):
            sl = slice(offset_of(o), offset_of(o) + len(value_of(dev, o)))
            keep = dev.o.sig[sl].copy()
            dev.o.sig[sl] = value_of(dev, o)
            apply(o)
            dev.o.sig[sl] = keep
        return fn
    out["pes previous step's act"] = {jp: with_signal(lambda o: o["act"], lambda dev, o: dev.start[0][o["act"]:o["act"] + o["cols"]])}
    out["pes error filter advanced before the update"] = {jp: with_signal(lambda o: o["err"], lambda dev, o: dev.o.sig[err_copy["src"]:err_copy["src"] + o["rows"]].copy())}

    def voja_no_decay(dev, o, apply):
        E0 = dev.o.buf[o["w"]].copy()
        a = dev.o.sig[o["spk"]:o["spk"] + o["rows"]]
        apply(o)
        dev.o.buf[o["w"]] += (o["lr_dt"] * (1.0 + dev.o.sig[o["learn"]]) * a[:, None] * E0).astype(E0.dtype)
    out["voja without - a E"] = {jv: voja_no_decay}

    def voja_scale_shift(dev, o, apply):
        sc = dev.o.buf[o["scale_buf"]]
        keep = sc.copy()
        sc[:] = np.roll(keep, -1)
        apply(o)
        sc[:] = keep
    out["voja scale of row i + 1"] = {jv: voja_scale_shift}

    def voja_silent(dev, o, apply):
        a = dev.o.sig[o["spk"]:o["spk"] + o["rows"]]
        row = int(np.flatnonzero(a == 0)[0])
        apply(o)
        E = dev.o.buf[o["w"]]
        E[row] -= (o["lr_dt"] * 1000.0 * E[row]).astype(E.dtype)
    out["voja silent row touched"] = {jv: voja_silent}
    out["lowpass a x (1 + 1e-4)"] = {jl: altered(a=lp["a"] * (1 + 1e-4))}

    def matvec_short(dev, o, apply):
        W = dev.o.buf[o["w"]]
        keep = W[:, -1].copy()
        W[:, -1] = 0
        apply(o)
        W[:, -1] = keep
    out["matvec last column dropped"] = {jm: matvec_short}

    def ens_swap(dev, o, apply):
        D = dev.o.buf[o["dec"]]
        D[[3, 4]] = D[[4, 3]]
        apply(o)
        D[[3, 4]] = D[[4, 3]]
    out["ensarray decoders of members 3 and 4 swapped"] = {je: ens_swap}
    out["LIF tau_ref + dt"] = {je: altered(neuron=dict(ens["neuron"], tau_ref=ens["neuron"]["tau_ref"] + model.dt))}

    def cleanup_neighbour(dev, o, apply):
        apply(o)
        T = dev.o.buf[o["w"]]
        row = dev.o.sig[o["dst"]:o["dst"] + o["cols"]]
        k = int(np.argmax(T @ row))
        dev.o.sig[o["dst"]:o["dst"] + o["cols"]] = T[k + 1 if k + 1 < T.shape[0] else k - 1]
    out["cleanup neighbouring grid row"] = {jc: cleanup_neighbour}
    out["gate rate x 1.001"] = {jg: altered(rate=gate["rate"] * 1.001)}

    def gate_always(dev, o, apply):
        x = dev.o.sig[o["src"]:o["src"] + 2 * o["d"] + 1]
        dev.o.sig[o["dst"]:o["dst"] + o["d"]] = o["rate"] * (x[:o["d"]] - x[o["d"]:2 * o["d"]])
    out["gate opens below the threshold"] = {jg: gate_always}
    return out


MUTANTS = ["pes kappa x (1 + 2e-3)", "pes ragged last 32-row block untouched", "pes previous step's act",
           "pes error filter advanced before the update", "voja without - a E", "voja scale of row i + 1", "voja silent row touched",
           "lowpass a x (1 + 1e-4)", "matvec last column dropped", "ensarray decoders of members 3 and 4 swapped", "LIF tau_ref + dt",
           "cleanup neighbouring grid row", "gate rate x 1.001", "gate opens below the threshold"]


@pytest.mark.parametrize("name", MUTANTS)
def test_mutant_fails(model, passing, name):
    by_step = {r["step"] - 1: r for r in passing}
    for p in (CLOSED, OPEN):                   # the points are decided ones: nothing marginal that could turn a failure into a skip
        assert not any(by_step[p]["marginal"].values()) and not by_step[p]["skipped"]
    s = run_mutant(model, wrap=mutants(model)[name])
    print(name, R.describe(s))
    assert not s["ok"] and s["skipped"] == 0, (name, R.describe(s))
    assert s["failures"] or s["worst"] > 1.0


def test_mutant_carried_signal_left_at_its_previous_value_fails(model):
    lo = model.probes[0]["src"]
    hi = lo + model.probes[0]["width"]

    def stale(dev):
        dev.o.sig[lo:hi] = dev.start[1][lo:hi]
    s = run_mutant(model, after_step=stale)
    assert not s["ok"] and s["skipped"] == 0 and s["region"]["sig %d:%d lowpass" % (lo, hi)] > 1.0, R.describe(s)


def test_mutation_list_is_complete(model):
    assert sorted(mutants(model)) == sorted(MUTANTS) and len(MUTANTS) + 1 == 15


# ---- masks: a marginal decision that flips is a skip, a second one fails -----------------------------------------------------------
def flipping_device(model, make_marginal=True):
    """A stand-in and a function that, at the current step, puts one neuron of the first ``neurons`` population (within f32 rounding)
    ON the threshold - marginal by construction - and makes the device decide it the other way than float64 does."""
    j, o = op_of(model, "neurons")
    chosen = {}

    def flip(dev, op, apply):
        apply(op)
        if "i" not in chosen:
            return
        i, V, Rr = chosen.pop("i"), dev.o.buf[op["v"]], dev.o.buf[op["r"]]
        V[i], Rr[i] = (0.99, 0.0) if chosen.pop("spikes_in_float64") else (0.0, op["neuron"]["tau_ref"] + 0.5 * model.dt)
    dev = R.OracleDevice(model, wrap={j: flip})

    def arm():
        ref = R.fork_from_device(model, dev)
        lif = R.bounded_step(model, ref).lif[o["v"]]
        R0 = R.canonical_R(dev.read_buffer(o["r"]), model.dt)
        em = -np.expm1(-model.dt / o["neuron"]["tau_rc"])
        cand = np.where((R0 == 0) & ~lif["spiked"] & (lif["J"] > 1.5), lif["Vt"], -np.inf)
        i = int(np.argmax(cand))
        assert np.isfinite(cand[i])
        if make_marginal:
            V = dev.read_buffer(o["v"])
            V[i] = (1.0 - 1e-9 - lif["J"][i] * em) / (1.0 - em)
            dev.write_buffer(o["v"], V)
        V0 = dev.read_buffer(o["v"])[i]                       # (as the device holds it: rounded to f32)
        chosen["i"], chosen["spikes_in_float64"] = i, bool(V0 + (lif["J"][i] - V0) * em > 1)
    return dev, arm


def test_a_marginal_decision_that_flips_is_a_skip_and_a_second_one_fails(model):
    dev, arm = flipping_device(model)
    reports = []
    for p in (CLOSED, OPEN):
        dev.run_steps(p - dev.n_steps)
        arm()
        reports.append(R.check_restart_step(model, dev))
        assert reports[-1]["skipped"] and not reports[-1]["failures"] and reports[-1]["marginal"]["neurons"] >= 1, reports[-1]["skip_reasons"]
    one, two = R.summarize(reports[:1]), R.summarize(reports)
    assert one["ok"] and one["skipped"] == 1
    assert not two["ok"] and two["skipped"] == 2 and not two["failures"]


def test_a_flip_of_a_neuron_that_is_not_marginal_fails(model):
    dev, arm = flipping_device(model, make_marginal=False)
    dev.run_steps(CLOSED)
    arm()
    r = R.check_restart_step(model, dev)
    assert r["failures"] and not r["skipped"] and not r["ok"], r


def test_a_flip_upstream_of_a_marginal_one_still_fails(model):
    """A skipped point keeps the decisions it can judge: a neuron of the oscillator array (an operator BEFORE the population with
    the marginal flip) that is not marginal and lands on the other side is a failure, skip or not; what differs behind the
    marginal flip is not."""
    je, ens = op_of(model, "ensarray", label="pathint_vco")
    jn, _ = op_of(model, "neurons")
    assert je < jn

    def spike_one(dev, o, apply):
        V0 = dev.o.buf[o["v"]].copy()
        apply(o)
        if dev.n_steps != CLOSED + 1:          # (only in the checked step)
            return
        V, Rr = dev.o.buf[o["v"]], dev.o.buf[o["r"]]
        k, i = np.argwhere((V0 > 0.2) & (V0 < 0.6) & (V > 0) & (V < 0.7))[0]          # integrating, far below the threshold
        V[k, i], Rr[k, i] = 0.0, o["neuron"]["tau_ref"] + 0.5 * model.dt
    dev, arm = flipping_device(model)
    dev.wrap[je] = spike_one
    dev.run_steps(CLOSED)
    arm()
    r = R.check_restart_step(model, dev)
    assert r["skipped"] and len(r["failures"]) == 1 and "op v=%d" % ens["v"] in r["failures"][0] and not r["ok"], r
    assert not R.summarize([r])["ok"]
