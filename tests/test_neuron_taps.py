"""Neuron probes on EnsembleArray members (``Probe(member.neurons[slice])``): the lowering - one tap per probed member on the
array operator, the hull of its probed slices - and the two float64 references the GPU tests of ``test_gpu_neuron_taps.py`` use:
``oracle.graphwalk`` samples the neuron output from the un-lowered network; the stepper's refractory state gives the spike mask
of a step (a neuron that spiked has ``R = tau_ref + t_spike > tau_ref``, every other one ``R <= tau_ref``).  The stepper itself is
frozen and does not know taps: its rows for such probes stay zero."""
import numpy as np
import pytest

import sspslam_amd.frontend as nengo
from sspslam_amd.builder import build
from oracle import OracleSimulator
from oracle.graphwalk import GraphWalkSimulator

from helpers import small_pathint


def _ens_ops(model):
    return [o for o in model.ops if o["kind"] == "ensarray"]


def _same(a, b):
    """Field-by-field equality of two operator fields (arrays by value)."""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape and np.array_equal(a, b)
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_reference_script_probes_build_and_leave_the_untapped_model_alone():
    """``run_pathint_gif.py``'s three probes - members 1, 2, 3, ``neurons[:500]``, every 100 steps - on (55, 600): one tap per
    probed member, 500 wide, inside ``core_to_post``; the same network without them lowers to what it lowered to before
    (operator list, signal layout and buffers compared field by field with a build that never saw a neuron probe)."""
    skip = 100
    pm = small_pathint(ssp_dim=55, n=600, T=2.0)
    plain = build(pm.model, n_eval_points=700)
    osc = pm.pathintegrator.oscillators
    with pm.model:
        ps = [nengo.Probe(osc.ea_ensembles[k].neurons[:500], synapse=None, sample_every=skip * 0.001) for k in (1, 2, 3)]
    tapped = build(pm.model, n_eval_points=700)
    (eo,) = _ens_ops(tapped)
    assert [(k, first, count) for k, first, count, _ in eo["taps"]] == [(1, 0, 500), (2, 0, 500), (3, 0, 500)]
    assert eo["tap_amp"] == 1.0 / tapped.dt
    c2p = tapped.stage_info["core_to_post"]
    by_probe = {id(p["probe"]): p for p in tapped.probes}
    for p, (k, first, count, dst) in zip(ps, eo["taps"]):
        assert any(lo <= dst and dst + count <= hi for lo, hi in c2p), (dst, count, c2p)
        bp = by_probe[id(p)]
        assert (bp["src"], bp["width"], bp["every"]) == (dst, 500, skip)
    assert eo["stage"] == 1
    # the tap signals are new; nothing else moved in front of them, and the untapped build is the parent's
    again = build(pm.model, probes=[pm.probe], n_eval_points=700)
    assert again.sig_size == plain.sig_size and tapped.sig_size == plain.sig_size + 3 * 500
    assert len(again.ops) == len(plain.ops) and len(again.buffers) == len(plain.buffers)
    for a, b in zip(again.ops, plain.ops):
        assert a.keys() == b.keys() and "taps" not in a
        for key in a:
            assert _same(a[key], b[key]), (a["kind"], key)
    for a, b in zip(again.buffers, plain.buffers):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    np.testing.assert_array_equal(again.sig_init, plain.sig_init)
    assert again.stage_info == plain.stage_info


def test_overlapping_slices_of_one_member_share_one_tap():
    pm = small_pathint(ssp_dim=7, n=64)
    osc = pm.pathintegrator.oscillators
    with pm.model:
        pa = nengo.Probe(osc.ea_ensembles[2].neurons[5:37])
        pb = nengo.Probe(osc.ea_ensembles[2].neurons[30:50], synapse=0.01)
        pc = nengo.Probe(osc.ea_ensembles[0].neurons)
    model = build(pm.model)
    (eo,) = _ens_ops(model)
    taps = {k: (first, count, dst) for k, first, count, dst in eo["taps"]}
    assert sorted(taps) == [0, 2] and taps[2][:2] == (5, 45) and taps[0][:2] == (0, 64)
    by_probe = {id(p["probe"]): p for p in model.probes}
    assert (by_probe[id(pa)]["src"], by_probe[id(pa)]["width"]) == (taps[2][2], 32)
    assert (by_probe[id(pc)]["src"], by_probe[id(pc)]["width"]) == (taps[0][2], 64)
    # the filtered probe samples a synapse state fed by its slice of the tap
    lows = [o for o in model.ops if o["kind"] == "lowpass" and o["dst"] <= by_probe[id(pb)]["src"] < o["dst"] + o["len"]]
    assert len(lows) == 1
    off = by_probe[id(pb)]["src"] - lows[0]["dst"]
    assert lows[0]["src"] + off == taps[2][2] + 25 and by_probe[id(pb)]["width"] == 20
    # taps are writes of the operator: disjoint from its decoded rows
    idx = set(np.asarray(model.buffers[eo["dst_idx"]]).reshape(-1).tolist())
    for first, count, dst in taps.values():
        assert not idx & set(range(dst, dst + count))


def test_sharded_builds_and_other_attributes_are_refused_by_name():
    pm = small_pathint(ssp_dim=7, n=64)
    osc = pm.pathintegrator.oscillators
    with pm.model:
        p = nengo.Probe(osc.ea_ensembles[1].neurons[:8])
    with pytest.raises(nengo.BuildError, match="shard"):
        build(pm.model, vco_shard=(0, 2), probes=[pm.probe, p])
    with pytest.raises(nengo.BuildError, match="shard"):
        build(pm.model, neuron_shard=(0, 2), probes=[pm.probe, p])
    with pm.model:
        pv = nengo.Probe(osc.ea_ensembles[1].neurons[:8], "voltage")
    with pytest.raises(nengo.BuildError, match="voltage"):
        build(pm.model, probes=[pm.probe, pv])


@pytest.mark.parametrize("ssp_dim,n,spikes", [(7, 64, 7430), (55, 60, 54989)])
def test_the_two_references_agree_exactly(ssp_dim, n, spikes):
    """Graph walk against the stepper's refractory state over 400 closed-loop steps, all neurons of every member: the same spikes,
    no mismatch - so exact equality is a condition the GPU tests may set (``spikes``: the count among the first 50 neurons of
    every member, the figure the feature's description records).  The stepper's own rows for the taps stay zero."""
    steps = 400
    pm = small_pathint(ssp_dim=ssp_dim, n=n, T=10.0, limit=0.2)
    osc = pm.pathintegrator.oscillators
    with pm.model:
        ps = [nengo.Probe(e.neurons, synapse=None) for e in osc.ea_ensembles]
    model = build(pm.model)
    (eo,) = _ens_ops(model)
    walk = GraphWalkSimulator(pm.model, model)
    ref = OracleSimulator(model)
    masks = []
    for _ in range(steps):
        ref.step()
        walk.step()
        masks.append(ref.buf[eo["r"]] > eo["neuron"]["tau_ref"])
    masks = np.array(masks)                                  # [steps, K, n]
    total = 0
    for k, p in enumerate(ps):
        w = walk.probe_data(p)
        assert w.shape == (steps, n)
        np.testing.assert_array_equal(w, masks[:, k] * eo["tap_amp"])
        total += int((w[:, :50] != 0).sum())
        i = [j for j, q in enumerate(model.probes) if q["probe"] is p][0]
        assert not ref.probe_data(i).any()
    assert total == spikes
