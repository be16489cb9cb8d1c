"""Parity tests proper (run with -m gpu on an MI355X): the HIP path, called through the C ABI, against
the NumPy oracle on the same built model and the same seeded inputs.

Bars: f64 (parity mode) - 1e-9 absolute on the probe trajectory (observed ~1e-16: same operation order,
-ffp-contract=off); f32 (fast mode) - 1e-3 cosine error, the tolerance BASELINE.json's north_star states,
on windows short enough that spike-level chaos has not amplified the rounding difference."""
import os

import numpy as np
import pytest

import sspslam_amd.frontend as nengo
from sspslam_amd import harness as H
from sspslam_amd import simulator as PLAN
from sspslam_amd.modelcache import cached_build as build      # (one build per model and session: conftest.py gives the suite a cache)
from oracle import OracleSimulator

from helpers import small_pathint

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def Simulator():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from sspslam_amd.simulator import Simulator
    return Simulator


def run_pair(Simulator, model, probe, steps, dtype, **kw):
    ref = OracleSimulator(model)
    ref.run_steps(steps)
    with Simulator(None, model=model, dtype=dtype, **kw) as sim:
        sim.run_steps(steps)
        got = sim.data[probe]
        counters = sim.counters()
    return got, ref.probe_data(0), counters


@pytest.mark.parametrize("ssp_dim,n", [(7, 64), (55, 500), (97, 130), (55, 1030), (1015, 70)])
def test_pathint_f64_matches_oracle(Simulator, ssp_dim, n):
    """cfg1 (ssp_dim=55, n=500), ragged sizes (n not a multiple of the vector width / workgroup chunk) and the
    benchmark's dimension (ssp_dim=1015: 508 VCOs, 1524 x 1015 read-in / read-out products) with few neurons per VCO."""
    pm = small_pathint(ssp_dim=ssp_dim, n=n, T=10.0, limit=0.2)
    model = build(pm.model)
    got, want, c = run_pair(Simulator, model, pm.probe, 400, "f64")
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, atol=1e-9, rtol=0)
    assert c["n_steps"] == 400 and c["launches_per_step"] <= 8


@pytest.mark.parametrize("ssp_dim,n", [(55, 500), (1015, 70)])
def test_pathint_f32_within_cosine_bar(Simulator, ssp_dim, n):
    pm = small_pathint(ssp_dim=ssp_dim, n=n, T=10.0, limit=0.2)
    model = build(pm.model)
    got, want, _ = run_pair(Simulator, model, pm.probe, 400, "f32")
    ce = H.cosine_error(got[20:], want[20:])
    assert ce.max() < 1e-3, ce.max()


def test_pathint_blocks_after_the_init_window_skip_the_zero_input_product(Simulator, monkeypatch):
    """The init-SSP input of the path integrator is zero from t = 50 ms on (reference run_pathint.py:136): in every block of
    timesteps that lies behind it the time-batched `to_Fourier` product has an all-zero input and is not multiplied out
    (run_batch's zero tracking, ssn_host.hip).  64-step blocks put four of five blocks behind the window: f64 against the
    oracle, and bit-equal to a run with the tracking switched off."""
    pm = small_pathint(ssp_dim=55, n=70, T=10.0, limit=0.2)
    model = build(pm.model)
    ref = OracleSimulator(model)
    ref.run_steps(320)
    outs = {}
    for skip in (True, False):
        if skip:
            monkeypatch.delenv("SSN_NO_ZERO_SKIP", raising=False)
        else:
            monkeypatch.setenv("SSN_NO_ZERO_SKIP", "1")
        with Simulator(None, model=model, dtype="f64", block_steps=64) as sim:
            sim.run_steps(200)
            sim.run_steps(120)
            outs[skip] = np.array(sim.data[pm.probe])
            assert sim.counters()["batch_products_skipped"] == (5 if skip else 0)       # blocks of 64, 64, 64, 8 | 64, 56 steps: all but the first lie behind t = 50 ms
    np.testing.assert_allclose(outs[True], ref.probe_data(0), atol=1e-9, rtol=0)
    np.testing.assert_array_equal(outs[True], outs[False])
    monkeypatch.delenv("SSN_NO_ZERO_SKIP", raising=False)
    with Simulator(None, model=model, dtype="f32", block_steps=64) as sim:
        sim.run_steps(320)
        assert H.cosine_error(np.array(sim.data[pm.probe])[20:], ref.probe_data(0)[20:]).max() < 1e-3


@pytest.mark.parametrize("shape", ["n=50000", "d=4033", "n=12000"])
def test_pathint_shapes_of_the_large_configurations(Simulator, shape):
    """Ensembles too large for the whole-block kernel (BASELINE config 4: 50 000 neurons per VCO - the per-timestep
    k_ensarray over 49 chunks of 1024 neurons; 12 000: just above the block kernel's 10 240) and config 4's dimension
    d = 4033 (2017 VCOs, n_scales 28 x n_rotates 24) with few neurons: f64 against the oracle, f32 within the cosine bar."""
    space, n, m_eval = {"n=50000": (H.make_ssp_space(2, 7), 50000, 1500),
                        "d=4033": (H.make_ssp_space(2, n_scales=28, n_rotates=24), 40, None),
                        "n=12000": (H.make_ssp_space(2, 55), 12000, 1500)}[shape]
    assert space.ssp_dim == {"n=50000": 7, "d=4033": 4033, "n=12000": 55}[shape]
    path, vels = H.make_random_path(20.0, limit=0.1, seed=0)
    pm = H.make_pathint_model(space, path, vels, n)
    model = build(pm.model, n_eval_points=m_eval)
    ref = OracleSimulator(model)
    ref.run_steps(150)
    want = ref.probe_data(0)
    for dtype in ("f64", "f32"):
        with Simulator(None, model=model, dtype=dtype) as sim:
            sim.run_steps(150)
            got = sim.data[pm.probe]
            assert sim.counters()["launches_per_step"] == (0 if shape == "d=4033" else 1)
        if dtype == "f64":
            np.testing.assert_allclose(got, want, atol=1e-9, rtol=0)
        else:
            assert H.cosine_error(got[20:], want[20:]).max() < 1e-3


def test_steps_per_graph_and_chunked_runs_are_equivalent(Simulator):
    """Graph replay (16 steps), eager remainder, profile mode and step-by-step runs give identical results - on the default
    plan, with one k_ensarray per timestep and on the generic item plan, each plain, with the dominant kernel timed
    (profile 1) and with every launch timed (profile 2)."""
    pm = small_pathint(ssp_dim=55, n=100, T=10.0, limit=0.2)
    model = build(pm.model)
    outs = []
    for spg, chunks, profile in ((16, [100], False), (1, [100], False), (7, [33, 1, 66], False), (16, [50, 50], True)):
        with Simulator(None, model=model, dtype="f64", steps_per_graph=spg) as sim:
            for c in chunks:
                sim.run_steps(c, profile=profile)
            outs.append(sim.data[pm.probe])
            assert sim.n_steps == 100 and np.allclose(sim.trange(), 0.001 * np.arange(1, 101))
    for o in outs[1:]:
        np.testing.assert_array_equal(o, outs[0])
    # every way run_steps walks a block, per plan (whole-block kernel / one k_ensarray per timestep / generic items) and per
    # profile mode: blocks of 25, 25 | 25, 5 | 20 timesteps, with graph replays of 16 and eager remainders inside them.
    # The whole-block kernel adds an ensemble's spike sums in another (fixed) order than the per-timestep kernels
    # (test_fused_recurrent_core_equals_generic_path): its runs are bit-equal to the runs above, which use it too; the other
    # two plans are bit-equal to each other and within 1e-13 of it - sums of 100 terms of magnitude <= 1 in another order
    # differ by a few units of 2.2e-16, fed back over 100 timesteps (observed: 1.1e-16).
    NO_BLOCK, NO_FUSED = PLAN.SSN_PLAN_NO_BLOCK_KERNEL, PLAN.SSN_PLAN_NO_FUSED_CORE
    runs = {}
    for flags in (0, NO_BLOCK, NO_FUSED):
        for profile in (0, 1, 2):
            with Simulator(None, model=model, dtype="f64", steps_per_graph=16, block_steps=25, flags=flags) as sim:
                for c in (50, 30, 20):
                    sim.run_steps(c, profile=profile)
                assert sim.n_steps == 100
                runs[flags, profile] = (np.array(sim.data[pm.probe]), sim.counters()["dominant_launches"],
                                        {k: v[0] for k, v in sim.kernel_times().items()})
    for (flags, profile), (out, _, _) in runs.items():
        np.testing.assert_array_equal(out, outs[0] if flags == 0 else runs[NO_BLOCK, 0][0], err_msg=f"flags {flags} profile {profile}")
        np.testing.assert_allclose(out, outs[0], atol=1e-13, rtol=0, err_msg=f"flags {flags} profile {profile}")
    assert runs[0, 1][1] == 3, runs[0, 1][1:]                        # the block launch is timed where the block is a whole one
    assert runs[NO_BLOCK, 1][1] == 100, runs[NO_BLOCK, 1][1:]
    assert runs[NO_BLOCK, 2][2] == {"k_ensarray": 100}, runs[NO_BLOCK, 2][1:]


def test_reset_and_state_access(Simulator):
    pm = small_pathint(ssp_dim=7, n=64, T=10.0, limit=0.2)
    model = build(pm.model)
    ens = next(o for o in model.ops if o["kind"] == "ensarray")
    with Simulator(None, model=model, dtype="f64") as sim:
        sim.run_steps(50)
        a = sim.data[pm.probe].copy()
        v = sim.read_buffer(ens["v"])
        assert v.shape == (4, 64) and v.max() > 0
        np.testing.assert_array_equal(sim.read_buffer(ens["enc"]), model.buffers[ens["enc"]])
        sim.reset()
        assert sim.n_steps == 0 and np.all(sim.read_buffer(ens["v"]) == 0)
        sim.run_steps(50)
        np.testing.assert_array_equal(sim.data[pm.probe], a)
        sig = sim.read_signal(0, model.sig_size)
        sim.write_signal(3, np.array([1.5, -2.5]))
        np.testing.assert_array_equal(sim.read_signal(3, 2), [1.5, -2.5])
        assert sig.shape == (model.sig_size,)
    built = sim.data[pm.pathintegrator.oscillators.ea_ensembles[1]]
    assert built.gain.shape == (64,) and built.scaled_encoders.shape == (64, 3)


def test_neuron_types_and_dense_ensembles(Simulator):
    """Dense (non-array) ensembles: encoder matvec + neuron kernel + decoder matvec, all three neuron types."""
    for nt in (nengo.LIF(), nengo.LIFRate(), nengo.RectifiedLinear()):
        with nengo.Network(seed=4) as m:
            u = nengo.Node(lambda t: [np.sin(8 * t), 0.5])
            e = nengo.Ensemble(300, 2, neuron_type=nt)
            o = nengo.Node(size_in=2)
            nengo.Connection(u, e, synapse=None)
            nengo.Connection(e, o, synapse=0.01, function=lambda x: [x[0] * x[1], x[0]])
            p = nengo.Probe(o, synapse=0.02)
            ps = nengo.Probe(e.neurons[:5])
        model = build(m)
        ref = OracleSimulator(model)
        ref.run_steps(300)
        with Simulator(None, model=model, dtype="f64") as sim:
            sim.run_steps(300)
            np.testing.assert_allclose(sim.data[p], ref.probe_data(0), atol=1e-9)
            np.testing.assert_allclose(sim.data[ps], ref.probe_data(1), atol=1e-9)


def test_encoder_product_with_the_neuron_update_in_its_epilogue(Simulator):
    """Round plan: where a dense population's encoder product is the last writer of its current vector and nothing else reads
    that vector, the workgroup that owns 16 rows of the product steps their 16 neurons and leaves their spikes as a 16-neuron
    segment of the spike list (matvec_neurons_body; by default for populations of more than 4096 neurons, here forced for small
    ones).  Sizes that leave a partial last workgroup and a partial wave, an input wider than one 16-byte vector per lane with
    a scalar tail, all three neuron types, a second decoded connection through the same spike list: f64 equal to the oracle and
    bit-equal to the unfused plan, f32 equal to the unfused plan up to the rounding of another summation order."""
    saved = {k: os.environ.get(k) for k in ("SSN_FUSE_MIN_ROWS", "SSN_FUSE_NEURONS")}
    try:
        # (an input of at most 16 dimensions makes the encoder product a glue micro-operator: nothing to fuse with)
        for nt, n, d in ((nengo.LIF(), 1003, 19), (nengo.LIF(), 330, 67), (nengo.LIFRate(), 300, 17), (nengo.RectifiedLinear(), 77, 18)):
            with nengo.Network(seed=4) as m:
                u = nengo.Node(lambda t, d=d: np.sin(8 * t + np.arange(d)) * 0.8)
                a = nengo.Ensemble(200, d)                 # (a tabulated input's encoder product runs time-batched: the fused
                e = nengo.Ensemble(n, d, neuron_type=nt)   #  population takes its input from another population's filtered output)
                o = nengo.Node(size_in=2)
                o2 = nengo.Node(size_in=1)
                nengo.Connection(u, a, synapse=None)
                nengo.Connection(a, e, synapse=0.01)
                nengo.Connection(e, o, synapse=0.01, function=lambda x: [x[0] * x[1], x[0]])
                nengo.Connection(e, o2, synapse=0.005, function=lambda x: x[0] ** 2)
                p = nengo.Probe(o, synapse=0.02)
                p2 = nengo.Probe(o2)
                ps = nengo.Probe(e.neurons[:5])
            model = build(m)
            ref = OracleSimulator(model)
            ref.run_steps(300)
            outs = {}
            for dtype in ("f64", "f32"):
                for fused in (True, False):
                    os.environ["SSN_FUSE_MIN_ROWS"] = "1"
                    os.environ["SSN_FUSE_NEURONS"] = "1" if fused else "0"
                    with Simulator(None, model=model, dtype=dtype) as sim:
                        assert sim.counters()["fused_populations"] == (1 if fused else 0), (nt, n, d, dtype)
                        sim.run_steps(300)
                        outs[dtype, fused] = (sim.data[p], sim.data[p2], sim.data[ps])
            for q in range(3):
                np.testing.assert_allclose(outs["f64", True][q], ref.probe_data(q), atol=1e-9, err_msg=f"{nt} {n} {d} probe {q}")
                np.testing.assert_array_equal(outs["f64", True][q], outs["f64", False][q], err_msg=f"{nt} {n} {d} probe {q}")
                # (f32: below 4097 rows the unfused product is the one-row-per-wave variant, which adds a row's terms in another
                #  order - rounding only; from 4097 rows on both are the four-rows-per-wave order and config 3 is bit-equal)
                np.testing.assert_allclose(outs["f32", True][q], outs["f32", False][q], atol=1e-5 * max(1.0, np.abs(outs["f32", False][q]).max()),
                                           err_msg=f"{nt} {n} {d} probe {q}")
            assert np.abs(outs["f32", True][0]).max() > 0.01
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.mark.parametrize("neuron_type,n", [("LIFRate", 13000), ("LIF", 16000)])
def test_dense_product_over_a_long_activity_vector(Simulator, neuron_type, n):
    """A learned (PES) decoder product over more activities than k_matvec's 48 KB LDS stage holds (12 288 f32 /
    6 144 f64).  Rate neurons: dense product, the source vector goes through the stage in slabs, and the two-row
    product leaves three of the workgroup's four waves without rows (they still join the slab barriers).  Spiking
    neurons: the spike-sparse product over neuron-major weights with segmented spike lists (no size limit)."""
    with nengo.Network(seed=1) as m:
        u = nengo.Node(lambda t: [np.sin(6 * t), np.cos(6 * t)])
        pre = nengo.Ensemble(n, 2, neuron_type=getattr(nengo, neuron_type)())
        post = nengo.Node(size_in=2)
        err = nengo.Node(size_in=2)
        nengo.Connection(u, pre, synapse=None)
        c = nengo.Connection(pre, post, function=lambda x: [0.0, 0.0], learning_rule_type=nengo.PES(2e-4), synapse=0.005)
        nengo.Connection(post, err, synapse=None)
        nengo.Connection(u, err, transform=-1, synapse=None)
        nengo.Connection(err, c.learning_rule, synapse=None)
        p = nengo.Probe(post, synapse=0.01)
    model = build(m)
    assert any(o["kind"] == "matvec" and o["cols"] == n for o in model.ops)
    ref = OracleSimulator(model)
    ref.run_steps(150)
    want = ref.probe_data(0)
    assert np.abs(want).max() > 0.3                                   # the rule has learned to follow the input
    with Simulator(None, model=model, dtype="f64") as sim:
        sim.run_steps(150)
        np.testing.assert_allclose(sim.data[p], want, atol=1e-9, rtol=0)
    with Simulator(None, model=model, dtype="f32") as sim:
        sim.run_steps(150)
        np.testing.assert_allclose(sim.data[p], want, atol=2e-3, rtol=0)


def test_dense_neuron_to_neuron_weights_wider_than_the_lds_stage(Simulator):
    """A 4200 x 6200 weight matrix between the neurons of two ensembles (rate neurons in front: a dense product): in f64 the
    6200-element source is wider than k_matvec's LDS stage (6144 doubles) and the matrix is tall enough for four rows per
    wave - the slab-staged variant of the tall-matrix kernel; f32 takes the one-stage kernel."""
    W = np.random.RandomState(0).randn(4200, 6200) * 2e-4
    with nengo.Network(seed=2) as m:
        u = nengo.Node(lambda t: [np.sin(5 * t), np.cos(3 * t)])
        a = nengo.Ensemble(6200, 2, neuron_type=nengo.LIFRate())
        b = nengo.Ensemble(4200, 2)
        nengo.Connection(u, a, synapse=None)
        nengo.Connection(a.neurons, b.neurons, transform=W, synapse=0.005)
        o = nengo.Node(size_in=2)
        nengo.Connection(b, o, synapse=0.01)
        p_spikes, p_out = nengo.Probe(b.neurons[:8]), nengo.Probe(o)
    model = build(m)
    assert any(x["kind"] == "matvec" and (x["rows"], x["cols"], x["stage"]) == (4200, 6200, 1) for x in model.ops)
    ref = OracleSimulator(model)
    ref.run_steps(80)
    with Simulator(None, model=model, dtype="f64") as sim:
        sim.run_steps(80)
        np.testing.assert_array_equal(sim.data[p_spikes], ref.probe_data(0))
        np.testing.assert_allclose(sim.data[p_out], ref.probe_data(1), atol=1e-9, rtol=0)
    with Simulator(None, model=model, dtype="f32") as sim:
        sim.run_steps(80)
        assert np.abs(sim.data[p_out] - ref.probe_data(1)).max() < 0.02 * np.abs(ref.probe_data(1)).max() + 1e-4


def test_config2_size_properties(Simulator):
    """BASELINE config 2 size (508 VCOs x 10 000 neurons) with cheap random decoders: the oracle cannot
    keep up at this size, so check size-independent properties - determinism across graph/eager paths,
    VCO independence (zeroing one VCO's decoders changes only its own outputs) and conservation of the
    DC oscillator."""
    K, n = 508, 10000
    rng = np.random.RandomState(0)
    from sspslam_amd.builder import BuiltModel
    m = BuiltModel(0.001)
    x_off, out_off = 0, 3 * K
    m.sig_size = 3 * K + 5 * K
    m.sig_init = np.zeros(m.sig_size)
    m.sig_init[:3 * K] = rng.uniform(-1, 1, 3 * K)
    enc = rng.randn(K, 3, n) * 3
    bias = rng.uniform(-1, 3, (K, n))
    dec = rng.randn(K, 5, n) * 1e-4
    idx = (out_off + np.arange(5 * K)).reshape(K, 5).astype(np.int32)
    b = [m.add_buffer(a, nm, role) for a, nm, role in ((enc, "enc", "param"), (bias, "bias", "param"), (dec, "dec", "param"),
                                                       (idx, "idx", "index"), (np.zeros((K, n)), "v", "state"),
                                                       (np.zeros((K, n)), "r", "state"))]
    nd = dict(type="lif", tau_rc=0.02, tau_ref=0.002, min_voltage=0.0, amplitude=1.0)
    m.ops = [dict(kind="ensarray", x=x_off, K=K, n=n, din=3, dout=5, enc=b[0], bias=b[1], dec=b[2], dst_idx=b[3],
                  v=b[4], r=b[5], neuron=nd, level=0, label="big", k_lo=0, k_total=K)]
    probe = object()
    m.probes = [dict(probe=probe, src=out_off, width=5 * K, every=1)]
    with Simulator(None, model=m, dtype="f32", steps_per_graph=8) as sim:
        sim.run_steps(24)
        a = sim.data[probe].copy()
        c = sim.counters()
        assert c["dominant_units_per_launch"] == K * n and c["dominant_bytes_per_launch"] == K * n * 13 * 4
    assert np.isfinite(a).all() and np.abs(a).max() > 0
    # oracle on the first 2 steps of 16 VCOs (slice of the same arrays)
    sub = BuiltModel(0.001)
    Ks = 16
    sub.sig_size = m.sig_size
    sub.sig_init = m.sig_init
    bs = [sub.add_buffer(arr, nm, role) for arr, nm, role in (
        (enc[:Ks], "enc", "param"), (bias[:Ks], "bias", "param"), (dec[:Ks], "dec", "param"), (idx[:Ks], "idx", "index"),
        (np.zeros((Ks, n)), "v", "state"), (np.zeros((Ks, n)), "r", "state"))]
    sub.ops = [dict(m.ops[0], K=Ks, enc=bs[0], bias=bs[1], dec=bs[2], dst_idx=bs[3], v=bs[4], r=bs[5])]
    sub.probes = [dict(probe=probe, src=out_off, width=5 * Ks, every=1)]
    ref = OracleSimulator(sub)
    ref.run_steps(3)
    np.testing.assert_allclose(a[:3, :5 * Ks], ref.probe_data(0), rtol=2e-4, atol=2e-4)
    # eager / profile path gives the same bits as graph replay
    with Simulator(None, model=m, dtype="f32", steps_per_graph=1) as sim:
        sim.run_steps(24, profile=True)
        np.testing.assert_array_equal(sim.data[probe], a)
    # VCO independence
    dec2 = dec.copy()
    dec2[100] = 0
    m.buffers[b[2]] = dec2
    with Simulator(None, model=m, dtype="f32", steps_per_graph=8) as sim:
        sim.run_steps(24)
        a2 = sim.data[probe]
    changed = np.any(a2 != a, axis=0).reshape(K, 5).any(1)
    assert changed[100] and changed.sum() == 1 and np.all(a2[:, 500:505] == 0)


def _small_slam(weights_every=0.1):
    s = H.make_ssp_space(2, 55)
    path, vels = H.make_random_path(20.0, limit=0.1, seed=0)
    return H.make_slam_model(s, path, vels, n_landmarks=10, pi_n_neurons=100, mem_n_neurons=300,
                             circonv_n_neurons=50, view_rad=0.6, weights_sample_every=weights_every)


def test_slam_f64_matches_oracle(Simulator):
    """SLAMNetwork end to end: clean-up, gate, circular convolutions (product
    ensemble arrays), dense ensembles, PES and Voja - trajectory, learned decoders and learned encoders."""
    sm = _small_slam()
    model = build(sm.model)
    kinds = {o["kind"] for o in model.ops}
    assert {"cleanup", "gate", "pes", "voja", "neurons", "ensarray", "matvec"} <= kinds
    ref = OracleSimulator(model)
    ref.run_steps(500)
    mem = sm.slam.assomemory.memory
    eb = model.params[mem].encoder_buffer
    with Simulator(None, model=model, dtype="f64") as sim:
        sim.run_steps(500)
        np.testing.assert_allclose(sim.data[sm.probe], ref.probe_data(0), atol=1e-9, rtol=0)
        W_gpu = sim.data[sm.weights_probe]
        W_ref = ref.probe_data(1)
        assert W_gpu.shape == W_ref.shape == (5, 55, 300) and np.abs(W_ref[-1]).max() > 1e-5   # PES learned something
        np.testing.assert_allclose(W_gpu, W_ref, atol=1e-12, rtol=1e-9)
        E_gpu = sim.read_buffer(eb)
        assert np.abs(ref.buf[eb] - model.buffers[eb]).max() > 0.05                            # Voja moved encoders
        np.testing.assert_allclose(E_gpu, ref.buf[eb], atol=1e-10, rtol=1e-9)
        # map recall (run_slam.py:263-268) from GPU-learned decoders vs oracle-learned decoders
        import sspslam_amd.frontend as fe
        rec_g, pos_g = H.map_recall(sm.ssp_space, sm.lm_space, model.params[mem], fe.LIF(), W_gpu[-1])
        rec_r, pos_r = H.map_recall(sm.ssp_space, sm.lm_space, model.params[mem], fe.LIF(), W_ref[-1])
        np.testing.assert_allclose(rec_g, rec_r, atol=1e-9)
        np.testing.assert_array_equal(pos_g, pos_r)


def test_slam_f32_within_cosine_bar(Simulator):
    """f32 fast mode: trajectory and map-recall vectors (run_slam.py:263-268) within 1e-3 cosine of the oracle."""
    import sspslam_amd.frontend as fe
    sm = _small_slam(weights_every=0.1)
    model = build(sm.model)
    ref = OracleSimulator(model)
    ref.run_steps(300)
    mem = sm.slam.assomemory.memory
    with Simulator(None, model=model, dtype="f32") as sim:
        sim.run_steps(300)
        ce = H.cosine_error(sim.data[sm.probe][20:], ref.probe_data(0)[20:])
        W_gpu = sim.data[sm.weights_probe]
    assert ce.max() < 1e-3, ce.max()
    rec_g, _ = H.map_recall(sm.ssp_space, sm.lm_space, model.params[mem], fe.LIF(), W_gpu[-1])
    rec_r, _ = H.map_recall(sm.ssp_space, sm.lm_space, model.params[mem], fe.LIF(), ref.probe_data(1)[-1])
    seen = np.linalg.norm(rec_r, axis=1) > 1e-6            # landmarks the memory has learned something about
    assert seen.any()
    assert H.cosine_error(rec_g[seen], rec_r[seen]).max() < 1e-3


def test_slamview_f64_matches_oracle(Simulator):
    """SLAMViewNetwork (reference slam_view.py, run_slamview.py): trajectory, recall and learned decoders."""
    s = H.make_ssp_space(2, 55)
    path, vels = H.make_random_path(20.0, limit=0.1, seed=0)
    sm = H.make_slamview_model(s, path, vels, n_landmarks=10, pi_n_neurons=100, mem_n_neurons=300, view_rad=0.6,
                               weights_sample_every=0.1)
    model = build(sm.model)
    ref = OracleSimulator(model)
    ref.run_steps(400)
    with Simulator(None, model=model, dtype="f64") as sim:
        sim.run_steps(400)
        np.testing.assert_allclose(sim.data[sm.probe], ref.probe_data(0), atol=1e-9, rtol=0)
        np.testing.assert_allclose(sim.data[sm.recall_probe], ref.probe_data(1), atol=1e-9, rtol=0)
        W = sim.data[sm.weights_probe]
        assert np.abs(W[-1]).max() > 1e-6
        np.testing.assert_allclose(W, ref.probe_data(2), atol=1e-12, rtol=1e-9)
    with Simulator(None, model=model, dtype="f32") as sim:
        sim.run_steps(300)
        assert H.cosine_error(sim.data[sm.probe][20:], ref.probe_data(0)[20:300]).max() < 1e-3


def test_dft_kernel_matches_the_transform_matrices(Simulator):
    """k_dft (the FFT of the circular-convolution transforms, f32 core) against the dense real-DFT matrices it replaces
    (reference binding.py:23-74): in ONE run, the probed output of each transform equals matrix @ probed input.  Both
    engines: the Stockham passes (default) and the four-step transform on the matrix cores (flag 536870912, round 3: two small
    dense DFTs as f32 MFMA products around a twiddle multiply).  d = 25 (5 x 5), 55 (5 x 11),
    217 (7 x 31), 1015 (35 x 29, the benchmark's dimension), 97 (prime: ONE dense DFT in the four-step engine, Bluestein in the
    Stockham one); d = 1801 (prime; what ssp_dim = 2047 gives in 3-D, BASELINE config 5) and d = 2049 (3 x 683; SURVEY's other
    reading of config 5) go through Bluestein's convolution in both; both operand layouts, with and without involution; the
    inverse transform."""
    from sspslam_amd.networks import CircularConvolution
    from sspslam_amd.builder import dft_structure
    FOURSTEP, BIG = PLAN.SSN_PLAN_FOUR_STEP_FFT, PLAN.SSN_PLAN_BLUESTEIN_FFT
    # (even lengths: 40 = 8 x 5, 44 = 4 x 11 and 70 = 2 x 7 x 5 run a radix-8 / 4 / 2 pass as in-register butterflies between
    #  generic ones - dft_pass_small; the odd lengths' chirp-z transforms run them in place - dft_pass_inplace)
    for d, inv_a, inv_b in ((25, False, True), (55, True, False), (217, False, False), (97, False, True), (1015, True, False),
                            (40, False, False), (44, True, False), (70, False, True), (1801, True, False), (2049, False, True)):
        rng = np.random.RandomState(d)
        fa, fb = rng.randn(d) / np.sqrt(d), rng.randn(d) / np.sqrt(d)
        with nengo.Network(seed=1) as m:
            ua = nengo.Node(lambda t, f=fa: f * np.cos(9 * t))
            ub = nengo.Node(lambda t, f=fb: f * np.sin(7 * t) + f[::-1] * 0.5)
            ea = nengo.Ensemble(60, d)
            eb = nengo.Ensemble(60, d)
            nengo.Connection(ua, ea, synapse=None)
            nengo.Connection(ub, eb, synapse=None)
            cc = CircularConvolution(12, d, invert_a=inv_a, invert_b=inv_b)
            nengo.Connection(ea, cc.input_a, synapse=0.005)
            nengo.Connection(eb, cc.input_b, synapse=0.005)
            p_a, p_b = nengo.Probe(cc.input_a), nengo.Probe(cc.input_b)
            p_fa, p_fb = nengo.Probe(cc.product.input_a), nengo.Probe(cc.product.input_b)
            p_prod, p_out = nengo.Probe(cc.product.output), nengo.Probe(cc.output)
            sink = nengo.Ensemble(30, d)                  # neurons downstream keep the inverse transform in the core
            nengo.Connection(cc.output, sink, synapse=None)
        model = build(m)
        assert all(o["stage"] == 1 for o in model.ops if o["kind"] == "matvec" and o.get("dft"))
        kinds = sorted(o.get("dft", 0) for o in model.ops if o["kind"] == "matvec" and o.get("dft"))
        assert kinds == sorted([3 if inv_a else 1, 4 if inv_b else 2, 5]), kinds
        assert dft_structure(cc.transform_out) == 5 and dft_structure(np.eye(8)) == 0
        big = d in (1801, 2049)
        if big:       # a chirp-z transform of 2048+ points: the planner prefers the dense matrix (spread over the chip) by default
            with Simulator(None, model=model, dtype="f32") as sim:
                assert sim.counters()["fft_transforms"] == 0
        for engine in (0, FOURSTEP):
            with Simulator(None, model=model, dtype="f32", flags=engine | (BIG if big else 0)) as sim:
                sim.run_steps(120)
                a, b, fa_, fb_ = sim.data[p_a], sim.data[p_b], sim.data[p_fa], sim.data[p_fb]
                prod, out = sim.data[p_prod], sim.data[p_out]
                c = sim.counters()
                n_blue = 3 if (big or (d == 97 and engine == 0)) else 0
                assert c["fft_transforms"] == 3 and c["fft_bluestein"] == n_blue, (d, engine, c)
            assert np.abs(a).max() > 0.005 and np.abs(prod).max() > 1e-5
            np.testing.assert_allclose(fa_, a @ cc.transform_a.T, atol=2e-6 * np.sqrt(d), err_msg=f"d {d} engine {engine}")
            np.testing.assert_allclose(fb_, b @ cc.transform_b.T, atol=2e-6 * np.sqrt(d), err_msg=f"d {d} engine {engine}")
            np.testing.assert_allclose(out, prod @ cc.transform_out.T, atol=2e-6, err_msg=f"d {d} engine {engine}")


def test_slam_optin_plans_equal_default(Simulator):
    """The A/B switches of ssn_model_desc.flags select alternative plans of the same operators: same trajectory as the
    default plan (f64; bit-equal where the summation order is the same).  Default: rounds (k_round), the 16 timesteps of a
    step graph software-pipelined; 2097152 selects the round-1 plan (one launch per operator / per program)."""
    sm = _small_slam(weights_every=None)
    model = build(sm.model)
    ref = OracleSimulator(model)
    ref.run_steps(120)
    OLD = PLAN.SSN_PLAN_NO_ROUNDS
    outs, launches = {}, {}
    for flags in (0, PLAN.SSN_PLAN_SPMV_OWN_LIST, PLAN.SSN_PLAN_ENS_PARTIALS, PLAN.SSN_PLAN_ENS_OWN_LAUNCH, PLAN.SSN_PLAN_NO_PIPELINE, PLAN.SSN_PLAN_NO_BALANCE, PLAN.SSN_PLAN_NO_CUTS, PLAN.SSN_PLAN_NO_CHAINS,
                  OLD, OLD | PLAN.SSN_PLAN_NO_ITEM_BATCH, PLAN.SSN_PLAN_NO_STAGE_BATCH):
        with Simulator(None, model=model, dtype="f64", flags=flags) as sim:
            sim.run_steps(120)             # 7 graph replays of 16 pipelined steps + 8 steps launched one round at a time
            outs[flags] = sim.data[sm.probe]
            launches[flags] = sim.counters()["launches_per_step"]
    np.testing.assert_allclose(outs[0], ref.probe_data(0), atol=1e-9, rtol=0)
    np.testing.assert_allclose(outs[1024], outs[0], atol=1e-12, rtol=0)   # spike list rebuilt in the product kernel: other chunking
    np.testing.assert_allclose(outs[PLAN.SSN_PLAN_ENS_PARTIALS], outs[0], atol=1e-12, rtol=0)   # finish operator vs direct write of one-workgroup ensembles
    for flags in (PLAN.SSN_PLAN_ENS_OWN_LAUNCH,        # ensemble arrays launched on their own vs as bodies of the round's grid
                  PLAN.SSN_PLAN_NO_PIPELINE,        # one timestep's rounds at a time vs 16 timesteps software-pipelined
                  PLAN.SSN_PLAN_NO_BALANCE,       # no splitting of heavy operators over the rounds of their slack window
                  PLAN.SSN_PLAN_NO_CUTS,       # merged element-wise operators kept whole vs cut at the other operators' range endpoints
                  PLAN.SSN_PLAN_NO_CHAINS,      # no chains of element-aligned micro-operators inside a block
                  PLAN.SSN_PLAN_NO_STAGE_BATCH):        # one launch per element-wise operator of the batched stages
        np.testing.assert_array_equal(outs[flags], outs[0], err_msg=str(flags))
    np.testing.assert_allclose(outs[OLD], outs[0], atol=1e-12, rtol=0)       # (the gate's dot product sums 16 wave partials there, 4 here)
    np.testing.assert_array_equal(outs[OLD | PLAN.SSN_PLAN_NO_ITEM_BATCH], outs[OLD])      # one launch per operator vs batched neighbours
    assert launches[0] < launches[PLAN.SSN_PLAN_NO_PIPELINE] < launches[OLD]
    # a profiled run computes what a plain one does: the pipelined sequence, one timestep's rounds at a time, generic items
    for flags in (0, PLAN.SSN_PLAN_NO_PIPELINE, OLD):
        for profile in (1, 2):
            with Simulator(None, model=model, dtype="f64", flags=flags) as sim:
                sim.run_steps(120, profile=profile)
                np.testing.assert_array_equal(sim.data[sm.probe], outs[flags], err_msg=f"flags {flags} profile {profile}")
                times = sim.kernel_times()
            if profile == 2:
                assert times and all(n > 0 for n, _ in times.values())
                assert flags == OLD or "k_round" in times, (flags, sorted(times))


def test_serial_chains_equal_plain_rounds(Simulator):
    """Serial chains (RK_SOLO: single-workgroup operators of consecutive rounds run by one block, a workgroup barrier between
    them) change where an operator runs, not what it computes: the f32 trajectory of a SLAM network is bit-equal with the
    chains off (SSN_SOLO_CHAINS=0), with the default glue-only chains, and with the transforms as members under a generous
    cap (SSN_SOLO_DFT=1, SSN_SOLO_CAP_US=40); the plans do differ (launches per timestep)."""
    sm = _small_slam(weights_every=None)
    model = build(sm.model)
    outs, launches = {}, {}
    saved = {k: os.environ.get(k) for k in ("SSN_SOLO_CHAINS", "SSN_SOLO_DFT", "SSN_SOLO_CAP_US")}
    try:
        for name, env in (("off", {"SSN_SOLO_CHAINS": "0"}), ("default", {}), ("dft", {"SSN_SOLO_DFT": "1", "SSN_SOLO_CAP_US": "40"})):
            for k in saved:
                os.environ.pop(k, None)
            os.environ.update(env)
            with Simulator(None, model=model, dtype="f32", steps_per_graph=16) as sim:
                sim.run_steps(200)
                outs[name] = sim.data[sm.probe]
                c = sim.counters()
                launches[name] = (c["launches_per_step"], c["fft_transforms"], c["serial_chains"])
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    assert np.abs(outs["off"]).max() > 0.01 and launches["off"][1] > 0
    np.testing.assert_array_equal(outs["default"], outs["off"])
    np.testing.assert_array_equal(outs["dft"], outs["off"])
    assert launches["dft"][0] <= launches["default"][0] <= launches["off"][0]
    assert launches["off"][2] == 0 and launches["default"][2] > 0 and launches["dft"][2] > 0


def test_feedforward_model_runs_fully_batched(Simulator):
    """No neurons at all (the multi-GPU read-out is such a model): every operator runs time-batched -
    GEMM over the block, lowpass scans with carry across block boundaries (block = 64 here)."""
    rng = np.random.RandomState(0)
    Tm = rng.randn(7, 5)
    with nengo.Network(seed=0) as m:
        u = nengo.Node(lambda t: np.sin(np.arange(1, 6) * 9 * t))
        a = nengo.Node(size_in=7)
        b = nengo.Node(size_in=7)
        nengo.Connection(u, a, transform=Tm, synapse=0.01)
        nengo.Connection(a, b, synapse=0.005)
        nengo.Connection(u[:2], b[3:5], transform=-2.0, synapse=None)
        p1, p2, p3 = nengo.Probe(b, synapse=0.02), nengo.Probe(a), nengo.Probe(u, sample_every=0.003)
    model = build(m)
    assert all(o["stage"] == 2 for o in model.ops) and model.stage_info["enabled"]
    ref = OracleSimulator(model)
    ref.run_steps(300)
    with Simulator(None, model=model, dtype="f64", block_steps=64) as sim:
        sim.run_steps(100)
        sim.run_steps(200)
        assert sim.counters()["launches_per_step"] == 0
        for i, p in enumerate((p1, p2, p3)):
            np.testing.assert_allclose(sim.data[p], ref.probe_data(i), atol=1e-12, rtol=0)
        assert sim.data[p3].shape == (100, 5)
    # f32: the chunked scan (blocks of >= 256 timesteps) against the same oracle run
    ref.run_steps(400)
    with Simulator(None, model=model, dtype="f32", block_steps=512) as sim:
        sim.run_steps(700)
        for i, p in enumerate((p1, p2, p3)):
            np.testing.assert_allclose(sim.data[p], ref.probe_data(i), atol=2e-5, rtol=0)
    # f32 products large enough for the matrix cores (kb_gemm_mfma_f32: cols >= 64, rows >= 32): ragged tiles - 150 rows
    # (two full 64-row tiles + 22), 100 columns (three K slabs of 32 + 4), 300-step blocks (four 64-step tiles + 44)
    T2, T3 = rng.randn(150, 100) / 10, rng.randn(70, 150) / 12
    with nengo.Network(seed=0) as m2:
        u = nengo.Node(lambda t: np.sin(np.arange(1, 101) * 3 * t))
        a = nengo.Node(size_in=150)
        b = nengo.Node(size_in=70)
        nengo.Connection(u, a, transform=T2, synapse=0.01)
        nengo.Connection(a, b, transform=T3, synapse=None)
        q1, q2 = nengo.Probe(a), nengo.Probe(b, synapse=0.005)
    model2 = build(m2)
    ref2 = OracleSimulator(model2)
    ref2.run_steps(700)
    with Simulator(None, model=model2, dtype="f32", block_steps=300) as sim:
        sim.run_steps(700)
        assert np.abs(ref2.probe_data(1)).max() > 0.05
        for i, p in enumerate((q1, q2)):
            np.testing.assert_allclose(sim.data[p], ref2.probe_data(i), atol=3e-6, rtol=0)


@pytest.mark.parametrize("ssp_dim,n", [(55, 60), (1015, 70)])
def test_sharded_runner_on_hip_matches_unsharded(Simulator, ssp_dim, n):
    from sspslam_amd.sharding import ShardedPathIntegration
    pm = small_pathint(ssp_dim=ssp_dim, n=n, T=10.0, limit=0.2)
    model = build(pm.model)
    ref = OracleSimulator(model)
    ref.run_steps(300)
    pm2 = small_pathint(ssp_dim=ssp_dim, n=n, T=10.0, limit=0.2)
    r = ShardedPathIntegration(pm2, 0, 1, dtype="f64", block=128)
    r.prepare(300)
    r.run_steps(300)
    np.testing.assert_allclose(r.probe_data(), ref.probe_data(0), atol=1e-9, rtol=0)
    assert r.readout.counters()["launches_per_step"] == 0        # read-out replays fully batched
    r.close()


SHARD_WORKER = r"""
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import torch.distributed as dist
from helpers import small_pathint
from sspslam_amd.sharding import ShardedPathIntegration
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
out = {{}}
for dtype in ("f64", "f32"):
    pm = small_pathint(ssp_dim=1015, n=70, T=10.0, limit=0.2)
    r = ShardedPathIntegration(pm, rank, world, dtype=dtype, block=128)
    assert r.hi - r.lo == 254
    r.prepare(300)
    r.run_steps(300)          # 128 + 128 + 44: ragged last block
    r.flush()
    if rank == 0:
        out[dtype] = r.probe_data()
    r.close()
if rank == 0:
    np.savez({out!r}, **out)
dist.barrier()
dist.destroy_process_group()
"""


def test_two_ranks_on_hip_equal_the_unsharded_model(Simulator, tmp_path):
    """Two ranks (gloo, sharing this GPU: RCCL needs one GPU per rank) each step 254 of the 508 VCOs of a
    ssp_dim = 1015 path integrator - the 2-GPU shard of BASELINE config 2, whole-block kernel - exchange their
    decoded oscillator outputs per block, and rank 0 replays the read-out: f64 equal to the oracle's unsharded run."""
    import subprocess
    import sys
    script, out = tmp_path / "worker.py", tmp_path / "probe.npz"
    script.write_text(SHARD_WORKER.format(root=ROOT, out=str(out)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29671")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29672", str(script)],
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    got = np.load(out)
    ref = OracleSimulator(build(small_pathint(ssp_dim=1015, n=70, T=10.0, limit=0.2).model))
    ref.run_steps(300)
    want = ref.probe_data(0)
    np.testing.assert_allclose(got["f64"], want, atol=1e-9, rtol=0)
    assert H.cosine_error(got["f32"][20:], want[20:]).max() < 1e-3


SLAM_SHARD_WORKER = r"""
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import torch
import torch.distributed as dist
from sspslam_amd import harness as H
from sspslam_amd.sharding import ShardedSLAM
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
s = H.make_ssp_space(2, 55)
path, vels = H.make_random_path(20.0, limit=0.1, seed=0)
res = {{}}
for dtype in ("f64", "f32"):
    for turn in range(world):            # ranks share one GPU here: build (rocSOLVER) one after the other
        if turn == rank:
            sm = H.make_slam_model(s, path, vels, n_landmarks=10, pi_n_neurons=100, mem_n_neurons=300, circonv_n_neurons=50, view_rad=0.6)
            r = ShardedSLAM(sm, rank, world, dtype=dtype)
        dist.barrier()
    r.prepare({steps})
    r.run_steps({steps})
    am = sm.slam.assomemory
    res[dtype] = r.probe_data()
    res[dtype + "_W"], res[dtype + "_E"] = r.learned_decoders(am.conn_out), r.learned_encoders(am.memory)
    res["launches"] = r.sim.counters()["launches_per_step"]
    r.close()
if rank == 0:
    np.savez({out!r}, **res)
dist.barrier()
dist.destroy_process_group()
"""


def test_two_ranks_of_a_neuron_sharded_slam_on_hip(Simulator, tmp_path):
    """SLAMNetwork split over two ranks (gloo, sharing this GPU; with one GPU per rank the same runner exchanges through
    RCCL in HBM): VCOs and product ensembles by ensemble, memory / recall / error by neuron, one all-reduce per timestep
    between the two captured halves of the step graph (ssn_run_phase).  f64: trajectory, gathered PES decoders and
    Voja encoders equal the UNSHARDED oracle run at 1e-9; f32 within the cosine bar."""
    import subprocess
    import sys
    steps = 300
    script, out = tmp_path / "worker.py", tmp_path / "slam.npz"
    script.write_text(SLAM_SHARD_WORKER.format(root=ROOT, out=str(out), steps=steps))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29674", str(script)],
                       env=env, capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    got = np.load(out)
    sm = _small_slam(weights_every=None)
    model = build(sm.model)
    ref = OracleSimulator(model)
    ref.run_steps(steps)
    want = ref.probe_data(0)
    am = sm.slam.assomemory
    W_ref = ref.buf[model.params[am.conn_out].learned_buffer]
    E_ref = ref.buf[model.params[am.memory].encoder_buffer]
    assert np.abs(W_ref).max() > 1e-6
    np.testing.assert_allclose(got["f64"], want, atol=1e-9, rtol=0)
    np.testing.assert_allclose(got["f64_W"], W_ref, atol=1e-12, rtol=1e-9)
    np.testing.assert_allclose(got["f64_E"], E_ref, atol=1e-10, rtol=1e-9)
    assert H.cosine_error(got["f32"][20:], want[20:]).max() < 1e-3
    assert 4 <= int(got["launches"]) <= 60


def test_sharded_runner_device_exchange(Simulator):
    """The all-device block exchange (probe -> RCCL all-gather -> read-out table, no host copies) on a
    single-rank RCCL group: same read-out as the oracle."""
    import torch.distributed as dist
    from sspslam_amd.sharding import ShardedPathIntegration
    pm = small_pathint(ssp_dim=55, n=60, T=10.0, limit=0.2)
    model = build(pm.model)
    ref = OracleSimulator(model)
    ref.run_steps(300)
    created = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29531", rank=0, world_size=1)
        created = True
    try:
        for dtype, tol, defer, every in (("f64", 1e-9, None, 4), ("f64", 1e-9, 2, 1), ("f32", None, None, 2)):
            pm2 = small_pathint(ssp_dim=55, n=60, T=10.0, limit=0.2)
            # read-out replayed on the worker thread (default for small shards) or deferred; exchange every
            # `every` blocks (the remainder is gathered by flush() / probe_data())
            r = ShardedPathIntegration(pm2, 0, 1, dtype=dtype, block=128, device_exchange=True, defer_readout=defer,
                                       gather_every=every)
            r.prepare(300)
            r.run_steps(300)
            got = r.probe_data()
            if tol:
                np.testing.assert_allclose(got, ref.probe_data(0), atol=tol, rtol=0)
            else:
                assert H.cosine_error(got[20:], ref.probe_data(0)[20:]).max() < 1e-3
            r.close()
    finally:
        if created:
            dist.destroy_process_group()
    # a failing device exchange raises (no silent switch to another collective while peers may be inside this one)
    pm4 = small_pathint(ssp_dim=55, n=60, T=10.0, limit=0.2)
    r = ShardedPathIntegration(pm4, 0, 1, dtype="f64", block=128, device_exchange=True, gather_every=1)

    def broken(n):
        raise RuntimeError("simulated failure of the local half")
    r._stage_send = broken
    r.prepare(300)
    with pytest.raises(nengo.SimulationError, match="block exchange failed on rank 0"):
        r.run_steps(300)
    r._ungathered = 0
    r.close()
    # ... and so does stepping without prepare() (the probe storage would be re-reserved block by block)
    pm5 = small_pathint(ssp_dim=55, n=60, T=10.0, limit=0.2)
    r = ShardedPathIntegration(pm5, 0, 1, dtype="f64", block=128, device_exchange=True)
    with pytest.raises(nengo.SimulationError, match="prepare"):
        r.run_block()
    r.close()
    # a last rank with fewer VCOs than the others (28 VCOs over 3 ranks: 10, 10, 8): its samples are padded to the
    # common width before the all-gather; without a process group its slot of the gathered block is checked alone
    pm3 = small_pathint(ssp_dim=55, n=60, T=10.0, limit=0.2)
    r = ShardedPathIntegration(pm3, 2, 3, dtype="f64", block=64, device_exchange=True)
    assert (r.lo, r.hi, r.per) == (20, 28, 10) and r.readout is None
    r.prepare(64)
    r.sim.run_steps(64, collect=False)
    full = r._gather_device(64).cpu().numpy()
    own = r.sim.data[r.osc_probe]
    assert full.shape == (64, 3 * 28) and np.abs(own).max() > 0
    np.testing.assert_array_equal(full[:, :60], 0.0)                   # the other ranks' slots (nobody filled them)
    np.testing.assert_array_equal(full[:, 60:84], own[:, :24])
    r.close()


class _ThreadDist:
    """torch.distributed stand-in for several ranks living in ONE process (one thread each, sharing the GPU): the
    collectives meet at a barrier and exchange device tensors directly - the world > 1 code path of the device
    exchange (padded all_gather_into_tensor, ok-flag all-reduce) without needing one GPU per rank."""

    class ReduceOp:
        MAX = "max"

    def __init__(self, world):
        import threading
        self.world = world
        self.barrier = threading.Barrier(world)
        self.slots = [None] * world
        self.local = threading.local()

    def is_initialized(self):
        return True

    def get_backend(self):
        return "nccl"

    def _meet(self, t):
        self.slots[self.local.rank] = t
        self.barrier.wait()
        got = list(self.slots)
        self.barrier.wait()
        return got

    # (stream-level waits, not torch.cuda.synchronize(): a device-wide synchronisation from one rank's thread invalidates a
    #  stream capture another rank's thread has open - ssn_phase_async captures its graphs at the first call of a run; real
    #  RCCL collectives never synchronise the device)
    # Like a real collective, ordered on the caller's CURRENT stream only: what the caller enqueued on that stream before is
    # complete when the ranks meet, and the result is complete when the call returns.  (No torch.cuda.synchronize(): a
    # device-wide wait would hide a caller that launched its kernels on a stream the collective is not ordered with.)
    def all_gather_into_tensor(self, out, send):
        import torch
        torch.cuda.current_stream().synchronize()
        for r, t in enumerate(self._meet(send)):
            out[r].copy_(t)
        torch.cuda.current_stream().synchronize()

    def all_reduce(self, t, op=None):
        import torch
        c = t.clone()
        torch.cuda.current_stream().synchronize()
        got = self._meet(c)
        st = torch.stack([g.to(t.device) for g in got])
        t.copy_(st.max(dim=0).values if op == "max" else st.sum(dim=0))
        torch.cuda.current_stream().synchronize()

    def all_gather(self, outs, t):
        for o, g in zip(outs, self._meet(t.clone())):
            o.copy_(g)


def test_device_exchange_with_three_ranks_in_one_process(Simulator):
    """World size 3 over 28 VCOs (shards of 10, 10 and 8: the last one padded) through the DEVICE exchange path -
    `_stage_send`, the ok-flag all-reduce, `all_gather_into_tensor`, `assemble_gathered`, gather_every > 1 and the
    deferred read-out - equal to the unsharded oracle run."""
    import threading
    from sspslam_amd.sharding import ShardedPathIntegration
    ref = OracleSimulator(build(small_pathint(ssp_dim=55, n=60, T=10.0, limit=0.2).model))
    ref.run_steps(320)
    world = 3
    fake = _ThreadDist(world)
    results, errors = {}, []
    runners = [ShardedPathIntegration(small_pathint(ssp_dim=55, n=60, T=10.0, limit=0.2), rank, world, dtype="f64", block=64,
                                      device_exchange=True, dist=fake, gather_every=2, defer_readout=2 if rank == 0 else 0)
               for rank in range(world)]
    assert [(r.lo, r.hi) for r in runners] == [(0, 10), (10, 20), (20, 28)]

    def work(rank):
        try:
            fake.local.rank = rank
            r = runners[rank]
            r._warm = True                       # (no communicator to warm up)
            r.prepare(320)
            r.run_steps(320)                     # 5 blocks: two exchanges of 2 blocks, flush() gathers the fifth
            r.flush()
            if rank == 0:
                results["out"] = r.probe_data()
        except BaseException as e:               # noqa: BLE001
            errors.append((rank, e))
            fake.barrier.abort()

    threads = [threading.Thread(target=work, args=(rank,)) for rank in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    assert not errors, errors
    np.testing.assert_allclose(results["out"], ref.probe_data(0), atol=1e-9, rtol=0)
    for r in runners:
        r.close()


def test_sharded_slam_device_exchange_with_two_ranks_in_one_process(Simulator):
    """The neuron-sharded SLAMNetwork through the DEVICE exchange path (what RCCL ranks run: ssn_exchange_pack into a
    device buffer -> all-reduce of that buffer -> ssn_exchange_unpack, between ssn_run_phase(0) and (1)), with two ranks
    living in one process and a stand-in communicator that sums the device tensors: trajectory and gathered PES decoders
    equal the unsharded oracle run."""
    import threading
    from sspslam_amd.sharding import ShardedSLAM
    steps, world = 150, 2
    sm0 = _small_slam(weights_every=None)
    model = build(sm0.model)
    ref = OracleSimulator(model)
    ref.run_steps(steps)
    W_ref = ref.buf[model.params[sm0.slam.assomemory.conn_out].learned_buffer]
    fake = _ThreadDist(world)
    sms = [_small_slam(weights_every=None) for _ in range(world)]
    runners = [ShardedSLAM(sms[rank], rank, world, dtype="f64", dist=fake) for rank in range(world)]
    assert all(len(r.model.exchange) > 0 for r in runners)
    for r in runners:
        assert r._stream_ordered()
        r.capture()            # (ranks that share a process build their step graphs one after the other, before the threads run)
    results, errors = {}, []

    def work(rank):
        try:
            import torch
            torch.cuda.set_device(0)
            fake.local.rank = rank
            r = runners[rank]
            r.prepare(steps)
            r.run_steps(steps)
            W = r.learned_decoders(sms[rank].slam.assomemory.conn_out)
            if rank == 0:
                results["out"], results["W"] = r.probe_data(), W
        except BaseException as e:               # noqa: BLE001
            errors.append((rank, e))
            fake.barrier.abort()

    threads = [threading.Thread(target=work, args=(rank,)) for rank in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    assert not errors, errors
    np.testing.assert_allclose(results["out"], ref.probe_data(0), atol=1e-9, rtol=0)
    np.testing.assert_allclose(results["W"], W_ref, atol=1e-12, rtol=1e-9)
    assert np.abs(W_ref).max() > 1e-6
    for r in runners:
        r.close()


def test_fused_recurrent_core_equals_generic_path(Simulator):
    """The fused [k_ensarray prologue + k_ens_finish] core and the generic program path are two plans of
    the same operators: identical trajectories (f64), incl. multi-chunk ensembles (n > 1024)."""
    pm = small_pathint(ssp_dim=55, n=2500, T=10.0, limit=0.2)
    model = build(pm.model, n_eval_points=600)
    outs = []
    for flags in (PLAN.SSN_PLAN_NO_BLOCK_KERNEL, PLAN.SSN_PLAN_NO_FUSED_CORE, PLAN.SSN_PLAN_SEPARATE_FINISH):    # deferred finish (1 launch/step) | generic programs | fused with separate finish kernel
        with Simulator(None, model=model, dtype="f64", flags=flags, block_steps=96) as sim:
            sim.run_steps(150)
            sim.run_steps(150)        # block boundaries, eager remainders and a second call: flush/begin paths
            outs.append(sim.data[pm.probe])
            outs.append(sim.counters()["launches_per_step"])
    assert outs[1] == 1 and 2 <= outs[3] <= 8 and outs[5] == 2      # (the generic plan: one launch per dependency round)
    np.testing.assert_array_equal(outs[0], outs[2])
    np.testing.assert_array_equal(outs[0], outs[4])
    # LIF fast path (packed state word, spike-sparse neuron-major decoders) vs the generic kernel: same bits
    with Simulator(None, model=model, dtype="f64", flags=PLAN.SSN_PLAN_NO_LIF_FAST, block_steps=96) as sim:
        sim.run_steps(300)
        np.testing.assert_array_equal(sim.data[pm.probe], outs[0])
    ref = OracleSimulator(model)
    ref.run_steps(300)
    np.testing.assert_allclose(outs[0], ref.probe_data(0), atol=1e-9, rtol=0)
    # default plan: the whole block in one launch (k_ens_block, one workgroup per VCO, state in registers);
    # same arithmetic per neuron, the spike sums are added in a different (fixed) order
    with Simulator(None, model=model, dtype="f64", block_steps=96) as sim:
        sim.run_steps(150)
        sim.run_steps(150)
        assert sim.counters()["launches_per_step"] == 0
        np.testing.assert_allclose(sim.data[pm.probe], ref.probe_data(0), atol=1e-9, rtol=0)
        # neuron state and filter states were written back: continuing per-timestep from here stays on the oracle
        v_buf = next(o for o in model.ops if o["kind"] == "ensarray")["v"]
        got_v = sim.read_buffer(v_buf)
        np.testing.assert_allclose(got_v, np.asarray(ref.buf[v_buf]).reshape(got_v.shape), atol=1e-9, rtol=0)
        batched_stage_out = sim.data[pm.probe]
    # one launch per element-wise operator of the time-batched stages vs independent neighbours sharing a launch
    with Simulator(None, model=model, dtype="f64", block_steps=96, flags=PLAN.SSN_PLAN_NO_STAGE_BATCH) as sim:
        sim.run_steps(150)
        sim.run_steps(150)
        np.testing.assert_array_equal(sim.data[pm.probe], batched_stage_out)


def test_example_script_with_the_reference_command_line(Simulator, tmp_path):
    """examples/run_pathint.py: the reference's run_pathint.py options end to end, result file in its format."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("run_pathint_example", os.path.join(ROOT, "examples", "run_pathint.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--ssp-dim", "7", "--pi-n-neurons", "64", "--T", "2.5", "--limit", "0.5", "--save", "--save-dir", str(tmp_path)])
    assert out.shape == (2500, 7) and np.isfinite(out).all()
    files = os.listdir(tmp_path)
    assert len(files) == 1 and files[0].startswith("pi_backend_mi355x_sspdim_7_pinneurons_64_T_2_")
    z = np.load(tmp_path / files[0], allow_pickle=True)
    assert z["pi_sim_out"].shape == (2500, 7) and z["pi_path"].shape == (2500, 2) and float(z["elapsed_time"]) > 0


def test_slam_example_script(Simulator, tmp_path):
    """examples/run_slam.py: options of the reference's run_slam.py, map recall and the result file."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("run_slam_example", os.path.join(ROOT, "examples", "run_slam.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out, lm_locs = mod.main(["--ssp-dim", "55", "--pi-n-neurons", "60", "--mem-n-neurons", "200", "--circonv-n-neurons", "30",
                             "--n-landmarks", "5", "--view-rad", "0.6", "--T", "5", "--limit", "0.2", "--save",
                             "--save-dir", str(tmp_path)])
    assert out.shape == (5000, 55) and lm_locs.shape == (5, 2) and np.isfinite(out).all()
    z = np.load(tmp_path / os.listdir(tmp_path)[0], allow_pickle=True)
    assert z["slam_sim_out"].shape == (5000, 55) and z["landmark_loc_est"].shape == (5, 2)


def test_pathint_3d_matches_oracle(Simulator):
    """Three-dimensional domain (BASELINE config 5's space family: simplex basis in 3-D, random rotations from a seeded
    generator): the VCO array has the same shape, so the whole-block kernel applies."""
    space = H.make_ssp_space(3, ssp_dim=33, rng=np.random.default_rng(3))
    assert space.ssp_dim == 33 and space.domain_dim == 3
    path, vels = H.make_random_path(10.0, limit=0.2, seed=2, domain_dim=3)
    pm = H.make_pathint_model(space, path, vels, 80)
    model = build(pm.model)
    ref = OracleSimulator(model)
    ref.run_steps(250)
    with Simulator(None, model=model, dtype="f64", block_steps=100) as sim:
        sim.run_steps(250)
        assert sim.counters()["launches_per_step"] == 0
        np.testing.assert_allclose(sim.data[pm.probe], ref.probe_data(0), atol=1e-9, rtol=0)
    with Simulator(None, model=model, dtype="f32") as sim:
        sim.run_steps(250)
        assert H.cosine_error(sim.data[pm.probe][20:], ref.probe_data(0)[20:]).max() < 1e-3


def test_slam_at_ssp_dim_1015_matches_oracle(Simulator):
    """SLAMNetwork at the benchmark's dimension (BASELINE configs 2 / 3: ssp_dim = 1015 = 29 * 7 * 5) with fewer neurons
    per population, so that the oracle can follow: the 10^4 x 1015 clean-up table, the 2032-row circular-convolution
    transforms (k_dft with a radix-29 stage in the f32 core), 508 VCOs, PES and Voja on 1015-column matrices."""
    space = H.make_ssp_space(2, 1015)
    path, vels = H.make_random_path(20.0, limit=0.1, seed=0)
    sm = H.make_slam_model(space, path, vels, n_landmarks=10, pi_n_neurons=100, mem_n_neurons=1200, circonv_n_neurons=20,
                           view_rad=0.6, weights_sample_every=0.05)
    with sm.model:
        p_clean = nengo.Probe(sm.slam.gridcells)
    model = build(sm.model)
    assert sorted(o["dft"] for o in model.ops if o["kind"] == "matvec" and o.get("dft")) == [1, 2, 2, 3, 5, 5]
    ref = OracleSimulator(model)
    ref.run_steps(100)
    with Simulator(None, model=model, dtype="f64") as sim:
        sim.run_steps(100)
        np.testing.assert_allclose(sim.data[sm.probe], ref.probe_data(0), atol=1e-9, rtol=0)
        np.testing.assert_allclose(sim.data[sm.weights_probe], ref.probe_data(1), atol=1e-12, rtol=1e-9)
        np.testing.assert_allclose(sim.data[p_clean], ref.probe_data(2), atol=1e-12, rtol=0)
    outs = []
    for flags in (0, PLAN.SSN_PLAN_NO_FFT, PLAN.SSN_PLAN_NO_ROUNDS | PLAN.SSN_PLAN_NO_ITEM_BATCH):       # FFT kernels | the dense transform matrices | the round-1 plan, one launch per operator
        with Simulator(None, model=model, dtype="f32", flags=flags) as sim:
            sim.run_steps(100)
            outs.append(sim.data[sm.probe])
            ce = H.cosine_error(outs[-1][20:], ref.probe_data(0)[20:])
            assert ce.max() < 1e-3, (flags, ce.max())


def test_slam_3d_matches_oracle(Simulator):
    """BASELINE config 5's shape at test size: SLAMNetwork over a three-dimensional domain, 20 landmarks.  The
    clean-up table is the reference's hard-coded 100 points per axis (slam.py:209) = 10^6 rows here, so the clean-up
    product and its argmax run over a million candidates every timestep."""
    import sspslam_amd.frontend as fe
    space = H.make_ssp_space(3, ssp_dim=33, rng=np.random.default_rng(3))
    path, vels = H.make_random_path(10.0, limit=0.5, seed=2, domain_dim=3)      # fast enough to cross grid cells
    sm = H.make_slam_model(space, path, vels, n_landmarks=20, pi_n_neurons=100, mem_n_neurons=200,
                           circonv_n_neurons=50, view_rad=0.6, weights_sample_every=0.02)
    with sm.model:
        p_clean = nengo.Probe(sm.slam.gridcells)
        p_x = nengo.Probe(sm.slam.pathintegrator.output, synapse=0.01)      # the same filter that feeds the clean-up (tau = 0.01)
    model = build(sm.model)
    cl = [o for o in model.ops if o["kind"] == "cleanup"]
    assert [o["rows"] for o in cl] == [100 ** 3] and space.domain_dim == 3
    assert (cl[0]["grid_rows"], cl[0]["grid_cols"], cl[0]["grid_k2"]) == (100, 100 ** 2, 34)
    ref = OracleSimulator(model)
    ref.run_steps(60)
    want_clean = ref.probe_data(2)
    assert len({tuple(r) for r in want_clean[20:]}) > 5                 # the cleaned-up position moves during the window
    S = sm.slam.sample_ssps
    x_o = ref.probe_data(3)
    # the clean-up of timestep t + 1 reads the filter state left by timestep t (reads precede updates)
    for t in range(10, 59):
        np.testing.assert_array_equal(want_clean[t + 1], S[np.argmax(S @ x_o[t])])
    with Simulator(None, model=model, dtype="f64") as sim:
        sim.run_steps(60)
        np.testing.assert_allclose(sim.data[sm.probe], ref.probe_data(0), atol=1e-9, rtol=0)
        np.testing.assert_allclose(sim.data[sm.weights_probe], ref.probe_data(1), atol=1e-12, rtol=1e-9)
        np.testing.assert_allclose(sim.data[p_clean], want_clean, atol=1e-12, rtol=0)
    # f32: the similarities come from the grid's factor tables (half spectrum -> left operand -> one MFMA product,
    # default for tables >= 64 MB) or from the pass over the table (flag 524288).  Near-ties between neighbouring grid
    # points (cosine 0.99 apart) may resolve differently in f32, so: the same row on nearly all steps, a neighbour otherwise
    launches = []
    for flags, split in ((0, None), (PLAN.SSN_PLAN_NO_FACTORED_GRID, None), (0, "2")):      # last: K-split product, partials summed by the argmax stage
        os.environ.pop("SSN_GRID_SPLIT", None)
        if split:
            os.environ["SSN_GRID_SPLIT"] = split
        with Simulator(None, model=model, dtype="f32", flags=flags) as sim:
            os.environ.pop("SSN_GRID_SPLIT", None)
            sim.run_steps(60)
            ce = H.cosine_error(sim.data[sm.probe][20:], ref.probe_data(0)[20:])
            assert ce.max() < 1e-3, (flags, ce.max())
            got_clean, x_g = sim.data[p_clean], sim.data[p_x]
            launches.append(sim.counters()["launches_per_step"])
        cc = H.cosine_error(got_clean[5:], want_clean[5:])
        assert (cc < 1e-6).mean() >= 0.7 and cc.max() < 0.05, (flags, (cc < 1e-6).mean(), cc.max())
        # ... and where the f32 route picks another row than the oracle it must still have picked a maximiser: against the exact
        # (float64) similarities of the kernel's OWN input vector, the chosen row is within f32 rounding of the best one
        # (neighbouring grid points are 0.99 similar: the two candidates differ in the sixth digit) - on every timestep
        worst = 0.0
        for t in range(10, 59):
            sims = S @ x_g[t]
            row = got_clean[t + 1]
            k = int(np.argmax(S @ row))                      # the grid point the kernel returned (rows are unit vectors)
            np.testing.assert_allclose(row, S[k], atol=2e-6, rtol=0)
            worst = max(worst, float(sims.max() - sims[k]) / float(np.linalg.norm(x_g[t])))
        assert worst < 2e-5, (flags, split, worst)
    assert launches[1] < launches[0] <= launches[1] + 6       # the factored route adds the half-spectrum, left-operand and product launches (and their rounds)


def test_long_run_pipelines_input_tabulation(Simulator):
    """run_steps() on an unprepared simulator tabulates the input nodes chunk by chunk on a helper thread while the
    device steps the previous chunk: same samples as preparing the whole run first."""
    pm = small_pathint(ssp_dim=7, n=64, T=10.0, limit=0.2)
    model = build(pm.model)
    with Simulator(None, model=model, dtype="f64") as sim:
        sim.prepare(7000)
        sim.run_steps(7000)
        want = sim.data[pm.probe]
    with Simulator(None, model=model, dtype="f64") as sim:
        assert 7000 > 2 * sim.PIPELINE_CHUNK
        sim.run_steps(7000)
        np.testing.assert_array_equal(sim.data[pm.probe], want)
        sim.run_steps(100)
        assert sim.data[pm.probe].shape[0] == 7100
    # the same with plain per-timestep closures (what the reference scripts pass, run_pathint.py:134-136): no `.table` twin,
    # one Python call per timestep on the helper thread, rows staged and run-length encoded in bulk (simulator.tabulate)
    saved = [tb["fn"] for tb in model.tables]
    try:
        for tb in model.tables:
            tb["fn"] = (lambda f: (lambda t: f(t)))(tb["fn"])
            assert not hasattr(tb["fn"], "table")
        with Simulator(None, model=model, dtype="f64") as sim:
            sim.run_steps(7000)
            np.testing.assert_array_equal(sim.data[pm.probe], want)
    finally:
        for tb, f in zip(model.tables, saved):
            tb["fn"] = f


def test_block_kernel_other_lif_parameters(Simulator):
    """Non-default LIF constants through the whole-block kernel; a refractory period shorter than dt (or dt / tau_rc
    above 1/8) is outside the branch-free f32 step's assumptions and must fall back to the per-timestep kernel."""
    import sspslam_amd.frontend as fe
    for lif, expect_block_f32 in ((fe.LIF(tau_rc=0.05, tau_ref=0.0022), True), (fe.LIF(tau_rc=0.03, tau_ref=0.0005), False),
                                  (fe.LIF(tau_rc=0.006, tau_ref=0.002), False)):
        pm = small_pathint(ssp_dim=19, n=700, T=10.0, limit=0.2, neuron_type=lif)
        model = build(pm.model, n_eval_points=400)
        ref = OracleSimulator(model)
        ref.run_steps(200)
        with Simulator(None, model=model, dtype="f64", block_steps=64) as sim:
            sim.run_steps(200)
            assert sim.counters()["launches_per_step"] == 0                      # f64 block kernel: the generic LIF step
            np.testing.assert_allclose(sim.data[pm.probe], ref.probe_data(0), atol=1e-9, rtol=0)
        with Simulator(None, model=model, dtype="f32", block_steps=64) as sim:
            sim.run_steps(200)
            assert (sim.counters()["launches_per_step"] == 0) == expect_block_f32
            assert H.cosine_error(sim.data[pm.probe][20:], ref.probe_data(0)[20:]).max() < 1e-3


def test_block_kernel_variants_f32(Simulator):
    """k_ens_block register / LDS variants (chosen by size; forced ones through the tuning knob) against the per-timestep
    kernel: f32, short window, cosine bar.  (The oracle comparison of the variants the planner picks at the benchmark's
    ensemble size is test_headline_block_variant_matches_oracle.)"""
    import os
    for n, variant in ((60, None), (700, None), (1500, None), (3000, None), (5000, None), (5200, "512,20,3"), (5200, "768,14,3"),
                       (2500, "1024,6,0"), (2500, "512,10,0")):
        pm = small_pathint(ssp_dim=19, n=n, T=10.0, limit=0.2)
        model = build(pm.model, n_eval_points=300)
        with Simulator(None, model=model, dtype="f32", flags=PLAN.SSN_PLAN_NO_BLOCK_KERNEL, block_steps=64) as sim:
            sim.run_steps(150)
            want = sim.data[pm.probe]
        os.environ.pop("SSN_BLOCK_VARIANT", None)
        if variant:
            os.environ["SSN_BLOCK_VARIANT"] = variant
        try:
            with Simulator(None, model=model, dtype="f32", block_steps=64) as sim:
                sim.run_steps(100)
                sim.run_steps(50)
                c = sim.counters()
                assert c["launches_per_step"] == 0
                if variant:
                    assert "%d,%d,%d" % (c["block_tpb"], c["block_npt"], c["block_enc_lds"]) == variant
                got = sim.data[pm.probe]
        finally:
            os.environ.pop("SSN_BLOCK_VARIANT", None)
        ce = H.cosine_error(got[20:], want[20:])
        assert ce.max() < 1e-3, (n, variant, ce.max())


@pytest.mark.parametrize("n,steps,variant", [(10000, 400, (512, 20, 3)), (7000, 200, (512, 20, 3)), (10240, 200, (512, 20, 3)),
                                             (10241, 200, (768, 14, 3)), (10752, 200, (768, 14, 3)), (10753, 200, None)])
def test_headline_block_variant_matches_oracle(Simulator, n, steps, variant):
    """The kernel variant behind the headline number, against the ORACLE, on the default plan: VCO ensembles of
    BASELINE config 2's size (n = 10 000 neurons each; 4 VCOs so that the NumPy oracle follows) must be stepped by
    k_ens_block<float,3,4,20,512,3> (encoder rows in LDS) - asserted through the counters - and stay within the 1e-3 cosine bar of
    the f64 oracle over 400 timesteps.  The other sizes pin the planner's variant boundaries: 10 240 = the capacity of
    (512, 20), 10 241 .. 10 752 -> (768, 14, LDS), 10 753 -> no block variant fits: per-timestep k_ensarray."""
    os.environ.pop("SSN_BLOCK_VARIANT", None)
    pm = small_pathint(ssp_dim=7, n=n, T=10.0, limit=0.2)
    model = build(pm.model, n_eval_points=1500)
    ref = OracleSimulator(model)
    ref.run_steps(steps)
    want = ref.probe_data(0)
    with Simulator(None, model=model, dtype="f32") as sim:
        sim.run_steps(steps)
        got = sim.data[pm.probe]
        c = sim.counters()
    if variant is None:
        assert c["launches_per_step"] == 1 and c["block_tpb"] == 0
    else:
        assert c["launches_per_step"] == 0
        assert (c["block_tpb"], c["block_npt"], c["block_enc_lds"]) == variant, c
        assert c["block_threads"] == variant[0]
    assert got.shape == want.shape
    ce = H.cosine_error(got[20:], want[20:])
    assert ce.max() < 1e-3, (n, ce.max())
    # the decoded oscillators really oscillate (a flat-line output would also have a tiny cosine error to itself only)
    assert np.abs(want[20:]).max() > 0.05


def test_scaled_encoders_probe_and_map_recall_of_the_learned_encoders(Simulator):
    """Probe(conn_in.learning_rule, "scaled_encoders") (reference run_slam_map_gif.py:208-209) against the oracle, and
    map-recall definition (ii) (slam_map_new.py:342-347: landmark SPs through the Voja-moved encoders, double gain
    as written) from GPU-learned vs oracle-learned state."""
    import sspslam_amd.frontend as fe
    sm = _small_slam(weights_every=0.1)
    am = sm.slam.assomemory
    with sm.model:
        p_enc = fe.Probe(am.conn_in.learning_rule, "scaled_encoders", sample_every=0.1)
    model = build(sm.model)
    i_enc = [i for i, p in enumerate(model.probes) if p["probe"] is p_enc][0]
    i_w = [i for i, p in enumerate(model.probes) if p["probe"] is sm.weights_probe][0]
    ref = OracleSimulator(model)
    ref.run_steps(500)
    E_ref, W_ref = ref.probe_data(i_enc), ref.probe_data(i_w)
    assert E_ref.shape == (5, 300, 55) and np.abs(E_ref[-1] - E_ref[0]).max() > 0.01        # Voja moved the encoders
    with Simulator(None, model=model, dtype="f64") as sim:
        sim.run_steps(300)
        sim.run_steps(200)                                        # a sample boundary inside and between runs
        E_gpu, W_gpu = sim.data[p_enc], sim.data[sm.weights_probe]
    assert E_gpu.shape == E_ref.shape
    np.testing.assert_allclose(E_gpu, E_ref, atol=1e-10, rtol=1e-9)
    np.testing.assert_allclose(W_gpu, W_ref, atol=1e-12, rtol=1e-9)
    mem = am.memory
    rec_g, pos_g = H.map_recall_learned(sm.ssp_space, sm.lm_space, model.params[mem], fe.LIF(), E_gpu[-1], W_gpu[-1])
    rec_r, pos_r = H.map_recall_learned(sm.ssp_space, sm.lm_space, model.params[mem], fe.LIF(), E_ref[-1], W_ref[-1])
    np.testing.assert_allclose(rec_g, rec_r, atol=1e-9)
    np.testing.assert_array_equal(pos_g, pos_r)
    with Simulator(None, model=model, dtype="f32") as sim:
        sim.run_steps(500)
        E32 = sim.data[p_enc]
    assert np.abs(E32 - E_ref).max() < 2e-3 * np.abs(E_ref).max()


def _gridcell_models(pi_n=80, slam_pi_n=60):
    """The two grid-cell population options of the reference: PathIntegration(with_gcs=True) (pathintegration.py:150-154)
    and SLAMNetwork(gc_n_neurons > 0) (slam.py:274-281; encoders from sample_grid_encoders, sspspace.py:733-762)."""
    import sspslam_amd.frontend as fe
    from sspslam_amd.networks import PathIntegration, SLAMNetwork, get_slam_input_functions2
    from sspslam_amd.sspspace import SPSpace
    from sspslam_amd.utils import Rd_sampling
    space = H.make_ssp_space(2, 55)
    space.rng = np.random.default_rng(11)       # grid-cell encoders are drawn from the space's generator (unseeded by default, like the reference)
    path, vels = H.make_random_path(10.0, limit=0.2, seed=1)
    real_ssp = space.encode(path)
    scale = 1.0 / np.max(np.abs(space.phase_matrix @ vels.T))
    with fe.Network(seed=2) as pi_model:
        vel = fe.Node(H.indexed_rows_node_fn(vels * scale, 0.001))
        init = fe.Node(H.indexed_rows_node_fn(real_ssp, 0.001, until=0.05))
        pi = PathIntegration(space, pi_n, 0.05, scaling_factor=scale, stable=True, with_gcs=True, n_gcs=400)
        fe.Connection(vel, pi.velocity_input, synapse=None)
        fe.Connection(init, pi.input, synapse=None)
        p1 = fe.Probe(pi.output, synapse=0.05)
        p1s = fe.Probe(pi.output.neurons[:50])
    lm_space = SPSpace(6, space.ssp_dim, seed=0)
    obj = 0.9 * 2 * (Rd_sampling(6, 2, seed=0) - 0.5)
    f = get_slam_input_functions2(space, lm_space, vels, obj[None] - path[:, None], 0.6)
    with fe.Network(seed=3) as slam_model:
        nodes = [fe.Node(fn) for fn in (f[0], f[6], f[4], f[2])]
        init = fe.Node(lambda t: real_ssp[int((t - 0.001) / 0.001)] if t < 0.05 else np.zeros(space.ssp_dim))
        slam = SLAMNetwork(space, lm_space, 0.6, 6, slam_pi_n, 150, 30, vel_scaling_factor=f[1], shift_rate=0.2, gc_n_neurons=120,
                           intercept=0.1, voja_learning_rate=1e-4, pes_learning_rate=5e-3, update_thres=0.2)
        for n, tgt in zip(nodes, (slam.velocity_input, slam.landmark_vec_ssp, slam.landmark_id_input, slam.no_landmark_in_view)):
            fe.Connection(n, tgt, synapse=None)
        fe.Connection(init, slam.pathintegrator.input, synapse=None)
        p2 = fe.Probe(slam.pathintegrator.output, synapse=0.05)
        p2g = fe.Probe(slam.gridcells, synapse=0.05)
    return (pi_model, [p1, p1s]), (slam_model, [p2, p2g])


def test_gridcell_populations_match_oracle(Simulator):
    for net, probes in _gridcell_models():
        model = build(net)
        ref = OracleSimulator(model)
        ref.run_steps(300)
        idx = {id(p["probe"]): i for i, p in enumerate(model.probes)}
        with Simulator(None, model=model, dtype="f64") as sim:
            sim.run_steps(300)
            for p in probes:
                want = ref.probe_data(idx[id(p)])
                assert np.abs(want).max() > 0
                np.testing.assert_allclose(sim.data[p], want, atol=1e-9, rtol=0)
    # f32 at north_star's 1e-3 bar, on oscillator populations that hold it: with 80 (60) neurons per oscillator a single spike
    # that falls one timestep earlier in f32 than in f64 (a voltage within an ulp of threshold) shows as a ~2e-3 transient of
    # the decoded vector (round 2 had widened the bar to 5e-3 for that); with 600 neurons per oscillator the same flip weighs
    # an eighth of that.  Both grid-cell options, all three plans.
    for net, probes in _gridcell_models(pi_n=600, slam_pi_n=600):
        model = build(net, n_eval_points=1200)
        ref = OracleSimulator(model)
        ref.run_steps(300)
        idx = {id(p["probe"]): i for i, p in enumerate(model.probes)}
        want = ref.probe_data(idx[id(probes[0])])
        for flags in (0, PLAN.SSN_PLAN_NO_PIPELINE, PLAN.SSN_PLAN_NO_ROUNDS):        # pipelined rounds | one timestep's rounds at a time | one launch per operator
            with Simulator(None, model=model, dtype="f32", flags=flags) as sim:
                sim.run_steps(300)
                ce = H.cosine_error(sim.data[probes[0]][20:], want[20:])
                assert ce.max() < 1e-3, (flags, np.median(ce), ce.max())


# ---- round 3: the configurations VERDICT r2 listed as untested ------------------------------------------------------------
def test_config2_full_size_block_kernel_matches_oracle(Simulator):
    """BASELINE configs[1] at FULL size - 508 VCOs x 10 000 LIF neurons, ssp_dim 1015 - on the default plan, i.e. the
    whole-block kernel k_ens_block<float,3,4,20,512,3> that the headline number is measured on, against the NumPy oracle of
    the same built model over 200 timesteps (bench.py compares the same pair in every run; this makes it a test)."""
    space = H.make_ssp_space(2, 1015)
    path, vels = H.make_random_path(20.0, limit=0.1, seed=0)
    pm = H.make_pathint_model(space, path, vels, 10000, seed=0)
    model = build(pm.model, n_eval_points=4000)
    assert model.n_neurons == 5080000
    steps = 200
    ref = OracleSimulator(model)
    ref.run_steps(steps)
    want = ref.probe_data(0)
    with Simulator(None, model=model, dtype="f32", block_steps=100) as sim:      # two blocks: the carry between launches is covered
        sim.run_steps(steps)
        got = sim.data[pm.probe]
        c = sim.counters()
    assert c["launches_per_step"] == 0 and (c["block_tpb"], c["block_npt"], c["block_enc_lds"]) == (512, 20, 3)
    assert c["dominant_units_per_launch"] == 5080000 * 100
    ce = H.cosine_error(got[20:], want[20:])
    assert ce.max() < 1e-3 and np.abs(want[20:]).max() > 0.01, ce.max()


def test_config3_full_size_with_learning_matches_oracle(Simulator):
    """BASELINE configs[2] at FULL size (5.53 M neurons: 508 x 10 000 VCO neurons, four 10 150 x 1015 populations, 8 128
    product ensembles; reference run_slam.py:180-235) with a landmark in view from the first timesteps
    (harness.make_config3_model), so that the landmark inputs, the two circular convolutions, PES and Voja are LIVE in the
    window the oracle can follow: f32 fast mode on the default plan (pipelined rounds) within 1e-3 cosine of the oracle over
    150 timesteps; PES-learned decoders, Voja-moved encoders and map recall (definition (i), run_slam.py:263-268) compared."""
    import sspslam_amd.frontend as fe
    sm = H.make_config3_model()
    model = build(sm.model, n_eval_points=4000)
    assert model.n_neurons == 5527000
    am = sm.slam.assomemory
    wb, eb = model.params[am.conn_out].learned_buffer, model.params[am.memory].encoder_buffer
    steps = 150
    ref = OracleSimulator(model)
    ref.run_steps(steps)
    want = ref.probe_data(0)
    W_ref, E_ref, E0 = ref.buf[wb], ref.buf[eb], model.buffers[eb]
    assert np.abs(W_ref).max() > 0 and np.abs(E_ref - E0).max() > 1e-5           # PES and Voja were at work in the window
    with Simulator(None, model=model, dtype="f32") as sim:
        sim.run_steps(steps)
        got = sim.data[sm.probe]
        W_gpu, E_gpu = sim.read_buffer(wb), sim.read_buffer(eb)
        assert sim.counters()["launches_per_step"] <= 8
    ce = H.cosine_error(got[20:], want[20:])
    assert ce.max() < 1e-3, ce.max()
    # learned state: a spike that falls one timestep earlier or later in f32 shifts one neuron's filtered activity, i.e. one
    # column of the decoders, by a few per cent of that column - so the matrices are compared in norm, the recall in cosine
    assert np.linalg.norm(W_gpu - W_ref) < 2e-2 * np.linalg.norm(W_ref), np.linalg.norm(W_gpu - W_ref) / np.linalg.norm(W_ref)
    assert np.linalg.norm((E_gpu - E0) - (E_ref - E0)) < 2e-2 * np.linalg.norm(E_ref - E0)
    rec_g, pos_g = H.map_recall(sm.ssp_space, sm.lm_space, model.params[am.memory], fe.LIF(), W_gpu)
    rec_r, pos_r = H.map_recall(sm.ssp_space, sm.lm_space, model.params[am.memory], fe.LIF(), W_ref)
    seen = np.linalg.norm(rec_r, axis=1) > 1e-3 * np.linalg.norm(rec_r, axis=1).max()
    assert seen.any()
    assert H.cosine_error(rec_g[seen], rec_r[seen]).max() < 1e-3


def test_sharded_pathint_streaming_plan_and_choose_plan(Simulator):
    """BASELINE configs[3]'s shard plan at test size: VCOs of 12 000 neurons do not fit a k_ens_block workgroup (capacity
    10 752), so a rank's shard is stepped by one streaming k_ensarray launch per timestep - also what SSN_PLAN_NO_BLOCK_KERNEL forces.
    ShardedPathIntegration(flags=SSN_PLAN_NO_BLOCK_KERNEL) and choose_plan (bench.py's default at N > 1: both candidates timed, the faster kept)
    must step to the oracle's trajectory."""
    from sspslam_amd.sharding import ShardedPathIntegration
    kw = dict(ssp_dim=7, n=12000, T=10.0, limit=0.2)
    model = build(small_pathint(**kw).model, n_eval_points=1500)
    ref = OracleSimulator(model)
    ref.run_steps(256)
    want = ref.probe_data(0)
    r = ShardedPathIntegration(small_pathint(**kw), 0, 1, dtype="f64", block=128, n_eval_points=1500, flags=PLAN.SSN_PLAN_NO_BLOCK_KERNEL)
    r.prepare(256)
    r.run_steps(256)
    assert r.sim.counters()["launches_per_step"] == 1 and r.sim.counters()["block_tpb"] == 0 and r.sim.counters()["block_members"] == 0
    np.testing.assert_allclose(r.probe_data(), want, atol=1e-9, rtol=0)
    r.close()
    # choose_plan on a shard where both plans exist (n = 600: block kernel vs streaming); the chosen one steps on
    kw = dict(ssp_dim=19, n=600, T=10.0, limit=0.2)
    model = build(small_pathint(**kw).model)
    ref = OracleSimulator(model)
    ref.run_steps(256)
    r = ShardedPathIntegration(small_pathint(**kw), 0, 1, dtype="f32", block=128)
    seconds = r.choose_plan((0, 128), steps=128)
    assert set(seconds) == {0, 128} and all(v > 0 for v in seconds.values())
    assert r._flags == min(seconds, key=lambda f: (seconds[f], f))
    assert (r.sim.counters()["launches_per_step"] == 0) == (r._flags == 0)
    assert r.readout.counters()["launches_per_step"] == 0
    r.prepare(256)
    r.run_steps(256)
    assert H.cosine_error(r.probe_data()[20:], ref.probe_data(0)[20:]).max() < 1e-3
    r.close()


SLAM3D_SHARD_WORKER = r"""
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import torch
import torch.distributed as dist
from sspslam_amd import harness as H
from sspslam_amd.sharding import ShardedSLAM
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
space = H.make_ssp_space(3, ssp_dim=33, rng=np.random.default_rng(3))
path, vels = H.make_random_path(10.0, limit=0.5, seed=2, domain_dim=3)
res = {{}}
for dtype in ("f64", "f32"):
    for turn in range(world):            # ranks share one GPU here: build (rocSOLVER) one after the other
        if turn == rank:
            sm = H.make_slam_model(space, path, vels, n_landmarks=20, pi_n_neurons=100, mem_n_neurons=200, circonv_n_neurons=50,
                                   view_rad=0.6)
            r = ShardedSLAM(sm, rank, world, dtype=dtype)
        dist.barrier()
    r.prepare({steps})
    r.run_steps({steps})
    am = sm.slam.assomemory
    res[dtype] = r.probe_data()
    res[dtype + "_W"], res[dtype + "_E"] = r.learned_decoders(am.conn_out), r.learned_encoders(am.memory)
    res[dtype + "_factored"] = int(any(o["kind"] == "cleanup" and "g_dft" in o for o in r.model.ops))
    r.close()
if rank == 0:
    np.savez({out!r}, **res)
dist.barrier()
dist.destroy_process_group()
"""


def test_two_ranks_of_a_neuron_sharded_3d_slam_on_hip(Simulator, tmp_path):
    """BASELINE configs[4]'s shape in its SHARDED form (configs_untested): the 3-D SLAMNetwork of
    test_slam_3d_matches_oracle (d = 33, 20 landmarks, the reference's 100-points-per-axis clean-up grid = 10^6 rows,
    slam.py:209) split over two ranks - f64: trajectory, gathered PES decoders and Voja encoders equal the UNSHARDED oracle
    run at 1e-9; f32 within the 1e-3 cosine bar with the factored clean-up (half spectrum -> left operand -> MFMA product ->
    two-stage argmax) running inside the two-phase graphs."""
    import subprocess
    import sys
    steps = 60
    script, out = tmp_path / "worker.py", tmp_path / "slam3d.npz"
    script.write_text(SLAM3D_SHARD_WORKER.format(root=ROOT, out=str(out), steps=steps))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29676", str(script)],
                       env=env, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    got = np.load(out)
    space = H.make_ssp_space(3, ssp_dim=33, rng=np.random.default_rng(3))
    path, vels = H.make_random_path(10.0, limit=0.5, seed=2, domain_dim=3)
    sm = H.make_slam_model(space, path, vels, n_landmarks=20, pi_n_neurons=100, mem_n_neurons=200, circonv_n_neurons=50, view_rad=0.6)
    model = build(sm.model)
    ref = OracleSimulator(model)
    ref.run_steps(steps)
    want = ref.probe_data(0)
    am = sm.slam.assomemory
    W_ref = ref.buf[model.params[am.conn_out].learned_buffer]
    E_ref = ref.buf[model.params[am.memory].encoder_buffer]
    assert int(got["f32_factored"]) == 1
    np.testing.assert_allclose(got["f64"], want, atol=1e-9, rtol=0)
    np.testing.assert_allclose(got["f64_W"], W_ref, atol=1e-12, rtol=1e-9)
    np.testing.assert_allclose(got["f64_E"], E_ref, atol=1e-10, rtol=1e-9)
    assert H.cosine_error(got["f32"][20:], want[20:]).max() < 1e-3


def test_sharded_slam_stream_ordered_run_equals_the_host_loop(Simulator):
    """ssn_phase_async / ssn_phase_sync (the whole run enqueued on one stream: per timestep ONE graph launch - [unpack] ->
    updates -> next step up to its exchange -> [pack] - and no host synchronisation) against round 2's loop (a blocking
    ssn_run_phase and a blocking exchange per timestep), one rank, f64: bit-identical trajectories and learned decoders, and
    both equal to the oracle."""
    from sspslam_amd.sharding import ShardedSLAM
    steps = 120
    sm0 = _small_slam(weights_every=None)
    model = build(sm0.model)
    ref = OracleSimulator(model)
    ref.run_steps(steps)
    outs = []
    for host_loop, cycles in ((False, True), (True, True), (False, False), (True, False)):
        sm = _small_slam(weights_every=None)
        r = ShardedSLAM(sm, 0, 1, dtype="f64", host_loop=host_loop, cycles=cycles)
        assert r._stream_ordered() == (not host_loop)
        # the plan pipelined over the exchange (ssn_cycle_steps timesteps as segments around the exchanges, phase 3) serves whole
        # cycles, the per-timestep phases 0 / 2 / 1 the rest: 70 = 4 cycles of 16 + 6, 50 = 3 cycles + 2
        assert r._cycle_steps() == (16 if cycles else 0)
        r.prepare(steps)
        r.run_steps(70)
        r.run_steps(steps - 70)                    # two runs: the sequence restarts cleanly
        outs.append((r.probe_data(), r.learned_decoders(sm.slam.assomemory.conn_out)))
        with pytest.raises(nengo.SimulationError, match="prepare"):
            r.run_steps(5)                          # past the prepared window: refused before anything is enqueued
        if cycles and host_loop:                    # inside a cycle the per-timestep phases are refused
            r.sim.reset()
            r.prepare(40)
            r.sim.run_phase(3)
            with pytest.raises(nengo.SimulationError, match="cycle is under way"):
                r.sim.run_phase(0)
        r.close()
    for o in outs[1:]:
        np.testing.assert_array_equal(outs[0][0], o[0])
        np.testing.assert_array_equal(outs[0][1], o[1])
    np.testing.assert_allclose(outs[0][0], ref.probe_data(0), atol=1e-9, rtol=0)


def test_split_vco_members_match_oracle(Simulator):
    """Split ensembles of the whole-block kernel (flag 1073741824): an array with fewer VCOs than the GPU has
    CUs - a 4- or 8-GPU shard of BASELINE config 2 - is stepped by 2 or 4 member workgroups per VCO that exchange their four
    partial sums every timestep (sentinel words in three rotating buffers).  Against the oracle (1e-3 cosine) and against the
    unsplit kernel (the sums are re-associated over the members: rounding only), members of unequal size (n not a multiple of
    4 P), several launches in a run (the exchange words are reset at every kernel boundary), the planner's own choice of P,
    and the cases it must leave alone (f64; a fifth decoded row; more VCOs than CUs)."""
    SPLIT = PLAN.SSN_PLAN_SPLIT_BLOCK
    os.environ.pop("SSN_BLOCK_SPLIT", None)
    os.environ.pop("SSN_BLOCK_SPLIT_CUS", None)
    try:
        for n, force, expect in ((5203, "2", 2), (5203, "4", 4), (9000, None, 4), (2600, None, 2)):
            pm = small_pathint(ssp_dim=19, n=n, T=10.0, limit=0.2)          # (ssp_dim 19 -> d = 7: 4 VCOs)
            model = build(pm.model, n_eval_points=600)
            ref = OracleSimulator(model)
            ref.run_steps(300)
            want = ref.probe_data(0)
            with Simulator(None, model=model, dtype="f32", block_steps=100) as sim:
                sim.run_steps(300)
                plain = sim.data[pm.probe]
                assert sim.counters()["block_members"] == 1
            if force:
                os.environ["SSN_BLOCK_SPLIT"] = force
            with Simulator(None, model=model, dtype="f32", flags=SPLIT, block_steps=100) as sim:
                os.environ.pop("SSN_BLOCK_SPLIT", None)
                sim.run_steps(130)                   # 100 + 30, then 100 + 70: four launches, two of them short
                sim.run_steps(170)
                got = sim.data[pm.probe]
                c = sim.counters()
            assert c["block_members"] == expect and c["launches_per_step"] == 0, c
            assert H.cosine_error(got[20:], want[20:]).max() < 1e-3
            assert np.abs(got - plain).max() < 2e-4 * np.abs(plain).max()
        # left alone: f64; a probe that keeps the fifth decoded row; more VCOs than (pretended) CUs
        pm = small_pathint(ssp_dim=19, n=5203, T=10.0, limit=0.2)
        model = build(pm.model, n_eval_points=600)
        with Simulator(None, model=model, dtype="f64", flags=SPLIT, block_steps=100) as sim:
            assert sim.counters()["block_members"] in (0, 1)
        os.environ["SSN_BLOCK_SPLIT_CUS"] = "7"       # 4 VCOs x 2 members > 7 "CUs"
        with Simulator(None, model=model, dtype="f32", flags=SPLIT, block_steps=100) as sim:
            assert sim.counters()["block_members"] == 1
        os.environ.pop("SSN_BLOCK_SPLIT_CUS", None)
        pm5 = small_pathint(ssp_dim=19, n=5203, T=10.0, limit=0.2)
        with pm5.model:
            nengo.Probe(pm5.pathintegrator.oscillators.output, synapse=None)
        with Simulator(None, model=build(pm5.model, n_eval_points=600), dtype="f32", flags=SPLIT, block_steps=100) as sim:
            assert sim.counters()["block_members"] == 1
    finally:
        os.environ.pop("SSN_BLOCK_SPLIT", None)
        os.environ.pop("SSN_BLOCK_SPLIT_CUS", None)
