"""Instrument of the map-recall tests (tests/test_recall.py on the CPU, tests/test_gpu_recall.py on the MI355X).

* ``recall_f64``     the recall in float64 NumPy, written from the formula (include/ssn.h, "Recall of a learned associative memory"),
                     not from harness.py.
* ``bound``          a first-order rounding bound B per output element for unit roundoff u (2^-24 for the f32 kernels, 2^-53 for the
                     parity kernels):
                         dJ = |s| (d_key + 2) u (|V| . |E|) + 2u (|s V.E| + |bias|) + u |J|
                         da = rate(J + dJ) - rate(J - dJ) + 4u a         (the rate function is monotone: a neuron at its threshold is
                                                                          priced with the whole jump it can make)
                         B  = |W| . da + (n + 2) u |W| . a
* ``check``          a device passes when |q_dev - q_f64| <= B everywhere; the inputs must satisfy B <= 1e-2 max_r |q[l][r]| for every
                     key row l, so that the bound cannot hide a wrong kernel.  Prints the worst err / B and the worst B / max|q|.
* ``emulate_f32``    the NumPy-f32 restatement of the f32 kernels (k-ordered products, 256-neuron partial sums added in order), with
                     switches that turn it into each of the wrong devices tests/test_recall.py must see fail.
* ``synthetic_state`` / ``memory_network``   the inputs: a made-up learned state for the CPU tests, a small AssociativeMemory driven
                     by table nodes for the GPU tests.
"""
import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53
SHAPES = [(100, 7, 5), (1100, 55, 5), (1030, 130, 129)]      # (n, d_key, d_val): no multiple of any tile, d_key != d_val
LIF = dict(type="lif", tau_rc=0.02, tau_ref=0.002, amplitude=1.0)
CONDITION = 1e-2
CHUNK = 256


def rate(J, neuron):
    J = np.asarray(J, dtype=np.float64)
    if neuron["type"] == "relu":
        return neuron["amplitude"] * np.maximum(J, 0.0)
    out = np.zeros_like(J)
    on = J > 1.0
    out[on] = neuron["amplitude"] / (neuron["tau_ref"] + neuron["tau_rc"] * np.log1p(1.0 / (J[on] - 1.0)))
    return out


def scale_of(gain, mode):
    assert mode in ("reference", "network")
    return np.asarray(gain, dtype=np.float64) if mode == "reference" else np.ones(len(gain))


def recall_f64(keys, E, W, gain, bias, neuron, mode):
    """q (L, d_val) from keys (L, d_key), E (n, d_key), W (d_val, n), gain and bias (n)."""
    keys, E, W = (np.asarray(x, dtype=np.float64) for x in (keys, E, W))
    J = scale_of(gain, mode)[None, :] * (keys @ E.T) + np.asarray(bias, dtype=np.float64)[None, :]
    return rate(J, neuron) @ W.T


def bound(keys, E, W, gain, bias, neuron, mode, u):
    """(q, B): the float64 recall and the bound on a device's error for unit roundoff u."""
    keys, E, W = (np.asarray(x, dtype=np.float64) for x in (keys, E, W))
    s, b = scale_of(gain, mode)[None, :], np.asarray(bias, dtype=np.float64)[None, :]
    n, d_key = E.shape
    dot = keys @ E.T
    J = s * dot + b
    dJ = np.abs(s) * (d_key + 2) * u * (np.abs(keys) @ np.abs(E).T) + 2 * u * (np.abs(s * dot) + np.abs(b)) + u * np.abs(J)
    a = rate(J, neuron)
    da = rate(J + dJ, neuron) - rate(J - dJ, neuron) + 4 * u * a
    aW = np.abs(W).T
    return a @ W.T, da @ aW + (n + 2) * u * (a @ aW)


def condition(q, B):
    """Worst B / max_r |q[l][r]| over the key rows."""
    return float(np.max(np.max(B, axis=1) / np.max(np.abs(q), axis=1)))


def check(q_dev, keys, E, W, gain, bias, neuron, mode, u, label=""):
    """Assert the condition on the inputs and |q_dev - q_f64| <= B; returns the worst err / B."""
    q, B = bound(keys, E, W, gain, bias, neuron, mode, u)
    q_dev = np.asarray(q_dev)
    assert q_dev.shape == q.shape and q_dev.dtype == np.float64, (label, q_dev.shape, q_dev.dtype, q.shape)
    assert np.all(np.max(np.abs(q), axis=1) > 0), f"{label}: a key row recalls nothing - the condition cannot be met"
    cond = condition(q, B)
    err = np.abs(q_dev - q)
    worst = float(np.max(err / B)) if np.all(B > 0) else float("inf") if np.any(err > B) else 0.0
    print(f"recall {label}: mode {mode} u = 2^{int(np.log2(u))} worst err / B = {worst:.3e}, worst B / max|q| = {cond:.3e}, max |q| = {np.max(np.abs(q)):.3e}")
    assert cond <= CONDITION, f"{label}: the inputs violate B <= {CONDITION} max|q| ({cond:.3e}): choose another seed"
    assert np.all(np.isfinite(q_dev)), label
    assert np.all(err <= B), f"{label}: |q_dev - q_f64| exceeds B by a factor of {worst:.3e}"
    return worst


# -- the NumPy-f32 restatement and its wrong variants -------------------------------------------------------------------------------
FAULTS = ("modes_swapped", "ragged_tile_dropped", "previous_W", "W_rows_cols_swapped", "threshold_at_zero", "tau_ref_dropped",
          "key_rows_exchanged", "padding_ones", "row_shifted", "partial_twice")


def emulate_f32(keys, E, W, gain, bias, neuron, mode, fault=None, W_prev=None):
    """The f32 kernels in NumPy float32: J from a float32 product, scale, bias and rate in float32, the decoder product as partial
    sums of 256 neurons added in ascending order.  ``fault``: one of FAULTS, the named mistake built in."""
    assert fault is None or fault in FAULTS
    f = np.float32
    keys, E, W = (np.asarray(x, dtype=f) for x in (keys, E, W))
    n, d_key = E.shape
    d_val = W.shape[0]
    if fault == "modes_swapped":
        mode = "network" if mode == "reference" else "reference"
    s, b = scale_of(gain, mode).astype(f), np.asarray(bias).astype(f)
    if fault == "key_rows_exchanged":
        keys = keys.copy()
        keys[[0, 1]] = keys[[1, 0]]
    if fault == "padding_ones":      # both operands padded to the 32-column slab with ones, and the padding multiplied
        pad = -d_key % 32 or 32
        keys = np.hstack([keys, np.ones((keys.shape[0], pad), dtype=f)])
        E = np.hstack([E, np.ones((n, pad), dtype=f)])
    if fault == "previous_W":
        W = np.asarray(W_prev, dtype=f)
    if fault == "W_rows_cols_swapped":
        W = np.ascontiguousarray(W).reshape(n, d_val).T
    J = (s[None, :] * (keys @ E.T).astype(f) + b[None, :]).astype(f)
    amp, tau_rc, tau_ref = f(neuron["amplitude"]), f(neuron["tau_rc"]), f(0.0 if fault == "tau_ref_dropped" else neuron["tau_ref"])
    if neuron["type"] == "relu":
        a = amp * np.maximum(J, f(0))
    else:
        a = np.zeros_like(J)
        if fault == "threshold_at_zero":
            on = J > 0
            a[on] = amp / (tau_ref + tau_rc * np.log1p(f(1) / np.maximum(np.abs(J[on] - f(1)), f(1e-6))))
        else:
            on = J > 1
            a[on] = amp / (tau_ref + tau_rc * np.log1p(f(1) / (J[on] - f(1))))
    a = a.astype(f)
    n_used = n - n % 64 if fault == "ragged_tile_dropped" else n
    q = np.zeros((keys.shape[0], d_val), dtype=f)
    for c0 in range(0, n_used, CHUNK):
        c1 = min(c0 + CHUNK, n_used)
        part = (a[:, c0:c1] @ W[:, c0:c1].T).astype(f)
        q = (q + part).astype(f)
        if fault == "partial_twice" and c0 == 0:
            q = (q + part).astype(f)
    if fault == "row_shifted":
        q = np.roll(q, 1, axis=1)
    return q.astype(np.float64)


# -- inputs -------------------------------------------------------------------------------------------------------------------------
def unit_rows(rng, rows, d):
    x = rng.standard_normal((rows, d))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def lif_gain_bias(max_rates, intercepts, neuron=LIF):
    """nengo's LIF.gain_bias: the rate is max_rates at x = 1 and zero at x = intercepts."""
    x = 1.0 / (1 - np.exp((neuron["tau_ref"] - 1.0 / max_rates) / neuron["tau_rc"]))
    gain = (1 - x) / (intercepts - 1.0)
    return gain, 1 - gain * intercepts


def synthetic_state(n, d_key, d_val, L=10, seed=0):
    """A made-up learned state: random unit keys, 5 encoders turned to each key (what Voja does), decoders of about 1e-4 that
    map the neurons of a key to a value of its own (what PES does) over a small random background; W_prev is the state a
    sample earlier.  -> dict(keys, E, W, W_prev, gain, bias)."""
    rng = np.random.RandomState(seed)
    keys = unit_rows(rng, L, d_key)
    enc = unit_rows(rng, n, d_key)
    owner = np.full(n, -1)
    for l in range(L):
        idx = np.arange(5 * l, 5 * l + 5) % n
        e = keys[l] + 0.1 * rng.standard_normal((idx.size, d_key)) / np.sqrt(d_key)
        enc[idx] = e / np.linalg.norm(e, axis=1, keepdims=True)
        owner[idx] = l
    gain, bias = lif_gain_bias(rng.uniform(200, 400, n), np.full(n, 0.1))
    E = enc * gain[:, None]
    values = unit_rows(rng, L, d_val)
    W = 1e-4 * 0.02 * rng.standard_normal((d_val, n))
    for l in range(L):
        W[:, owner == l] += 1e-4 * values[l][:, None]
    W_prev = W * 0.9 + 1e-4 * 0.02 * rng.standard_normal((d_val, n))
    return dict(keys=keys, E=E, W=W, W_prev=W_prev, gain=gain, bias=bias)


N_KEYS = 10
STEPS, EVERY = 200, 50


def memory_network(n, d_key, d_val, neuron_type=None, voja=True, seed=3, dt=0.001, map_modes=("reference", "network"), L=N_KEYS):
    """An AssociativeMemory alone, driven by table nodes: every 20 timesteps the next of L key / value pairs, learning on.  With
    ``Probe(conn_out, "weights")`` and (Voja on) ``Probe(conn_in.learning_rule, "scaled_encoders")`` every EVERY timesteps and one
    MapProbe per mode beside them.  -> (network, dict(memory, keys, values, w_probe, e_probe, map_probes))."""
    from sspslam_amd import frontend as nengo
    from sspslam_amd import MapProbe
    from sspslam_amd.networks.associativememory import AssociativeMemory
    rng = np.random.RandomState(seed)
    keys, values = unit_rows(rng, L, d_key), unit_rows(rng, L, d_val)
    which = lambda t: int(round(t / dt) - 1) // 20 % L      # noqa: E731
    net = nengo.Network(seed=seed)
    if neuron_type is not None:
        net.config[nengo.Ensemble].neuron_type = neuron_type
    with net:
        key_in = nengo.Node(lambda t: keys[which(t)], label="key")
        val_in = nengo.Node(lambda t: values[which(t)], label="value")
        learn = nengo.Node(lambda t: np.zeros(1), label="learn")
        mem = AssociativeMemory(n, d_key, d_val, 0.1, voja_learning_rate=5e-3, pes_learning_rate=2e-2, voja=voja, seed=seed)
        nengo.Connection(key_in, mem.key_input, synapse=None)
        nengo.Connection(val_in, mem.value_input, synapse=None)
        nengo.Connection(learn, mem.learning, synapse=None)
        out = dict(memory=mem, keys=keys, values=values)
        out["w_probe"] = nengo.Probe(mem.conn_out, "weights", sample_every=EVERY * dt)
        out["e_probe"] = nengo.Probe(mem.conn_in.learning_rule, "scaled_encoders", sample_every=EVERY * dt) if voja else None
        out["map_probes"] = {m: MapProbe(mem, keys, sample_every=EVERY * dt, mode=m) for m in map_modes}
        out["recall_probe"] = nengo.Probe(mem.recall, synapse=0.01)
    return net, out


def recall_keys(keys, L, seed=11):
    """L keys for Simulator.recall on a memory trained with ``keys``: each a trained key, slightly turned."""
    rng = np.random.RandomState(seed)
    k = keys[np.arange(L) % keys.shape[0]] + 0.2 * unit_rows(rng, L, keys.shape[1])
    return k / np.linalg.norm(k, axis=1, keepdims=True)
