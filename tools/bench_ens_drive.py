"""Cost of neuron-input drive columns in the per-timestep ensemble-array kernel: bench_ens.py's model (the oscillator array
of SLAM config 3 by default: 508 x 10 000 LIF neurons, din 3, dout 5, nengo-default gains / biases, ~10 % of the neurons
spiking per step, random decoders) with m = 0, 1, 2 drive columns.  m = 0 is the plain k_ensarray; every case runs on a launch
of its own (SSN_PLAN_ENS_OWN_LAUNCH), a driven array always does.  The column scalars are 0 (the gates are open: the array
spikes as it does undriven, and the weights are streamed all the same); the cases alternate, `reps` times.
usage: bench_ens_drive.py [K] [n] [steps] [reps] [m ...]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from sspslam_amd.builder import BuiltModel
from sspslam_amd.simulator import Simulator, SSN_PLAN_ENS_OWN_LAUNCH
import sspslam_amd.frontend as fe

K = int(sys.argv[1]) if len(sys.argv) > 1 else 508
n = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 300
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
ms = [int(v) for v in sys.argv[5:]] or [0, 1, 2]
rng = np.random.RandomState(0)
lif = fe.LIF()
enc = rng.randn(K, n, 3); enc /= np.linalg.norm(enc, axis=2, keepdims=True)
gain, bias = lif.gain_bias(rng.uniform(200, 400, (K, n)), rng.uniform(-1, 0.9, (K, n)))
enc = (enc * (gain / np.sqrt(2))[:, :, None]).transpose(0, 2, 1).copy()
th = rng.uniform(0, 2 * np.pi, K)
x = np.stack([np.cos(th), np.sin(th), rng.uniform(-0.3, 0.3, K)], 1)
dec = rng.randn(K, 5, n) * 1e-4
nd = dict(type="lif", tau_rc=0.02, tau_ref=0.002, min_voltage=0.0, amplitude=1.0)
probe = object()


def model(m_cols):
    m = BuiltModel(0.001)
    m.sig_size = 3 * K + 5 * K + 4                       # x | decoded rows | column scalars (zeros)
    m.sig_init = np.zeros(m.sig_size); m.sig_init[:3 * K] = x.reshape(-1)
    idx = (3 * K + np.arange(5 * K)).reshape(K, 5).astype(np.int32)
    b = [m.add_buffer(a, nm, role) for a, nm, role in ((enc, "enc", "param"), (bias, "bias", "param"), (dec, "dec", "param"), (idx, "idx", "index"),
                                                       (np.zeros((K, n)), "v", "state"), (np.zeros((K, n)), "r", "state"))]
    op = dict(kind="ensarray", x=0, K=K, n=n, din=3, dout=5, enc=b[0], bias=b[1], dec=b[2], dst_idx=b[3], v=b[4], r=b[5], neuron=nd,
              level=0, label="big", k_lo=0, k_total=K)
    if m_cols:
        src = np.tile(8 * K + np.arange(m_cols, dtype=np.int32), (K, 1))
        op["drive"] = {"m": m_cols, "w": m.add_buffer(np.full((K, m_cols, n), -10.0), "drive"),
                       "src": m.add_buffer(src, "drive_src", "index")}
    m.ops = [op]
    m.probes = [dict(probe=probe, src=3 * K, width=5 * K, every=1)]
    return m


times, outs = {m_cols: [] for m_cols in ms}, {}
for rep in range(reps):
    for m_cols in ms:
        sim = Simulator(None, model=model(m_cols), dtype="f32", flags=SSN_PLAN_ENS_OWN_LAUNCH)
        sim.run_steps(100)                       # reach stationary spiking
        sim.run_steps(steps, profile=True, collect=False)
        c = sim.counters()
        us = c["dominant_ms_total"] / c["dominant_launches"] * 1e3
        times[m_cols].append(us)
        print("rep %d m = %d: k_ensarray avg %.2f us (events, %d launches); %.1f us per timestep" %
              (rep, m_cols, us, c["dominant_launches"], c["last_run_ms"] / steps * 1e3), flush=True)
        sim._collect()
        outs.setdefault(m_cols, sim.data[probe])
        sim.close()
for m_cols in ms:
    t = times[m_cols]
    med = float(np.median(t))
    print("m = %d: median %.2f us, runs %s; %d algorithmic bytes per neuron-step -> %.0f GB/s" %
          (m_cols, med, ["%.2f" % v for v in t], 52 + 4 * m_cols, K * n * (52 + 4 * m_cols) / med / 1e3))
for m_cols in ms[1:]:
    print("m = %d output identical to m = %d:" % (m_cols, ms[0]), np.array_equal(outs[m_cols], outs[ms[0]]))
