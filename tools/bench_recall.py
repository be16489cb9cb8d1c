"""Map recall at the shapes of config 3 (memory of 10 150 neurons, d = 1015, L = 10 landmark SPs padded out to 50 keys): the
device recall (csrc/ssn_recall.hip behind MapProbe / Simulator.recall) against the only way there was before it - the two buffer
probes read back at every sample and harness.map_recall_learned on the host.

usage: python tools/bench_recall.py [--steps N] [--every SECONDS] [--repeats R] [--keys L] [--skip-host]

Three runs of the same SLAM network (harness.make_config3_model, f32, one GPU), each `--repeats` times `--steps` timesteps after a
warm-up of the same length (the first call pays graph capture and, with the buffer probes, the first page faults of the host arrays):
  (0) no learned-signal probe at all
  (1) a MapProbe on the keys at sample_every = --every
  (2) Probe(conn_out, "weights") + Probe(conn_in.learning_rule, "scaled_encoders") at the same rate, then map_recall_learned's
      arithmetic on the host for every sample
Reported: wall time per run (median, min, max), the cost per sample over run (0), the kernel time of one recall from HIP events
(2 warm-up calls, median and minimum of 20), the fraction of HBM bandwidth that is for the bytes of E and W streamed once (against
the 8.0 TB/s of the data sheet and the 6.3 TB/s a copy kernel reaches), host bytes kept per sample both ways, and the device answer
against the float64 recall under the rounding bound B of tests/recall_checks.py."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import recall_checks as rc
from sspslam_amd import MapProbe, frontend as nengo, harness as H
from sspslam_amd.modelcache import cached_build
from sspslam_amd.simulator import Simulator


def fmt(x, unit="s"):
    x = np.asarray(x)
    return "median %.4f %s (min %.4f, max %.4f, %d runs)" % (np.median(x), unit, x.min(), x.max(), len(x))


def network(kind, keys, every, T):
    sm = H.make_config3_model(T=max(20.0, T))
    mem = sm.slam.assomemory
    probes = {}
    with sm.model:
        if kind == "map":
            probes["map"] = MapProbe(mem, keys, sample_every=every)
        elif kind == "buffers":
            probes["w"] = nengo.Probe(mem.conn_out, "weights", sample_every=every)
            probes["e"] = nengo.Probe(mem.conn_in.learning_rule, "scaled_encoders", sample_every=every)
    return sm, mem, probes


def all_keys(sm, L):
    """The 10 landmark SPs and, up to L rows, slightly turned copies of them (config 3 has 10 landmarks; the figures' scripts use 50)."""
    v = np.asarray(sm.lm_space.vectors, dtype=float)
    if L <= v.shape[0]:
        return v[:L]
    extra = rc.recall_keys(v, L - v.shape[0])
    return np.vstack([v, extra * np.linalg.norm(v, axis=1).mean()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--every", type=float, default=0.1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--keys", type=int, default=50)
    ap.add_argument("--skip-host", action="store_true", help="leave out run (2), which keeps 165 MB of host memory per sample")
    args = ap.parse_args()
    dt = 0.001
    T = (args.repeats + 1) * args.steps * dt + 0.1
    keys = all_keys(H.make_config3_model(T=20.0), args.keys)
    per_run = int(round(args.steps * dt / args.every))
    print("config 3 memory: n = 10150, d_key = d_val = 1015, L = %d keys; %d timesteps per run, a sample every %g s (%d per run)" % (
        keys.shape[0], args.steps, args.every, per_run), flush=True)
    walls = {}
    for kind in ("none", "map") + (() if args.skip_host else ("buffers",)):
        t0 = time.perf_counter()
        sm, mem, probes = network(kind, keys, args.every, T)
        model = cached_build(sm.model, dt=dt)
        print("run (%s): built in %.1f s (cache: %s)" % (kind, time.perf_counter() - t0, model.stats.get("cache")), flush=True)
        be = model.params[mem.memory]
        neuron = nengo.LIF()
        with Simulator(None, model=model, dtype="f32") as sim:
            wall = []
            for r in range(args.repeats + 1):
                t0 = time.perf_counter()
                sim.run_steps(args.steps)
                host_recalled = None
                if kind == "buffers":          # what the figures' scripts do with the two probes: every sample through the host function
                    Ws, Es = sim.data[probes["w"]], sim.data[probes["e"]]
                    host_recalled = np.stack([neuron.rates(keys @ Es[i].T, be.gain, be.bias) @ Ws[i].T for i in range(Ws.shape[0])])
                    kept = Ws[0].nbytes + Es[0].nbytes
                wall.append(time.perf_counter() - t0)
                del host_recalled
                if r < args.repeats:
                    sim.clear_probe_data()
            walls[kind] = np.array(wall[1:])
            print("  wall per run of %d timesteps: %s; first (warm-up) run %.3f s" % (args.steps, fmt(walls[kind]), wall[0]), flush=True)
            if kind == "map":
                frames = sim.data[probes["map"]]
                print("  MapProbe: %d samples of shape %s, %d bytes of host memory kept per sample; recalls took %.4f s of host time in all, their kernels %.3f ms"
                      % (frames.shape[0], frames.shape[1:], frames[0].nbytes, sim.recall_seconds, sim.recall_kernel_ms))
                # one recall on demand: kernel time from HIP events, and the answer against float64
                for _ in range(2):
                    sim.recall(mem, keys)
                kern, wall1 = [], []
                for _ in range(20):
                    t0 = time.perf_counter()
                    q = sim.recall(mem, keys)
                    wall1.append(1e3 * (time.perf_counter() - t0))
                    kern.append(sim.recall_info(mem)["last_kernel_ms"])
                info = sim.recall_info(mem)
                streamed = 4.0 * (info["n"] * info["d_key"] + info["d_val"] * info["n"])
                k = np.median(kern)
                print("  one recall, kernels alone: %s; Simulator.recall wall %s" % (fmt(kern, "ms"), fmt(wall1, "ms")))
                print("  plan: %s" % {f: info[f] for f in ("padded_keys", "chunk", "n_chunks", "chunks_per_pass", "scratch_bytes", "dec_neuron_major", "last_launches")})
                print("  E and W streamed once: %.1f MB -> %.2f TB/s, %.3f of the 8.0 TB/s data-sheet peak, %.3f of the 6.3 TB/s a copy reaches" % (
                    streamed / 1e6, streamed / (k * 1e-3) / 1e12, streamed / (k * 1e-3) / 8.0e12, streamed / (k * 1e-3) / 6.3e12))
                print("  a sample against the %g timesteps between samples at 97.6 us per timestep (%.2f ms): kernels %.4f of that, wall %.4f" % (
                    args.every / dt, args.every / dt * 0.0976, k / (args.every / dt * 0.0976), np.median(wall1) / (args.every / dt * 0.0976)))
                E, W = sim.read_buffer(be.encoder_buffer), sim.read_buffer(model.params[mem.conn_out].learned_buffer)
                for mode in ("reference", "network"):
                    qd = sim.recall(mem, keys, mode=mode)
                    qf, B = rc.bound(keys, E, W, be.gain, be.bias, be.neuron, mode, rc.U32)
                    live = np.max(np.abs(qf), axis=1) > 0
                    err = np.abs(qd - qf)
                    print("  mode %-9s against float64 after %d timesteps: max |q| = %.3e, worst err / B = %.3e (%s), worst B / max|q| over the %d rows that recall "
                          "anything = %.3e (the tests' condition asks <= %.0e)" % (
                              mode, sim.n_steps, np.abs(qf).max(), float(np.max(err[B > 0] / B[B > 0])) if np.any(B > 0) else 0.0,
                              "within B everywhere" if np.all(err <= B) else "OUTSIDE B", int(live.sum()),
                              float(np.max(np.max(B[live], axis=1) / np.max(np.abs(qf[live]), axis=1))) if live.any() else float("nan"), rc.CONDITION), flush=True)
            if kind == "buffers":
                print("  buffer probes: %.1f MB of host memory kept per sample (two float64 matrices), %d samples per run through the host function" % (
                    kept / 1e6, per_run), flush=True)
    base = np.median(walls["none"])
    for kind in walls:
        if kind != "none":
            extra = (np.median(walls[kind]) - base) / max(1, per_run)
            print("run (%s) over run (none): %+.4f s per run, %.2f ms per sample = %.2f x the %.2f ms of device time between two samples" % (
                kind, np.median(walls[kind]) - base, 1e3 * extra, 1e3 * extra / (args.every / dt * 0.0976), args.every / dt * 0.0976))


if __name__ == "__main__":
    main()
