#!/usr/bin/env python3
"""Path integration on the MI355X backend with the command line of the reference's
``experiments/run_pathint.py`` (same option names, defaults and result file; ``--backend mi355x`` /
``mi355x-f64`` in place of ``cpu`` / ``ocl``).

    python examples/run_pathint.py --ssp-dim 1015 --pi-n-neurons 10000 --T 20 --save

Writes ``<save-dir>/pi_backend_<backend>..._sspdim_<d>_pinneurons_<n>_T_<T>_limit_<limit>_seed_<seed>.npz`` with the
field names ``plot_trials_2d.py`` of the reference reads (ts, path, real_ssp, pi_sim_out, pi_sims, pi_path, pi_error,
elapsed_time, ...).  Only plotting (``--plot``) and the Loihi back ends are not provided.

``--spike-probes M`` adds the neuron probes of the reference's ``experiments/run_pathint_gif.py``
(``nengo.Probe(pathintegrator.oscillators.ea_ensembles[k].neurons[:500], synapse=None, sample_every=100*dt)``) for the
oscillators k = 1 .. M; with ``--save`` their samples go to ``<result file minus .npz>_spikes.npz`` as ``vco_n<k>``, with
the sample times ``ts``.

``--gate-oscillators T0 T1`` inhibits every oscillator for T0 < t <= T1 through ``oscillators.add_neuron_input()`` (a
weight of -10 on every neuron, the gate of the reference's ``AdditiveInputGatedMemory``; at the oscillators' default
rates of up to 400 Hz that thins their spikes out, it does not silence every neuron).

``--save-maps N`` makes the similarity maps every figure script of the reference ends with (``sim_grid`` of
``run_pathint_gif.py:231-232``: every 10th probed sample against the N x N sample grid, squared, raw rows) through
``harness.similarity_frames`` - NumPy, or ``k_decode_map`` on the GPU with ``--decode-backend hip`` - prints the map seconds next to
the decode seconds and, with ``--save``, writes them to ``<result file minus .npz>_maps.npz`` (``ts``, ``sim_grid``).
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sspslam_amd.frontend as nengo          # noqa: E402  (the nengo-shaped object model; fe.install_as_nengo() for `import nengo`)
from sspslam_amd import harness as H           # noqa: E402
from sspslam_amd.simulator import Simulator    # noqa: E402
from sspslam_amd.sspspace import HexagonalSSPSpace, RandomSSPSpace   # noqa: E402


def parse(argv=None):
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--backend", default="mi355x", type=str, help="mi355x (float32) or mi355x-f64 (parity mode)")
    p.add_argument("--path-data", default=None, type=str, help="The path and name to path data.")
    p.add_argument("--data-dt", default=0.001, type=float)
    p.add_argument("--domain-dim", default=2, type=int, help="Dim of path to generate")
    p.add_argument("--limit", default=0.1, type=float)
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--T", default=20, type=float, help="The total simulation time in seconds.")
    p.add_argument("--pi-n-neurons", default=800, type=int, help="Number of neurons per VCO population in the PI net.")
    p.add_argument("--ssp-dim", default=97, type=int)
    p.add_argument("--n-scales", default=0, type=int)
    p.add_argument("--n-rotates", default=3, type=int)
    p.add_argument("--length-scale", default=0.2, type=float)
    p.add_argument("--save", action="store_true")
    p.add_argument("--use-rand", action="store_true")
    p.add_argument("--neuron-type", default="lif", help="lif, lifrate, relu")
    p.add_argument("--save-dir", default="data")
    p.add_argument("--save-name-extra", default="")
    p.add_argument("--n-eval-points", default=0, type=int,
                   help="decoder-solve evaluation points per ensemble; 0 = nengo's default max(1500, 2 n)")
    p.add_argument("--spike-probes", default=0, type=int,
                   help="probe neurons[:500] of the oscillators 1..M every 100 steps (run_pathint_gif.py probes 1, 2 and 3)")
    p.add_argument("--gate-oscillators", default=None, type=float, nargs=2, metavar=("T0", "T1"),
                   help="inhibit the oscillators' neurons (weight -10, through add_neuron_input()) for T0 < t <= T1")
    p.add_argument("--decode-backend", default="numpy", choices=["numpy", "hip"],
                   help="grid decode of the probed trajectory: NumPy on the host, or the GPU grid decoder (decoding.GridDecoder)")
    p.add_argument("--decode-table", default=None, choices=["host", "device"],
                   help="with --decode-backend hip: the decoder's sample table encoded on the host and uploaded, or encoded on the "
                        "GPU from the sample points; prints the decoder-creation seconds")
    p.add_argument("--encode-backend", default=None, choices=["numpy", "hip"],
                   help="encode the true path (real_ssp of the metrics) with NumPy or on the GPU (encoding.SSPEncoder); prints the "
                        "encode seconds")
    p.add_argument("--decode-refine", action="store_true",
                   help="also decode with 'grid-refine' (Newton steps from the grid point) and print both position errors")
    p.add_argument("--save-maps", default=0, type=int, metavar="N",
                   help="similarity maps of every 10th probed sample over the N x ... x N sample grid (sim_grid of "
                        "run_pathint_gif.py: squared, raw rows), made by --decode-backend; with --save written to <result>_maps.npz")
    return p.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    dt, tau, radius = 0.001, 0.05, 1.0
    if args.path_data is None:
        T, domain_dim = args.T, args.domain_dim
        path, vels = H.make_random_path(T, dt=dt, limit=args.limit, seed=args.seed, domain_dim=domain_dim, radius=radius)
    else:
        path, vels = H.load_path(args.path_data, data_dt=args.data_dt, dt=dt, radius=radius)
        T, domain_dim = path.shape[0] * dt, path.shape[1]
    bounds = radius * np.tile([-1.0, 1.0], (domain_dim, 1))
    if args.use_rand:
        space = RandomSSPSpace(domain_dim, ssp_dim=args.ssp_dim, domain_bounds=bounds, length_scale=args.length_scale,
                               rng=np.random.default_rng(args.seed))
    elif args.n_scales > 0:
        space = HexagonalSSPSpace(domain_dim, n_scales=args.n_scales, n_rotates=args.n_rotates, domain_bounds=bounds,
                                  length_scale=args.length_scale)
    else:
        space = HexagonalSSPSpace(domain_dim, ssp_dim=args.ssp_dim, domain_bounds=bounds, length_scale=args.length_scale)
    neuron_type = {"lif": nengo.LIF, "lifrate": nengo.LIFRate, "relu": nengo.RectifiedLinear}[args.neuron_type]()
    pm = H.make_pathint_model(space, path, vels, args.pi_n_neurons, tau=tau, neuron_type=neuron_type, seed=args.seed, dt=dt)
    skip = 100
    spike_probes = {}
    oscillators = pm.pathintegrator.oscillators.ea_ensembles
    if not 0 <= args.spike_probes < len(oscillators):
        raise SystemExit("--spike-probes %d: the path integrator has oscillators 1 .. %d" % (args.spike_probes, len(oscillators) - 1))
    with pm.model:
        for k in range(1, args.spike_probes + 1):
            spike_probes[k] = nengo.Probe(oscillators[k].neurons[:500], synapse=None, sample_every=skip * dt)
    if args.gate_oscillators is not None:
        g0, g1 = args.gate_oscillators
        array = pm.pathintegrator.oscillators
        with pm.model:
            gate = nengo.Node(lambda t: 1.0 if g0 < t <= g1 else 0.0, label="oscillator_gate")
            nengo.Connection(gate, array.add_neuron_input(), transform=-10.0 * np.ones((array.n_neurons, 1)), synapse=None)
    dtype = "f64" if args.backend.endswith("f64") else "f32"
    t0 = time.time()
    sim = Simulator(pm.model, dt=dt, dtype=dtype, n_eval_points=args.n_eval_points or None)
    build_time = time.time() - t0
    start, start2 = time.thread_time(), time.time()
    with sim:
        sim.run(T)
        elapsed_thread_time, elapsed_time = time.thread_time() - start, time.time() - start2
        out, ts = sim.data[pm.probe], sim.trange()
        spikes, spike_ts = {k: np.array(sim.data[p]) for k, p in spike_probes.items()}, sim.trange(sample_every=skip * dt)
    n = out.shape[0]
    t0 = time.time()
    real_ssp, table = pm.real_ssp[:n], args.decode_table or "host"
    if args.decode_table is not None or args.encode_backend is not None:
        if table == "device" and args.decode_backend != "hip":
            raise SystemExit("--decode-table device needs --decode-backend hip")
        real_ssp, encode_time, creation_time = H.timed_metric_inputs(space, path[:n], args.decode_backend, table, args.encode_backend)
        print("encode of %d true positions %.3f s (%s); decoder creation %s (table: %s)" % (
            n, encode_time, args.encode_backend or "numpy", "-" if creation_time is None else "%.3f s" % creation_time, table))
        t0 = time.time()
    est, sims, err = H.pathint_metrics(space, out, real_ssp, path[:n], backend=args.decode_backend, table=table)
    decode_time = time.time() - t0
    sim_grid = None
    if args.save_maps > 0:
        t0 = time.time()
        map_ts = ts[9::10]
        sim_grid = np.moveaxis(H.similarity_frames(space, out[9::10], args.save_maps, power=2, backend=args.decode_backend, table=table), 0, -1)
        print("similarity maps: %d samples over %s samples, %.1f MB: maps %.2f s (%s), decode %.2f s" % (
            sim_grid.shape[-1], " x ".join(["%d" % args.save_maps] * domain_dim), sim_grid.nbytes / 1e6, time.time() - t0,
            args.decode_backend, decode_time))
    print("d = %d, %d VCOs x %d neurons, T = %.1f s: build %.1f s, run %.2f s (%.1f sim-s/wall-s), decode %.2f s (%s); similarity "
          "to the true SSP mean %.4f, final position error %.4f" % (space.ssp_dim, (space.ssp_dim + 1) // 2, args.pi_n_neurons, T,
                                                                   build_time, elapsed_time, T / elapsed_time, decode_time,
                                                                   args.decode_backend, sims[min(200, n - 1):].mean(), err[-1]))
    if args.decode_refine:
        t0 = time.time()
        _, _, err_r = H.pathint_metrics(space, out, real_ssp, path[:n], backend=args.decode_backend, refine=True, table=table)
        print("position error, grid decode | grid-refine (%.2f s): median %.4f | %.4f, mean %.4f | %.4f, final %.4f | %.4f" % (
            time.time() - t0, np.median(err), np.median(err_r), err.mean(), err_r.mean(), err[-1], err_r[-1]))
    if args.save:
        os.makedirs(args.save_dir, exist_ok=True)
        name = "pi_backend_%s%s_sspdim_%d_pinneurons_%d_T_%d_limit_%s_seed_%d.npz" % (
            args.backend, args.save_name_extra, space.ssp_dim, args.pi_n_neurons, int(T), args.limit, args.seed)
        H.save_pathint_results(os.path.join(args.save_dir, name), space, ts, path, pm.real_ssp, out, elapsed_time, args=args,
                               elapsed_thread_time=elapsed_thread_time)
        print("saved", os.path.join(args.save_dir, name))
        if sim_grid is not None:
            maps_name = name[:-len(".npz")] + "_maps.npz"
            np.savez(os.path.join(args.save_dir, maps_name), ts=map_ts, sim_grid=sim_grid)
            print("saved", os.path.join(args.save_dir, maps_name))
        if spikes:
            spike_name = name[:-len(".npz")] + "_spikes.npz"
            np.savez(os.path.join(args.save_dir, spike_name), ts=spike_ts, **{"vco_n%d" % k: v for k, v in spikes.items()})
            print("saved", os.path.join(args.save_dir, spike_name))
    for k, v in spikes.items():
        print("oscillator %d: %d samples of %d neurons, %.1f %% of them spikes" % (k, v.shape[0], v.shape[1], 100.0 * (v != 0).mean()))
    return out


if __name__ == "__main__":
    main()
