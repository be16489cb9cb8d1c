#!/usr/bin/env python3
"""SSP-SLAM on the MI355X backend with the command line of the reference's ``experiments/run_slam.py`` (the options
that concern the model; ``--backend mi355x`` / ``mi355x-f64``).

    python examples/run_slam.py --ssp-dim 1015 --pi-n-neurons 10000 --mem-n-neurons 10150 --n-landmarks 10 --T 20 --save

Prints the trajectory accuracy and the recalled landmark map (``run_slam.py:263-268``: activities of the memory
population for each landmark's semantic pointer times the final PES decoders, decoded to positions) and, with
``--save``, writes the result file with the reference's field names.  With ``--decode-backend hip`` the final map is recalled on
the GPU from the learned state (``sim.recall``: the Voja-learned encoders, as ``slam_map_new.py:342-347`` does) and neither matrix
is read back.  ``--map-every SECONDS`` also watches the map being learned: a ``MapProbe`` on the landmark SPs, decoded to positions
(``landmark_loc_over_time`` in the result file, the frames of ``run_slam_map_gif.py``).  ``--save-maps N`` adds that script's
similarity maps over the N x N sample grid at every map sample (``harness.similarity_frames``; ``k_decode_map`` on the GPU with
``--decode-backend hip``): ``sim_grid`` of the probed trajectory (squared, raw rows) and ``landmark_sim_grid`` of the recalled
frames (normalised, squared; a landmark not seen yet gives a zero map where the reference's ``q / norm`` gives NaN), written with
``--save`` to ``<result file minus .npz>_maps.npz``; the map seconds are printed next to the decode seconds.  ``--inverse-memory``
learns the inverse map beside the SLAM network (landmark SSP -> landmark SP, ``slam_map_new.py:243-250``) and ``--area-query X0 X1 Y0
Y1`` (repeatable) asks it which landmarks lie in a box: ``harness.area_query``, the script's ``get_sims_for_area`` with the mesh sum
in closed form (``SSPSpace.encode_region``) and the recall on the GPU.  ``--vector-queries`` (with ``--map-every``) asks where every
landmark lies relative to the agent at every map sample (``slam_map_new.py:453-485``, ``harness.vector_query``): the pose estimate
cleaned up on the grid, inverted and unbound from the recalled landmark SSPs - on the GPU with ``--decode-backend hip``
(``SSPBinder``) -, its cosine and distance errors printed for the last sample and saved as ``landmark_vec_*``.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sspslam_amd.frontend as nengo          # noqa: E402
from sspslam_amd import MapProbe, harness as H # noqa: E402
from sspslam_amd.simulator import Simulator    # noqa: E402


def parse(argv=None):
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--backend", default="mi355x", type=str, help="mi355x (float32) or mi355x-f64 (parity mode)")
    p.add_argument("--domain-dim", default=2, type=int)
    p.add_argument("--path-data", default=None, type=str)
    p.add_argument("--data-dt", default=0.001, type=float)
    p.add_argument("--limit", default=0.1, type=float)
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--T", default=200, type=float)
    p.add_argument("--n-landmarks", default=50, type=int)
    p.add_argument("--view-rad", default=0.2, type=float)
    p.add_argument("--update-thres", default=0.2, type=float)
    p.add_argument("--shift-rate", default=0.2, type=float)
    p.add_argument("--pi-n-neurons", default=800, type=int)
    p.add_argument("--mem-n-neurons", default=970, type=int)
    p.add_argument("--circonv-n-neurons", default=100, type=int)
    p.add_argument("--ssp-dim", default=97, type=int)
    p.add_argument("--n-scales", default=0, type=int)
    p.add_argument("--n-rotates", default=3, type=int)
    p.add_argument("--length-scale", default=0.2, type=float)
    p.add_argument("--save", action="store_true")
    p.add_argument("--save-dir", default="data")
    p.add_argument("--save-name-extra", default="")
    p.add_argument("--n-eval-points", default=0, type=int, help="decoder-solve evaluation points; 0 = nengo's default")
    p.add_argument("--decode-backend", default="numpy", choices=["numpy", "hip"],
                   help="grid decodes of the trajectory and the recalled map: NumPy on the host, or the GPU grid decoder")
    p.add_argument("--decode-table", default=None, choices=["host", "device"],
                   help="with --decode-backend hip: the decoder's sample table encoded on the host and uploaded, or encoded on the "
                        "GPU from the sample points; prints the decoder-creation seconds")
    p.add_argument("--encode-backend", default=None, choices=["numpy", "hip"],
                   help="encode the true path (real_ssp of the metrics) with NumPy or on the GPU (encoding.SSPEncoder); prints the "
                        "encode seconds")
    p.add_argument("--decode-refine", action="store_true",
                   help="also decode with 'grid-refine' (Newton steps from the grid point) and print both sets of errors")
    p.add_argument("--map-every", default=0.0, type=float, metavar="SECONDS",
                   help="recall the landmark map on the GPU every SECONDS of simulated time (a MapProbe) and decode it to positions")
    p.add_argument("--save-maps", default=0, type=int, metavar="N",
                   help="with --map-every: similarity maps over the N x ... x N sample grid at every map sample - sim_grid of the "
                        "probed trajectory (squared, raw rows) and landmark_sim_grid of the MapProbe frames (normalised, squared), "
                        "made by --decode-backend; with --save written to <result>_maps.npz")
    p.add_argument("--vector-queries", action="store_true",
                   help="with --map-every: where every landmark lies relative to the agent at every map sample (slam_map_new.py:453-485) - "
                        "the cleaned-up pose estimate unbound from the recalled landmark SSPs, decoded (harness.vector_query, made by "
                        "--decode-backend); with --save written as landmark_vec_est, landmark_vec_cos_err, landmark_vec_dist_err")
    p.add_argument("--inverse-memory", action="store_true",
                   help="learn the inverse memory (landmark SSP -> landmark SP) beside the SLAM network, as slam_map_new.py does")
    p.add_argument("--area-query", action="append", nargs="+", type=float, default=None, metavar="LO HI",
                   help="with --inverse-memory: X0 X1 Y0 Y1 (lo hi per axis) of a box; prints every landmark's similarity to the recall "
                        "of the box's region SSP beside whether the landmark lies in it.  Repeatable")
    return p.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    dt = 0.001
    if args.save_maps > 0 and not args.map_every > 0:
        raise SystemExit("--save-maps needs --map-every: the maps are made at the map samples")
    if args.vector_queries and not args.map_every > 0:
        raise SystemExit("--vector-queries needs --map-every: the queries are made at the map samples")
    if args.area_query and not args.inverse_memory:
        raise SystemExit("--area-query needs --inverse-memory: the boxes are recalled through the inverse memory")
    if args.area_query and any(len(b) != 2 * args.domain_dim for b in args.area_query):
        raise SystemExit("--area-query takes lo hi per axis: %d numbers" % (2 * args.domain_dim))
    if args.path_data is None:
        T = args.T
        path, vels = H.make_random_path(T, dt=dt, limit=args.limit, seed=args.seed, domain_dim=args.domain_dim)
    else:
        path, vels = H.load_path(args.path_data, data_dt=args.data_dt, dt=dt)
        T = path.shape[0] * dt
    space = H.make_ssp_space(path.shape[1], ssp_dim=args.ssp_dim, n_scales=args.n_scales, n_rotates=args.n_rotates,
                             length_scale=args.length_scale)
    sm = H.make_slam_model(space, path, vels, n_landmarks=args.n_landmarks, pi_n_neurons=args.pi_n_neurons,
                           mem_n_neurons=args.mem_n_neurons, circonv_n_neurons=args.circonv_n_neurons, view_rad=args.view_rad,
                           update_thres=args.update_thres, shift_rate=args.shift_rate, seed=args.seed, dt=dt,
                           weights_sample_every=None if args.decode_backend == "hip" else T)
    inv_memory = None
    if args.inverse_memory:      # slam_map_new.py:243-250: keyed by the landmark's SSP, valued by its SP, gated by the in-view node
        from sspslam_amd.networks import AssociativeMemory
        d = space.ssp_dim
        with sm.model:
            inv_memory = AssociativeMemory(args.mem_n_neurons, d, d, 0.1, voja_learning_rate=5e-4, pes_learning_rate=1e-2, voja=True,
                                           encoders=space.sample_grid_encoders(args.mem_n_neurons), radius=1.3, seed=args.seed)
            nengo.Connection(sm.slam.landmark_ssp_ens.output, inv_memory.key_input, synapse=0.05)
            nengo.Connection(sm.slam.landmark_id_input, inv_memory.value_input, synapse=None)
            nengo.Connection(sm.slam.no_landmark_in_view, inv_memory.learning, synapse=None)
    map_probe = None
    if args.map_every > 0:
        with sm.model:
            map_probe = MapProbe(sm.slam.assomemory, sm.lm_space.vectors, sample_every=args.map_every, label="landmark map")
    dtype = "f64" if args.backend.endswith("f64") else "f32"
    t0 = time.time()
    sim = Simulator(sm.model, dt=dt, dtype=dtype, n_eval_points=args.n_eval_points or None)
    build_time = time.time() - t0
    start = time.time()
    with sim:
        sim.run(T)
        elapsed = time.time() - start
        out, ts = sim.data[sm.probe], sim.trange()
        built_memory = sim.data[sm.slam.assomemory.memory]
        if args.decode_backend == "hip":      # the learned map from the device: L x d numbers instead of both matrices
            lm_ssps = sim.recall(sm.slam.assomemory, sm.lm_space.vectors)
        else:
            decoders = sim.data[sm.weights_probe][-1]
        frames = sim.data[map_probe] if map_probe is not None else None
        map_ts = sim.trange(sample_every=args.map_every) if map_probe is not None else None
        recall_time, recall_kernel_ms = sim.recall_seconds, sim.recall_kernel_ms
        if args.area_query:
            boxes = np.asarray(args.area_query, dtype=float).reshape(len(args.area_query), space.domain_dim, 2)
            backend = "hip" if dtype == "f32" else "hip-f64"
            t0 = time.time()
            space.encode_region(boxes, samples=20, normalize=True, backend=backend)
            area_encode = time.time() - t0
            area_sims = H.area_query(sim, inv_memory, space, boxes, sm.lm_space.vectors, samples=20, backend=backend)
            area_time = time.time() - t0 - area_encode
    n = out.shape[0]
    t0 = time.time()
    real_ssp, table = sm.real_ssp[:n], args.decode_table or "host"
    if args.decode_table is not None or args.encode_backend is not None:
        if table == "device" and args.decode_backend != "hip":
            raise SystemExit("--decode-table device needs --decode-backend hip")
        real_ssp, encode_time, creation_time = H.timed_metric_inputs(space, path[:n], args.decode_backend, table, args.encode_backend)
        print("encode of %d true positions %.3f s (%s); decoder creation %s (table: %s)" % (
            n, encode_time, args.encode_backend or "numpy", "-" if creation_time is None else "%.3f s" % creation_time, table))
        t0 = time.time()
    est, sims, err = H.pathint_metrics(space, out, real_ssp, path[:n], backend=args.decode_backend, table=table)
    if args.decode_backend == "hip":
        lm_locs = space.decode(lm_ssps, "from-set", "grid", 100, backend="hip", table=table)
    else:
        lm_ssps, lm_locs = H.map_recall(space, sm.lm_space, built_memory, nengo.LIF(), decoders, backend=args.decode_backend)
    decode_time = time.time() - t0
    lm_over_time = sim_grid = landmark_sim_grid = vector_fields = None
    if frames is not None:
        t0 = time.time()
        lm_over_time = H.map_over_time(space, frames, backend=None if args.decode_backend == "numpy" else args.decode_backend, table=table)
        print("map recall: %d samples of %d landmarks every %.3f s: recall %.3f s (kernels %.1f ms), decode %.2f s (%s); median landmark "
              "error first -> last sample %.3f -> %.3f" % (frames.shape[0], frames.shape[1], args.map_every, recall_time, recall_kernel_ms,
                                                        time.time() - t0, args.decode_backend,
                                                        float(np.median(np.linalg.norm(lm_over_time[0] - sm.obj_locs, axis=1))) if len(frames) else np.nan,
                                                        float(np.median(np.linalg.norm(lm_over_time[-1] - sm.obj_locs, axis=1))) if len(frames) else np.nan))
        if args.save_maps > 0:
            # sim_grid of run_slam_map_gif.py:316-317 at the map samples, and q_sims of :366-368 for every landmark of every frame.  A
            # landmark not seen yet recalls a near-zero row: it stays as it is and its map is zero (the reference's q / norm is NaN)
            t1 = time.time()
            backend = None if args.decode_backend == "numpy" else args.decode_backend
            rows = out[np.searchsorted(ts, map_ts - 0.5 * dt)]
            sim_grid = np.moveaxis(H.similarity_frames(space, rows, args.save_maps, power=2, backend=backend, table=table), 0, -1)
            landmark_sim_grid = H.similarity_frames(space, frames, args.save_maps, power=2, normalize=True, backend=backend, table=table)
            print("similarity maps: %d path and %d x %d landmark maps over %s samples, %.1f MB: maps %.2f s (%s), decode %.2f s" % (
                rows.shape[0], frames.shape[0], frames.shape[1], " x ".join(["%d" % args.save_maps] * space.domain_dim),
                (sim_grid.nbytes + landmark_sim_grid.nbytes) / 1e6, time.time() - t1, args.decode_backend, t1 - t0))
        if args.vector_queries:
            t1 = time.time()
            at = np.searchsorted(ts, map_ts - 0.5 * dt)
            vq_backend = None if args.decode_backend == "numpy" else ("hip" if dtype == "f32" else "hip-f64")
            vq = H.vector_query(space, out[at], frames, backend=vq_backend, table=table)
            true_vecs = sm.obj_locs[None, :, :] - path[at][:, None, :]
            vec_cos_err, vec_dist_err = H.vector_query_errors(space, vq, true_vecs)
            vector_fields = dict(landmark_vec_est=vq["vec_est"], landmark_vec_cos_err=vec_cos_err, landmark_vec_dist_err=vec_dist_err)
            print("vector queries: %d samples x %d landmarks in %.3f s (%s); last sample: cosine error median %.3f (max %.3f), distance error "
                  "median %.3f (max %.3f)" % (frames.shape[0], frames.shape[1], time.time() - t1, vq_backend or "numpy",
                                               float(np.median(vec_cos_err[-1])), float(np.max(vec_cos_err[-1])),
                                               float(np.median(vec_dist_err[-1])), float(np.max(vec_dist_err[-1]))))
    elif recall_time:
        print("map recall: final map on the GPU in %.4f s (kernels %.2f ms)" % (recall_time, recall_kernel_ms))
    lm_err = np.linalg.norm(lm_locs - sm.obj_locs, axis=1)
    print("d = %d, T = %.1f s: build %.1f s, run %.2f s (%.2f sim-s/wall-s), decode %.2f s (%s); similarity to the true SSP mean "
          "%.4f, final position error %.4f; recalled landmark positions: median error %.3f" % (
              space.ssp_dim, T, build_time, elapsed, T / elapsed, decode_time, args.decode_backend, sims[min(200, n - 1):].mean(),
              err[-1], float(np.median(lm_err))))
    if args.area_query:
        print("area queries: %d boxes, region encode %.4f s (%s, the first call makes the encoder); harness.area_query - encode, recall "
              "through the inverse memory on the GPU, compare - %.4f s" % (
            len(boxes), area_encode, backend, area_time))
        for box, row in zip(boxes, area_sims):
            inside = np.all((sm.obj_locs >= box[:, 0]) & (sm.obj_locs <= box[:, 1]), axis=1)
            print("  box %s: %s" % (" x ".join("[%g, %g]" % tuple(ax) for ax in box),
                                    "  ".join("%d%s %+.3f" % (j, "*" if inside[j] else "", row[j]) for j in range(len(row)))))
        print("  (* the landmark lies in the box)")
    if args.decode_refine:
        t0 = time.time()
        _, _, err_r = H.pathint_metrics(space, out, real_ssp, path[:n], backend=args.decode_backend, refine=True, table=table)
        if args.decode_backend == "hip":
            lm_locs_r = space.decode(lm_ssps, "grid-refine", "grid", 100, backend="hip", table=table)
        else:
            _, lm_locs_r = H.map_recall(space, sm.lm_space, built_memory, nengo.LIF(), decoders, backend=args.decode_backend, refine=True)
        lm_err_r = np.linalg.norm(lm_locs_r - sm.obj_locs, axis=1)
        print("grid decode | grid-refine (%.2f s): position error median %.4f | %.4f, final %.4f | %.4f; recalled landmark "
              "positions: median error %.4f | %.4f" % (time.time() - t0, np.median(err), np.median(err_r), err[-1], err_r[-1],
                                                      float(np.median(lm_err)), float(np.median(lm_err_r))))
    if args.save:
        os.makedirs(args.save_dir, exist_ok=True)
        name = "slam_backend_%s%s_sspdim_%d_pinneurons_%d_memnneurons_%d_ccnneurons_%d_T_%d_limit_%s_seed_%d.npz" % (
            args.backend, args.save_name_extra, space.ssp_dim, args.pi_n_neurons, args.mem_n_neurons, args.circonv_n_neurons,
            int(T), args.limit, args.seed)
        H.save_slam_results(os.path.join(args.save_dir, name), space, ts, path, sm.real_ssp, sm.obj_locs, args.view_rad, out,
                            lm_ssps, lm_locs, elapsed, args=args, landmark_loc_over_time=lm_over_time, landmark_loc_over_time_ts=map_ts,
                            extra_fields=vector_fields)
        print("saved", os.path.join(args.save_dir, name))
        if sim_grid is not None:
            maps_name = name[:-len(".npz")] + "_maps.npz"
            np.savez(os.path.join(args.save_dir, maps_name), ts=map_ts, sim_grid=sim_grid, landmark_sim_grid=landmark_sim_grid)
            print("saved", os.path.join(args.save_dir, maps_name))
    return out, lm_locs


if __name__ == "__main__":
    main()
