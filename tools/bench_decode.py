"""Grid decode of a probed trajectory: the GPU decoder (decoding.GridDecoder) against the NumPy path of SSPSpace.decode.

usage: python tools/bench_decode.py [a] [b] [c] [--rows N] [--repeats R] [--numpy-rows M] [--refine]

  a   20 000 x 1015 rows over the 100 x 100 grid (what examples/run_pathint.py decodes after a 20 s config-2 run)
  b   20 000 rows over a 3-D 50^3 grid at ssp_dim 1015 as built (the f32 table is about 0.5 GB)
  c   2 048 x 1015 over 100 x 100, small enough to write the similarity matrix out: the fused kernel against the composition it
      replaces (k_gemm_nt_mfma_f32 into a buffer, then k_argmax_partial), both with the same prepare kernel in front

Per shape: device milliseconds of the kernels alone (HIP events around prepare + product + finish of every chunk, copies outside),
wall time of GridDecoder.decode including the upload of the rows, wall time of the NumPy decode on the same box (on --numpy-rows
rows, scaled to all of them, when that is fewer), the fraction of the 157.3 TFLOP/s f32 matrix peak the kernels reach
(2 T S d FLOP), and whether the two answers agree.  2 warm-up calls, then the median and minimum of --repeats calls.

--refine (shapes a and b): GridDecoder.refine (8 Newton steps per row from the grid point, 'grid-refine') on the same rows with the
same decoder in the same run: kernels and wall time next to the plain decode's, the median position error of both against the
encoded path, and the NumPy float64 backend of the same rule on --numpy-rows rows."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from sspslam_amd import harness as H
from sspslam_amd.decoding import GridDecoder

PEAK = 157.3e12


def inputs(dim, ssp_dim, T):
    space = H.make_ssp_space(domain_dim=dim, ssp_dim=ssp_dim, rng=np.random.RandomState(0))
    rng = np.random.RandomState(1)
    path = rng.uniform(-0.9, 0.9, (T, dim))
    rows = space.encode(path) + rng.randn(T, space.ssp_dim) * 0.5 / np.sqrt(space.ssp_dim)
    return space, rows


def timed(fn, repeats, after=None):
    for _ in range(2):
        fn()
    wall, extra = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        wall.append(1e3 * (time.perf_counter() - t0))
        if after:
            extra.append(after())
    return np.array(wall), np.array(extra)


def fmt(x):
    return "median %.3f ms (min %.3f, max %.3f, %d calls)" % (np.median(x), x.min(), x.max(), len(x))


def shape_ab(name, dim, n, args):
    t0 = time.perf_counter()
    space, rows = inputs(dim, 1015, args.rows)
    table, points = space.get_sample_pts_and_ssps(n, "grid")
    S, d, T = table.shape[0], table.shape[1], rows.shape[0]
    print("shape (%s): %d rows x d = %d over %d^%d = %d samples (inputs and table encoded in %.1f s)" % (name, T, d, n, dim, S, time.perf_counter() - t0), flush=True)
    t0 = time.perf_counter()
    with GridDecoder(space, n) as dec:
        print("  decoder created (table converted and uploaded) in %.2f s; plan %s" % (
            time.perf_counter() - t0, {k: v for k, v in dec.info(T).items() if k in ("row_chunk", "n_chunks", "n_strips", "tiles_per_strip")}), flush=True)
        wall, kern = timed(lambda: dec.decode(rows), args.repeats, lambda: dec.info()["last_kernel_ms"])
        est = dec.decode(rows)
        if args.refine:
            wall_r, kern_r = timed(lambda: dec.refine(rows), args.repeats, lambda: dec.info()["last_kernel_ms"])
            x, _, status, _ = dec.refine(rows, return_info=True)
    flop = 2.0 * T * S * d
    print("  kernels alone:          %s -> %.1f TFLOP/s, %.3f of the f32 matrix peak" % (fmt(kern), flop / np.median(kern) / 1e9, flop / (np.median(kern) * 1e-3) / PEAK))
    print("  GridDecoder.decode:     %s  (wall, rows uploaded as float64)" % fmt(wall), flush=True)
    m = min(T, args.numpy_rows)
    if args.refine:
        path = np.random.RandomState(1).uniform(-0.9, 0.9, (T, dim))          # what inputs() encoded
        K = space.refine_tables()[0]
        print("  refine, kernels alone:  %s  (prepare + tiles + finish + spectrum + k_decode_refine, K = %d bins)" % (fmt(kern_r), K))
        print("  GridDecoder.refine:     %s  (wall); added to the grid decode: kernels %.3f ms (%.2f x the decode's), wall %.3f ms" % (
            fmt(wall_r), np.median(kern_r) - np.median(kern), (np.median(kern_r) - np.median(kern)) / np.median(kern),
            np.median(wall_r) - np.median(wall)))
        print("  median position error:  grid %.5f, refined %.5f; status words: %s" % (
            np.median(np.linalg.norm(est - path, axis=1)), np.median(np.linalg.norm(x - path, axis=1)),
            dict(zip(*[v.tolist() for v in np.unique(status, return_counts=True)]))), flush=True)
        t0 = time.perf_counter()
        xh = space.decode(rows[:m], "grid-refine", "grid", n)
        t_np = 1e3 * (time.perf_counter() - t0)
        print("  NumPy 'grid-refine':    %.0f ms for %d rows (grid decode included); largest |x_device - x_numpy| %.2e" % (
            t_np, m, np.abs(x[:m] - xh).max()), flush=True)
    t0 = time.perf_counter()
    host = space.decode(rows[:m], "from-set", "grid", n)
    t_np = 1e3 * (time.perf_counter() - t0)
    print("  NumPy SSPSpace.decode:  %.0f ms for %d rows%s (one call, table cached)" % (t_np, m, "" if m == T else " -> %.0f ms for %d rows" % (t_np * T / m, T)))
    differ = np.flatnonzero(np.any(est[:m] != host, axis=1))
    print("  host path / GridDecoder.decode = %.0f x; answers equal on %d of %d rows" % (t_np * T / m / np.median(wall), m - differ.size, m), flush=True)
    if differ.size:       # near-ties: the float64 similarities of the two answers against the decoder's bar (tests/decoding_checks.py)
        nrm = np.linalg.norm(rows[differ], axis=1, keepdims=True)
        u = rows[differ] / nrm
        s_host = np.sum(u * space.encode(host[differ]), axis=1)
        s_dev = np.sum(u * space.encode(est[differ]), axis=1)
        bar = 2 * (1.5e-7 + 2 * 2.0 ** -24) * (np.abs(u) @ np.abs(table).T).max(axis=1)
        print("  the %d rows that differ are near-ties: float64 similarity of the host's sample minus the decoder's at most %.2e, bar %.2e"
              % (differ.size, np.max(s_host - s_dev), bar.min()), flush=True)


def shape_c(args):
    space, rows = inputs(2, 1015, 2048)
    table, _ = space.get_sample_pts_and_ssps(100, "grid")
    S, d, T = table.shape[0], table.shape[1], rows.shape[0]
    print("shape (c): %d rows x d = %d over %d samples: fused kernel vs k_gemm_nt_mfma_f32 + k_argmax_partial" % (T, d, S), flush=True)
    with GridDecoder(space, 100) as dec:
        _, fused = timed(lambda: dec.indices(rows), args.repeats, lambda: dec.info()["last_kernel_ms"])
        a = dec.indices(rows)
        _, comp = timed(lambda: dec.indices_composed(rows), args.repeats, lambda: dec.info()["last_kernel_ms"])
        b = dec.indices_composed(rows)
    flop = 2.0 * T * S * d
    print("  fused (prepare + k_decode_tiles + k_decode_finish):          %s, %.3f of peak" % (fmt(fused), flop / (np.median(fused) * 1e-3) / PEAK))
    print("  composed (prepare + k_gemm_nt_mfma_f32 + k_argmax_partial):  %s, %.3f of peak; writes and re-reads %.0f MB" % (
        fmt(comp), flop / (np.median(comp) * 1e-3) / PEAK, T * S * 4 / 1e6))
    print("  composed / fused = %.2f; indices equal on %d of %d rows" % (np.median(comp) / np.median(fused), int((a == b).sum()), T), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["a", "b", "c"])
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--numpy-rows", type=int, default=20000, help="rows of the NumPy timing (scaled up when fewer than --rows)")
    ap.add_argument("--refine", action="store_true", help="also time GridDecoder.refine on shapes a and b")
    args = ap.parse_args()
    for s in args.shapes:
        if s == "a":
            shape_ab("a", 2, 100, args)
        elif s == "b":
            shape_ab("b", 3, 50, args)
        elif s == "c":
            shape_c(args)
        else:
            raise SystemExit("unknown shape %r" % s)
