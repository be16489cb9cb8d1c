"""Similarity maps: GridDecoder.similarity (k_decode_map) against the decode of the same rows, the composition it replaces and NumPy.

usage: python tools/bench_map.py [a] [b] [c] [--repeats R] [--numpy-rows M]

  a    2 000 x 1015 rows over the 100 x 100 grid to host float64 and float32 (the gif frames of a 20 s run)
  b   20 000 x 1015 rows over 100 x 100 with out="device" (800 MB of float32)
  c    2 000 rows over a 3-D 50^3 grid at ssp_dim 1015 as built, out="device" (1 GB)

Per shape, all in the same run with the same decoder: device milliseconds of the map kernels alone (HIP events around prepare +
k_decode_map of every chunk, copies outside) and the wall time of the call, the fraction of the 157.3 TFLOP/s f32 matrix peak
(2 T S d FLOP), bytes stored per second of kernel time; the decode kernels on the same rows (prepare + k_decode_tiles +
k_decode_finish: the product without the stores); the composition the map kernel replaces, through torch on the same device (rows
converted to float32, a matmul into a T x S buffer, the square in place; torch events); and the NumPy float64 path of
SSPSpace.similarity_map on --numpy-rows rows, scaled to all of them.  Maps are power=2 over raw rows, as the figure scripts make
them.  2 warm-up calls, then the median and extremes of --repeats calls."""
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


def torch_composed(rows_dev, table32, repeats):
    """Rows to float32, matmul into a (T, S) buffer, square in place: device ms by torch events."""
    import torch
    out = torch.empty((rows_dev.shape[0], table32.shape[0]), dtype=torch.float32, device=rows_dev.device)
    ms = []
    for i in range(2 + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r32 = rows_dev.to(torch.float32)
        torch.matmul(r32, table32.T, out=out)
        out.mul_(out)
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    return np.array(ms), out


def shape(name, dim, n, T, outs, args, numpy_cap=None):
    import torch
    t0 = time.perf_counter()
    space, rows = inputs(dim, 1015, T)
    table, _ = space.get_sample_pts_and_ssps(n, "grid")
    S, d = table.shape
    print("shape (%s): %d rows x d = %d over %d^%d = %d samples (inputs and table encoded in %.1f s)" % (name, T, d, n, dim, S, time.perf_counter() - t0), flush=True)
    flop = 2.0 * T * S * d
    rows_dev = torch.from_numpy(rows).to("cuda:0")
    with GridDecoder(space, n) as dec:
        kern = lambda: dec.info()["last_kernel_ms"]
        _, dk = timed(lambda: dec.indices(rows_dev), args.repeats, kern)
        print("  decode kernels, same rows (prepare + k_decode_tiles + k_decode_finish):  %s, %.3f of peak" % (fmt(dk), flop / (np.median(dk) * 1e-3) / PEAK), flush=True)
        last = None
        for out, out_dtype in outs:
            esz = 8 if (out == "host" and out_dtype is None) else 4
            call = lambda: dec.similarity(rows_dev if out == "device" else rows, power=2, out=out, out_dtype=out_dtype)
            wall, mk = timed(call, args.repeats, kern)
            last = call()
            label = "out=%s%s" % (out, "" if out == "device" else " float%d" % (8 * esz))
            print("  map %-19s kernels (prepare + k_decode_map): %s, %.3f of peak, %.1f GB/s stored, %d launches" % (
                label + ":", fmt(mk), flop / (np.median(mk) * 1e-3) / PEAK, T * S * esz / (np.median(mk) * 1e-3) / 1e9, dec.info()["last_launches"]))
            print("  %-23s wall: %s; map kernels - decode kernels = %+.3f ms" % ("", fmt(wall), np.median(mk) - np.median(dk)), flush=True)
        dev_map = last if hasattr(last, "is_cuda") else dec.similarity(rows_dev, power=2, out="device")
        table32 = torch.from_numpy(table).to("cuda:0").to(torch.float32)
        comp, ref = torch_composed(rows_dev, table32, args.repeats)
        diff = float((dev_map - ref).abs().max())
        print("  composition through torch (to float32, matmul into a %d MB buffer, square): %s; composed / map kernels = %.2f; largest |difference| %.1e" % (
            T * S * 4 / 1e6, fmt(comp), np.median(comp) / np.median(mk), diff), flush=True)
        m = min(T, args.numpy_rows, numpy_cap or T)
        host_map = dev_map[:m].cpu().numpy().astype(np.float64)
        del dev_map, ref, table32
    t0 = time.perf_counter()
    want = space.similarity_map(rows[:m], n, power=2)
    t_np = 1e3 * (time.perf_counter() - t0)
    print("  NumPy SSPSpace.similarity_map: %.0f ms for %d rows%s; largest |device - NumPy| %.1e (largest value %.2f)" % (
        t_np, m, "" if m == T else " -> %.0f ms for %d rows" % (t_np * T / m, T), np.abs(host_map - want).max(), want.max()), flush=True)
    return t_np * T / m


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["a", "b", "c"])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--numpy-rows", type=int, default=2000, help="rows of the NumPy timing (scaled up when fewer than the shape's)")
    args = ap.parse_args()
    for s in args.shapes:
        if s == "a":
            shape("a", 2, 100, 2000, [("host", None), ("host", "f32"), ("device", None)], args)
        elif s == "b":
            shape("b", 2, 100, 20000, [("device", None)], args)
        elif s == "c":
            shape("c", 3, 50, 2000, [("device", None)], args, numpy_cap=250)      # 125 000 samples: NumPy on 250 rows, scaled
        else:
            raise SystemExit("unknown shape %r" % s)
