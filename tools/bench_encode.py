"""SSP encoding on the GPU (encoding.SSPEncoder, GridDecoder(table="device")) against the NumPy path of SSPSpace.encode.

usage: python tools/bench_encode.py [a] [b] [big] [e2e] [--repeats R] [--host-rows M] [--out FILE]

  a     the 100 x 100 sample grid of a 2-D space at ssp_dim 1015 (the table examples/run_pathint.py decodes against)
  b     the 50^3 sample grid of a 3-D space at ssp_dim 1015 as built
  big   the 100^3 sample grid of the same 3-D space (the f32 table is about 4 GB; the host encode is timed on --host-rows points
        and scaled, the host-table decoder is not made)
  e2e   examples/run_pathint.py --ssp-dim 1015 --pi-n-neurons 10000 --T 20 --decode-backend hip, once with each --decode-table

Per shape, for the N sample points: device milliseconds of the encoder kernels alone, phase and product apart (HIP events of
ssn_encoder_get_info, output left on the device), for both dtypes; the f32 product as a fraction of the 157.3 TFLOP/s f32 matrix peak
(2 N d 2K FLOP); wall time of SSPEncoder.encode with the result left on the device and read back; SSPSpace.encode on the host; and
the wall time of GridDecoder(...) with table="host" (sample table encoded on the host, converted, uploaded) and table="device".
2 warm-up calls, then the median of --repeats calls; creations are timed once each, in a fresh state.  Everything is written to
--out (default profiles/encode_device.txt) as well as printed."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from sspslam_amd import SSPEncoder, harness as H
from sspslam_amd.decoding import GridDecoder

PEAK = 157.3e12
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


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
    return np.array(wall), extra


def fmt(x):
    x = np.asarray(x, dtype=float)
    return "median %.3f ms (min %.3f, max %.3f, %d calls)" % (np.median(x), x.min(), x.max(), len(x))


def shape(name, dim, n, args, host_table=True):
    import torch
    space = H.make_ssp_space(domain_dim=dim, ssp_dim=1015, rng=np.random.RandomState(0))
    pts = space.get_sample_points(n, "grid")
    N, d = pts.shape[0], space.ssp_dim
    K = space.refine_tables()[0]
    say("shape (%s): N = %d^%d = %d points, d = %d, K = %d bins" % (name, n, dim, N, d, K))
    m = N if host_table else min(N, args.host_rows)
    t0 = time.perf_counter()
    want = space.encode(pts[:m])
    t_host = 1e3 * (time.perf_counter() - t0)
    say("  SSPSpace.encode (host):       %.0f ms for %d points%s" % (t_host, m, "" if m == N else " -> %.0f ms for %d" % (t_host * N / m, N)))
    t_host *= N / m
    for dtype in ("f32", "f64"):
        with SSPEncoder(space, dtype=dtype) as enc:
            info = enc.info(N)
            wall_d, k = timed(lambda: enc.encode(pts, out="device"), args.repeats, lambda: enc.info())
            phase, prod = [i["last_phase_ms"] for i in k], [i["last_product_ms"] for i in k]
            flop = 2.0 * N * d * 2 * K
            say("  %s encoder, %d chunks of %d points:" % (dtype, info["n_chunks"], info["row_chunk"]))
            say("    k_encode_phase:             %s" % fmt(phase))
            say("    product:                    %s -> %.1f TFLOP/s%s" % (fmt(prod), flop / np.median(prod) / 1e9,
                                                                        ", %.3f of the f32 matrix peak" % (flop / (np.median(prod) * 1e-3) / PEAK) if dtype == "f32" else ""))
            say("    encode(out='device'):       %s  (wall, points uploaded as float64)" % fmt(wall_d))
            if N * d * 8 <= 4 << 30:
                wall_h, _ = timed(lambda: enc.encode(pts), max(3, args.repeats // 2))
                say("    encode(out='host'):         %s  (wall, %d MB read back as float64); host path / this = %.0f x" % (
                    fmt(wall_h), N * d * 8 >> 20, t_host / np.median(wall_h)))
            got = enc.encode(pts[:m][:4096])
            say("    largest |device - host| on %d points: %.2e" % (got.shape[0], np.abs(got - want[:4096]).max()))
            del got
        torch.cuda.empty_cache()
    del want
    for dtype in ("f32", "f64"):
        times = {}
        for table in (("host", "device") if host_table else ("device",)):
            space._grid_cache = {}                      # a first decode of a script: no table cached on the space
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec = GridDecoder(space, n, dtype=dtype, table=table)
            times[table] = 1e3 * (time.perf_counter() - t0)
            dec.close()
            torch.cuda.empty_cache()
        space._grid_cache = {}
        say("  GridDecoder(%s) creation:    %s" % (dtype, ", ".join("table='%s' %.0f ms" % kv for kv in times.items()))
            + (" -> %.0f x" % (times["host"] / times["device"]) if host_table else ""))
    say()


def end_to_end():
    say("end to end: examples/run_pathint.py --ssp-dim 1015 --pi-n-neurons 10000 --T 20 --decode-backend hip")
    for table in ("host", "device"):
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_pathint.py"), "--ssp-dim", "1015", "--pi-n-neurons", "10000", "--T", "20",
                            "--decode-backend", "hip", "--decode-table", table], capture_output=True, text=True, cwd=ROOT)
        say("  --decode-table %s (process wall %.1f s, exit %d):" % (table, time.perf_counter() - t0, r.returncode))
        for line in (r.stdout if r.returncode == 0 else r.stdout + r.stderr[-2000:]).strip().splitlines():
            say("    " + line)
    say()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["a", "b", "big", "e2e"])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-rows", type=int, default=125000, help="points of the host timing of shape big (scaled up)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_device.txt"))
    args = ap.parse_args()
    say("tools/bench_encode.py %s: one box, one run; kernels by HIP events, median of %d calls after 2 warm-ups" % (" ".join(args.shapes), args.repeats))
    for s in args.shapes:
        if s == "a":
            shape("a", 2, 100, args)
        elif s == "b":
            shape("b", 3, 50, args)
        elif s == "big":
            shape("big", 3, 100, args, host_table=False)
        elif s == "e2e":
            end_to_end()
        else:
            raise SystemExit("unknown shape %r" % s)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
