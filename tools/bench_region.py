"""Region SSPs on the GPU (SSPEncoder.encode_region, k_encode_phase_box) against the point encode, the NumPy closed form and the
reference's way (encode a 20 x 20 mesh and sum).

usage: python tools/bench_region.py [--dims 1015 241] [--counts 1 1000 100000] [--repeats R] [--out FILE]

Per ssp_dim (2-D Hexagonal space) and box count N, in the same run on the same box: device milliseconds of the encoder kernels, phase
and product apart (HIP events of ssn_encoder_get_info, output left on the device), and the wall time of the call, for encode_region
in its three modes (integral, mean, mesh of 20 x 20) and for the point encode of N points; k_encode_phase_box / k_encode_phase is the
cost of the amplitude.  Then the NumPy closed form (SSPSpace.encode_region) and the reference's mesh-and-sum (SSPSpace.encode of
400 N points, summed; timed on at most --mesh-rows boxes and scaled).  Last, the worst |error| / bar of the instrument of
tests/region_checks.py over its cases, as the GPU tests measure it.  2 warm-up calls, then the median of --repeats calls.  Everything is
written to --out (default profiles/encode_region.txt) as well as printed."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from sspslam_amd import SSPEncoder, harness as H

LINES = []
MODES = (("integral", {}), ("mean", {"mean": True}), ("mesh 20 x 20", {"samples": 20}))


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


def med(x):
    x = np.asarray(x, dtype=float)
    return "%.4f ms (min %.4f, max %.4f)" % (np.median(x), x.min(), x.max())


def boxes_for(space, n, rng):
    b = space.domain_bounds
    span = b[:, 1] - b[:, 0]
    L = span * 10.0 ** rng.uniform(-3.0, 0.0, (n, b.shape[0]))
    lo = b[:, 0] + rng.uniform(0.0, 1.0, L.shape) * (span - L)
    return np.stack([lo, lo + L], axis=2)


def one_dim(d, args):
    # d = 241 is the Hexagonal space of 8 scales x 5 rotations at length scale 0.3; any other d is make_ssp_space's
    space = H.make_ssp_space(2, n_scales=8, n_rotates=5, length_scale=0.3) if d == 241 else H.make_ssp_space(2, ssp_dim=d)
    d = space.ssp_dim
    K = space.refine_tables()[0]
    rng = np.random.RandomState(3)
    say("ssp_dim %d (2-D, K = %d bins)" % (d, K))
    for n in args.counts:
        boxes = boxes_for(space, n, rng)
        pts = boxes[:, :, 0].copy()
        say("  N = %d" % n)
        for dtype in ("f32", "f64"):
            with SSPEncoder(space, dtype=dtype) as enc:
                wall, k = timed(lambda: enc.encode(pts, out="device"), args.repeats, lambda: enc.info())
                p_phase = np.median([i["last_phase_ms"] for i in k])
                say("    %s points           k_encode_phase     %s   product %s   call %s" % (
                    dtype, med([i["last_phase_ms"] for i in k]), med([i["last_product_ms"] for i in k]), med(wall)))
                for label, kw in MODES:
                    wall, k = timed(lambda: enc.encode_region(boxes, out="device", **kw), args.repeats, lambda: enc.info())
                    phase = [i["last_phase_ms"] for i in k]
                    say("    %s %-16s k_encode_phase_box %s   product %s   call %s   phase / point phase = %.2f" % (
                        dtype, label, med(phase), med([i["last_product_ms"] for i in k]), med(wall), np.median(phase) / p_phase))
                wall, k = timed(lambda: enc.encode_region(boxes, samples=20, normalize=True, out="device"), args.repeats, lambda: enc.info())
                say("    %s mesh, normalised   product + k_encode_rownorm %s   call %s" % (dtype, med([i["last_product_ms"] for i in k]), med(wall)))
        m = min(n, args.numpy_rows)
        wall, _ = timed(lambda: space.encode_region(boxes[:m], samples=20), max(3, args.repeats // 2))
        say("    NumPy closed form (mesh)          %.3f ms for %d boxes%s" % (np.median(wall), m, "" if m == n else " -> %.1f ms for %d" % (np.median(wall) * n / m, n)))
        m = min(n, args.mesh_rows)
        t0 = time.perf_counter()
        for box in boxes[:m]:
            axes = [np.linspace(box[a, 0], box[a, 1], 20) for a in range(2)]
            space.encode(np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 2)).sum(axis=0)
        t = 1e3 * (time.perf_counter() - t0)
        say("    encode a 20 x 20 mesh and sum     %.1f ms for %d boxes%s" % (t, m, "" if m == n else " -> %.0f ms for %d" % (t * n / m, n)))
    say()


def ratios():
    import encode_checks as ec
    import region_checks as rg
    say("worst |error| / bar of tests/region_checks.py (130 boxes per case, every entry):")
    for dtype in ("f32", "f64"):
        worst = {}
        for name in ec.CASES:
            with SSPEncoder(ec.case_space(name), dtype=dtype) as enc:
                for mode, samples in rg.variants(ec.case_space(name)):
                    ref = rg.reference(name, mode, samples)
                    r = float(ref.ratio(enc.encode_region(ref.boxes, samples=samples, mean=mode == "mean"), dtype).max())
                    if r > worst.get(mode, (0.0, ""))[0]:
                        worst[mode] = (r, "%s%s" % (name, "" if samples is None else " n = %d" % samples))
        say("  %s: %s" % (dtype, ", ".join("%s %.3f (%s)" % (k, v[0], v[1]) for k, v in worst.items())))
    say()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs="*", default=[1015, 241])
    ap.add_argument("--counts", type=int, nargs="*", default=[1, 1000, 100000])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--numpy-rows", type=int, default=10000, help="boxes of the NumPy closed-form timing (scaled up)")
    ap.add_argument("--mesh-rows", type=int, default=200, help="boxes of the mesh-and-sum timing (scaled up)")
    ap.add_argument("--no-ratios", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_region.txt"))
    args = ap.parse_args()
    say("tools/bench_region.py: one box, one run; kernels by HIP events, median of %d calls after 2 warm-ups" % args.repeats)
    for d in args.dims:
        one_dim(d, args)
    if not args.no_ratios:
        ratios()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
