"""Binding on the GPU (binding.SSPBinder: k_bind_rows, k_bind_direct) against NumPy's SSPSpace.bind and a torch.fft composition.

usage: python tools/bench_bind.py [d1015] [d151] [d3751] [pairing] [--pairs N] [--repeats R] [--host-rows M] [--out FILE]

  d1015    N pairs (default 100 000) at d = 1015 (29 * 7 * 5, direct), f32 and f64 (the f64 binder on N / 10 pairs, scaled)
  d151     N pairs at d = 151, the default HexagonalSSPSpace: the chirp-z route (M = 320)
  d3751    N / 4 pairs at d = 3751 (31 * 11 * 11, direct)
  pairing  the vector queries of examples/run_slam.py --map-every at its README shape: S = 200 pose rows x L = 10 landmark rows at
           d = 1015, (S, d) x (S, L, d) with invert_a and normalize

Per case, operands and result left on the device as f32 tensors: device milliseconds of the binder's kernels alone (HIP events of
ssn_binder_get_info) and nanoseconds per pair; the same pairs through torch.fft.irfft(torch.fft.rfft(a) * torch.fft.rfft(b), n=d) on
the same tensors (torch.cuda events around the three calls); and np.fft through SSPSpace.bind on --host-rows pairs on the host, scaled
to N (said so on the line).  2 warm-up calls, then the median of --repeats calls, one process.  Everything is written to --out
(default profiles/bind_rows.txt) as well as printed."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from sspslam_amd import SSPBinder, harness as H

LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def fmt(x):
    x = np.asarray(x, dtype=float)
    return "median %.3f ms (min %.3f, max %.3f, %d calls)" % (np.median(x), x.min(), x.max(), len(x))


def kernel_ms(binder, call, repeats):
    for _ in range(2):
        call()
    out = []
    for _ in range(repeats):
        call()
        out.append(binder.info()["last_kernel_ms"])
    return np.array(out)


def torch_ms(fn, repeats):
    import torch
    for _ in range(2):
        fn()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return np.array(out)


def case(name, d, n, args, group=0):
    import torch
    rng = np.random.RandomState(d)
    space = H.make_ssp_space(2, ssp_dim=d) if d in (151, 1015) else None
    n_a = n // group if group else n
    a = torch.tensor(rng.randn(n_a, d), dtype=torch.float32, device="cuda")
    b = torch.tensor(rng.randn(n, d), dtype=torch.float32, device="cuda")
    kw = dict(invert_a=True, normalize=True, norm_floor=1e-6) if group else {}
    say("case %s: %d pairs at d = %d%s" % (name, n, d, ", %d pose rows x %d landmark rows, invert_a, normalize" % (n_a, group) if group else ""))
    with SSPBinder(d) as binder:
        info = binder.info(n)
        ms = kernel_ms(binder, lambda: binder.bind(a, b, out="device", **kw), args.repeats)
        say("  route: L = %d, M = %d, radices %s, %d threads, %d B of LDS per workgroup; %d chunk(s) of %d rows" % (
            info["transform_length"], info["bluestein_m"], info["radices"], info["threads"], info["lds_bytes"], info["n_chunks"], info["row_chunk"]))
        say("  k_bind_rows (f32):        %s -> %.1f ns per pair" % (fmt(ms), 1e6 * np.median(ms) / n))
        got = binder.bind(a, b, out="device", **kw)
    aa = a.repeat_interleave(group, dim=0) if group else a

    def composed():
        x = aa[:, (-torch.arange(d, device="cuda")) % d] if group else aa
        c = torch.fft.irfft(torch.fft.rfft(x) * torch.fft.rfft(b), n=d)
        return c / torch.clamp(torch.linalg.norm(c, dim=1, keepdim=True), min=1e-6) if group else c

    tm = torch_ms(composed, args.repeats)
    say("  torch.fft composition:    %s -> %.1f ns per pair; k_bind_rows / torch = %.2f" % (fmt(tm), 1e6 * np.median(tm) / n, np.median(ms) / np.median(tm)))
    ref = composed()
    say("  largest |k_bind_rows - torch| = %.2e (largest |value| %.2e)" % (float((got - ref).abs().max()), float(ref.abs().max())))
    del ref, got
    n64 = max(1, n // 10)
    with SSPBinder(d, dtype="f64") as binder:
        ms64 = kernel_ms(binder, lambda: binder.bind(aa[:n64], b[:n64], out="device"), max(3, args.repeats // 2))
        say("  k_bind_direct (f64):      %s for %d pairs -> %.0f ns per pair, %.0f ms for %d" % (fmt(ms64), n64, 1e6 * np.median(ms64) / n64, np.median(ms64) * n / n64, n))
    m = min(n, args.host_rows)
    ah, bh = aa[:m].cpu().double().numpy(), b[:m].cpu().double().numpy()
    bind = space.bind if space is not None else (lambda x, y: np.fft.ifft(np.fft.fft(x, axis=1) * np.fft.fft(y, axis=1), axis=1).real)
    t0 = time.perf_counter()
    bind(ah, bh)
    t_host = 1e3 * (time.perf_counter() - t0)
    say("  NumPy bind (host, float64): %.0f ms for %d pairs%s -> %.0f ns per pair; host / k_bind_rows = %.0f x" % (
        t_host, m, "" if m == n else ", scaled to %d: %.0f ms" % (n, t_host * n / m), 1e6 * t_host / m, (t_host * n / m) / np.median(ms)))
    say()
    torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", default=["d1015", "d151", "d3751", "pairing"])
    ap.add_argument("--pairs", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-rows", type=int, default=10000, help="pairs of the host timing (scaled up)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bind_rows.txt"))
    args = ap.parse_args()
    say("tools/bench_bind.py %s: one box, one run, one process; kernels by HIP events, median of %d calls after 2 warm-ups" % (" ".join(args.cases), args.repeats))
    for c in args.cases:
        if c == "d1015":
            case(c, 1015, args.pairs, args)
        elif c == "d151":
            case(c, 151, args.pairs, args)
        elif c == "d3751":
            case(c, 3751, args.pairs // 4, args)
        elif c == "pairing":
            case(c, 1015, 2000, args, group=10)
        else:
            raise SystemExit("unknown case %r" % c)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
