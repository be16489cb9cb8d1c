"""Wall time of small calls of the three device services - 100 rows at d = 151, device operands, out="device" or into= - where
the Python wrapper (service.py) and the host half of the call dominate, not the kernels.  One process; per line the median over 7
batches of the mean microseconds per call in a batch of 300, after 100 warm-up calls.

    python tools/bench_service_calls.py [ROOT]      # ROOT: another tree with its own built library, for an A / B"""
import os
import sys
import time

ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from sspslam_amd import SSPBinder, SSPEncoder, harness as H
from sspslam_amd.decoding import GridDecoder

import sspslam_amd
assert os.path.abspath(sspslam_amd.__path__[0]).startswith(ROOT), sspslam_amd.__path__

N, d = 100, 151
rng = np.random.RandomState(0)
space = H.make_ssp_space(2, ssp_dim=d)
pts = torch.tensor(rng.uniform(-0.9, 0.9, (N, 2)), device="cuda")
rows = torch.tensor(space.encode(pts.cpu().numpy()), dtype=torch.float32, device="cuda")
lo = rng.uniform(-0.9, 0.5, (N, 2))
boxes = torch.tensor(np.stack([lo, lo + 0.2], axis=2), device="cuda")
other = torch.tensor(rng.randn(N, d), dtype=torch.float32, device="cuda")


def timed(name, call):
    for _ in range(100):
        call()
    torch.cuda.synchronize()
    per = []
    for _ in range(7):
        t0 = time.perf_counter()
        for _ in range(300):
            call()
        per.append(1e6 * (time.perf_counter() - t0) / 300)
    print("small call | %-48s median %8.2f us per call (min %.2f, max %.2f, 7 batches of 300)" % (name, np.median(per), min(per), max(per)), flush=True)


with GridDecoder(space, 40) as dec, SSPEncoder(space, dtype="f32") as enc, SSPBinder(d) as binder:
    into = torch.empty((N, dec.n_samples), dtype=torch.float32, device="cuda")
    out = torch.empty((N, d), dtype=torch.float32, device="cuda")
    timed("GridDecoder.indices", lambda: dec.indices(rows))
    timed("GridDecoder.similarity out=device", lambda: dec.similarity(rows, out="device"))
    timed("GridDecoder.similarity into=", lambda: dec.similarity(rows, into=into))
    timed("SSPEncoder.encode out=device", lambda: enc.encode(pts, out="device"))
    timed("SSPEncoder.encode_region out=device", lambda: enc.encode_region(boxes, out="device"))
    timed("SSPBinder.bind out=device", lambda: binder.bind(rows, other, out="device"))
    timed("SSPBinder.bind into=", lambda: binder.bind(rows, other, into=out))
print("done", flush=True)
