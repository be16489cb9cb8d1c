"""SSPBinder on the GPU (csrc/ssn_bind.hip): every length and route against the direct float64 circular sum, under the bars of
bind_checks; pairing, invert flags, scratch sizes, operand locations and strides, normalisation, the planned route, space.bind and
harness.vector_query through it, and the example's --vector-queries."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bind_checks as bc
from sspslam_amd import SSPBinder, harness as H
from sspslam_amd.sspspace import SPSpace

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64_LENGTHS = tuple(d for d in bc.LENGTHS if d <= 3751)


def _torch():
    import torch
    return torch


# -- every length: the bar, zero rows, row counts, the route -------------------------------------------------------------------
@pytest.mark.parametrize("d", bc.LENGTHS)
def test_every_length_f32(d):
    route = bc.plan(d)
    n = bc.n_rows(d)
    A, B = bc.pairs(d, n)
    ref = bc.direct(A, B)
    with SSPBinder(d) as binder:
        out = binder.bind(A, B)
        info = binder.info(n)
        one, three = binder.bind(A[:1], B[:1]), binder.bind(A[:3], B[:3])
    assert out.shape == (n, d) and out.dtype == np.float64
    r = bc.worst(out, ref, bc.bar32(A, B, bc.C[route.cls]))
    print(f"d {d} {route!r}: {n} rows, worst |error| / bar = {r:.3f} (c = {bc.C[route.cls]})")
    assert r <= 1.0
    zero = (np.abs(A).sum(1) == 0) | (np.abs(B).sum(1) == 0)
    assert zero.sum() == 2 and not np.any(out[zero]) and not np.any(np.signbit(out[zero]))
    # n = 1, 3: a row's bits do not depend on how many rows ride with it
    assert one.tobytes() == out[:1].tobytes() and three.tobytes() == out[:3].tobytes()
    # the route the binder planned is the restated one
    assert (info["d"], info["bluestein_m"], info["radices"]) == route.key()
    assert info["transform_length"] == route.L and info["threads"] == route.threads and info["lds_bytes"] == 24 * route.L
    assert info["n_chunks"] == 1 and info["last_launches"] == 1 and info["last_kernel_ms"] > 0


@pytest.mark.parametrize("d", F64_LENGTHS)
def test_every_length_f64(d):
    n = bc.n_rows(d)
    A, B = bc.pairs(d, n)
    with SSPBinder(d, dtype="f64") as binder:
        out = binder.bind(A, B)
        info = binder.info(n)
    r = bc.worst(out, bc.direct(A, B), bc.bar64(A, B))
    print(f"d {d} f64: {n} rows, worst |error| / bar = {r:.3f}")
    assert r <= 1.0
    assert info["bluestein_m"] == 0 and info["radices"] == () and info["lds_bytes"] == 16 * d and info["threads"] == min(1024, (d + 63) // 64 * 64)


def test_unsupported_lengths_are_named():
    with pytest.raises(ValueError, match="SSN_EUNSUPPORTED.*d 3203"):
        SSPBinder(3203)
    with pytest.raises(ValueError, match="SSN_EUNSUPPORTED.*d 10001"):
        SSPBinder(10001, dtype="f64")
    with SSPBinder(3203, dtype="f64") as binder:          # the parity mode takes it
        A, B = bc.pairs(3203, 3)
        assert bc.worst(binder.bind(A, B), bc.direct(A, B), bc.bar64(A, B)) <= 1.0


# -- pairing, flags, scratch, location: bit-equal to the plain call ------------------------------------------------------------
@pytest.mark.parametrize("dtype", ("f32", "f64"))
def test_pairing(dtype):
    d, S, L = 55, 3, 5
    A, B = bc.pairs(d, S * L)
    P = A[:S]
    with SSPBinder(d, dtype=dtype) as binder:
        want = binder.bind(P[bc.pair_index(S * L, S)], B)                     # count n on both sides
        assert binder.bind(P, B.reshape(S, L, d)).tobytes() == want.tobytes()                 # n / L: (S, d) x (S, L, d)
        assert binder.bind(P, B.reshape(S, L, d)).shape == (S, L, d)
        assert binder.bind(P, B).tobytes() == want.tobytes()                                  # ... and flat
        assert binder.bind(B.reshape(S, L, d), P).tobytes() == binder.bind(B, P[bc.pair_index(S * L, S)]).tobytes()
        assert binder.bind(P[0], B).tobytes() == binder.bind(np.repeat(P[:1], S * L, 0), B).tobytes()      # count 1
        assert binder.bind(B, P[1]).tobytes() == binder.bind(B, np.repeat(P[1:2], S * L, 0)).tobytes()
        assert binder.bind(P[0], P[1]).shape == (1, d)
        with pytest.raises(ValueError, match="do not pair"):
            binder.bind(A[:2], B)
        rc = binder._lib.ssn_binder_bind(binder._h, A.ctypes.data, 2, B.ctypes.data, S * L, S * L, 0, 1e-8, np.empty((S * L, d)).ctypes.data)
        assert rc == -1
        bar = bc.bar32(P[bc.pair_index(S * L, S)], B, bc.C["direct"]) if dtype == "f32" else bc.bar64(P[bc.pair_index(S * L, S)], B)
        assert bc.worst(want, bc.direct(P[bc.pair_index(S * L, S)], B), bar) <= 1.0


@pytest.mark.parametrize("dtype", ("f32", "f64"))
@pytest.mark.parametrize("d", (55, 58, 151))
def test_invert_flags_are_an_index(d, dtype):
    A, B = bc.pairs(d, 20)
    with SSPBinder(d, dtype=dtype) as binder:
        for ia in (False, True):
            for ib in (False, True):
                got = binder.bind(A, B, invert_a=ia, invert_b=ib)
                want = binder.bind(bc.invert(A) if ia else A, bc.invert(B) if ib else B)
                assert got.tobytes() == want.tobytes(), (ia, ib)
        ref = bc.direct(bc.invert(A), B)
        bar = bc.bar32(A, B, bc.C[bc.plan(d).cls]) if dtype == "f32" else bc.bar64(bc.invert(A), B)
        assert bc.worst(binder.bind(A, B, invert_a=True), ref, bar) <= 1.0


@pytest.mark.parametrize("dtype", ("f32", "f64"))
def test_scratch_size_never_changes_a_bit(dtype):
    d, S, L = 151, 3, 5
    A, B = bc.pairs(d, S * L)
    P = A[:S]
    torch = _torch()
    with SSPBinder(d, dtype=dtype) as binder:
        want = binder.bind(P, B.reshape(S, L, d), invert_a=True, normalize=True, norm_floor=1e-6)
        assert binder.info(S * L)["n_chunks"] == 1 and binder.info()["scratch_bytes"] == 64 << 20
    for scratch, chunk in ((24 * d, 1), (4 * 24 * d, 4), (7 * 24 * d + 100, 7)):          # 4 and 7: seams inside groups of L = 5
        with SSPBinder(d, dtype=dtype, scratch_bytes=scratch) as binder:
            info = binder.info(S * L)
            assert info["row_chunk"] == chunk and info["n_chunks"] == -(-S * L // chunk) and info["min_scratch_bytes"] == 24 * d
            got = binder.bind(P, B.reshape(S, L, d), invert_a=True, normalize=True, norm_floor=1e-6)
            assert got.tobytes() == want.tobytes(), scratch
            assert binder.info()["last_launches"] == info["n_chunks"]
            dev = binder.bind(torch.tensor(P, device="cuda"), B.reshape(S, L, d), invert_a=True, normalize=True, norm_floor=1e-6)      # one side staged
            assert dev.tobytes() == want.tobytes(), scratch
    with pytest.raises(ValueError, match="too small for one row"):
        SSPBinder(d, dtype=dtype, scratch_bytes=24 * d - 1)


@pytest.mark.parametrize("dtype", ("f32", "f64"))
def test_operand_location_dtype_and_stride(dtype):
    torch = _torch()
    d, n = 58, 37
    A, B = bc.pairs(d, n)
    tdtype = torch.float32 if dtype == "f32" else torch.float64
    with SSPBinder(d, dtype=dtype) as binder:
        want = binder.bind(A, B)
        assert binder.bind(A, B).tobytes() == want.tobytes()                                     # run to run
        forms = {"host f32": lambda X: X.astype(np.float32),
                 "device f64": lambda X: torch.tensor(X, device="cuda"),
                 "device f32": lambda X: torch.tensor(X, device="cuda", dtype=torch.float32),
                 "device f64 strided": lambda X: torch.tensor(np.pad(X, ((0, 0), (3, 10))), device="cuda")[:, 3:3 + d],
                 "device f32 strided": lambda X: torch.tensor(np.pad(X, ((0, 0), (0, 7))), device="cuda", dtype=torch.float32)[:, :d],
                 "host strided": lambda X: np.pad(X, ((0, 0), (2, 2)))[:, 2:2 + d]}
        for name_a, fa in forms.items():
            for name_b, fb in (("host f64", lambda X: X), ("device f32 strided", forms["device f32 strided"]), (name_a, fa)):
                got = binder.bind(fa(A), fb(B))
                assert got.dtype == np.float64 and got.tobytes() == want.tobytes(), (name_a, name_b)
        dev = binder.bind(forms["device f32"](A), B, out="device")
        assert dev.is_cuda and dev.dtype == tdtype and dev.shape == (n, d)
        assert dev.cpu().double().numpy().tobytes() == want.tobytes()
        # into=: a wide caller's tensor, nothing outside [:n, :d] touched
        into = torch.full((n + 2, d + 9), 7.0, dtype=tdtype, device="cuda")
        res = binder.bind(A, forms["device f64 strided"](B), into=into)
        assert res is into
        host = into.cpu().double().numpy()
        assert host[:n, :d].tobytes() == want.tobytes() and np.all(host[n:] == 7.0) and np.all(host[:, d:] == 7.0)
        with pytest.raises(ValueError, match="into must be"):
            binder.bind(A, B, into=torch.zeros((n, d - 1), dtype=tdtype, device="cuda"))
        with pytest.raises(ValueError, match="must be"):
            binder.bind(A[:, :-1], B)
        assert binder.bind(np.zeros((0, d)), np.zeros((0, d))).shape == (0, d)
    with pytest.raises(Exception, match="closed"):
        binder.bind(A, B)


# -- normalise -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ("f32", "f64"))
@pytest.mark.parametrize("floor", (1e-8, 1e-6))
def test_normalize(dtype, floor):
    for d in (55, 151, 1015):
        A, B = bc.pairs(d, 30)
        B = B * np.where(np.arange(30) % 5 == 4, 2.0 ** -40, 1.0)[:, None]          # every fifth product lies under both floors
        ref = bc.direct(A, B)
        nrm = np.linalg.norm(ref, axis=1)
        assert np.any((nrm > 0) & (nrm < floor)) and np.any(nrm > 1) and not np.any(np.abs(nrm / floor - 1) < 1e-3)
        bar, u = (bc.bar32(A, B, bc.C[bc.plan(d).cls]), bc.U32) if dtype == "f32" else (bc.bar64(A, B), bc.U64)
        with SSPBinder(d, dtype=dtype) as binder:
            got = binder.bind(A, B, normalize=True, norm_floor=floor)
        r = bc.worst(got, bc.normalized(ref, floor), bc.bar_normalized(ref, bar, floor, u))
        print(f"d {d} {dtype} floor {floor:g}: normalised rows, worst |error| / bar = {r:.3f}")
        assert r <= 1.0
        unit = np.linalg.norm(got, axis=1)
        assert np.allclose(unit[nrm >= floor], 1.0, atol=1e-5) and np.all(unit[nrm < floor] < 1.0)


# -- the spaces and the harness ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ("hip", "hip-f64"))
def test_space_bind_backends(backend):
    rng = np.random.RandomState(7)
    s = H.make_ssp_space(2, ssp_dim=151)
    v = SPSpace(6, 58, seed=1)
    pts = rng.uniform(-0.8, 0.8, (9, 2))
    for space, a, b in ((s, s.encode(pts).astype(np.float32).astype(np.float64), s.encode(pts[::-1]).astype(np.float32).astype(np.float64)),
                        (v, v.vectors.astype(np.float32).astype(np.float64), v.inverse_vectors.astype(np.float32).astype(np.float64)[::-1])):
        got = space.bind(a, b, backend=backend)
        d = a.shape[1]
        bar = bc.bar32(a, b, bc.C[bc.plan(d).cls]) if backend == "hip" else bc.bar64(a, b)
        assert got.shape == a.shape and bc.worst(got, bc.direct(a, b), bar) <= 1.0
        assert np.allclose(got, space.bind(a, b), atol=1e-5)
        assert space.bind(a[0], b[0], backend=backend).shape == (1, d)
    assert len(s._binder_cache) == 1
    s._drop_decoders()
    assert "_binder_cache" not in s.__dict__


@pytest.mark.parametrize("backend", ("hip", "hip-f64"))
def test_vector_query_on_the_device(backend):
    """Against backend=None.  The device path binds the poses its own encoder made (clean_up(encode="device")), so the bar of
    vec_ssps is the binder's plus the encoder's own bar (encode_checks) carried through the binding - sum_i E_i |b_(j-i)| - both
    propagated through the normalisation.  vec_est has to be equal: the inputs are chosen so that every float64 decode - of the
    poses and of the unbound rows - has a top-two gap above the decoder tests' f32 bar."""
    import decoding_checks as dk
    import encode_checks as ec
    n, S, L, d = 41, 4, 3, 55
    s = H.make_ssp_space(2, ssp_dim=d)
    table, points = s.get_sample_pts_and_ssps(n, "grid")
    pitch = (s.domain_bounds[:, 1] - s.domain_bounds[:, 0]) / (n - 1)
    rng = np.random.RandomState(3)
    # items 0.3 and poses -0.1 of a pitch off grid points of the inner part of the domain: every decode is unambiguous, and so is
    # item - (cleaned-up pose), 0.3 of a pitch off a grid point
    lo = s.domain_bounds[:, 0]
    item = lo + rng.randint(12, 29, (L, 2)) * pitch + 0.3 * pitch
    path = lo + rng.randint(12, 29, (S, 2)) * pitch - 0.1 * pitch
    frames = (np.repeat(s.encode(item)[None], S, axis=0) * (1 + 0.05 * rng.randn(S, L, 1))).astype(np.float32).astype(np.float64)
    poses = (s.encode(path) + 0.01 * rng.randn(S, d)).astype(np.float32).astype(np.float64)
    want = H.vector_query(s, poses, frames, num_samples=n)
    assert dk.Reference(table, poses).guard() and dk.Reference(table, want["vec_ssps"].reshape(S * L, d)).guard()
    got = H.vector_query(s, poses, frames, num_samples=n, backend=backend)
    assert np.array_equal(got["vec_est"], want["vec_est"])
    clean_pts = s.decode(poses, "from-set", "grid", n)
    E = ec.Reference(s, clean_pts).bar("f32" if backend == "hip" else "f64")
    a = bc.invert(s.encode(clean_pts))[bc.pair_index(S * L, S)]
    b = frames.reshape(S * L, d)
    ref = bc.direct(a, b)
    bar = (bc.bar32(a, b, bc.C["direct"]) if backend == "hip" else bc.bar64(a, b)) + bc.direct(bc.invert(E)[bc.pair_index(S * L, S)], np.abs(b))
    r = bc.worst(got["vec_ssps"].reshape(S * L, d), want["vec_ssps"].reshape(S * L, d),
                 bc.bar_normalized(ref, bar, 1e-6, bc.U32 if backend == "hip" else bc.U64) + 1e-15)
    print(f"vector_query {backend}: vec_ssps worst |error| / bar = {r:.3f}")
    assert r <= 1.0
    cos_err, dist_err = H.vector_query_errors(s, got, item[None] - path[:, None])
    assert np.all(dist_err <= 2 * np.linalg.norm(pitch))


def test_example_vector_queries(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "run_slam.py"), "--ssp-dim", "55", "--pi-n-neurons", "100", "--mem-n-neurons", "110",
           "--circonv-n-neurons", "20", "--n-landmarks", "3", "--view-rad", "0.6", "--T", "2.0", "--limit", "0.5", "--n-eval-points", "200",
           "--decode-backend", "hip", "--map-every", "0.5", "--vector-queries", "--save", "--save-dir", str(tmp_path)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "vector queries:" in run.stdout and "cosine error" in run.stdout and "distance error" in run.stdout
    saved = [f for f in os.listdir(tmp_path) if f.endswith(".npz")]
    assert len(saved) == 1
    with np.load(os.path.join(tmp_path, saved[0]), allow_pickle=True) as z:
        assert z["landmark_vec_est"].shape == (4, 3, 2)
        assert z["landmark_vec_cos_err"].shape == (4, 3) and z["landmark_vec_dist_err"].shape == (4, 3)
        assert np.all(np.isfinite(z["landmark_vec_dist_err"]))
