"""Binding on the GPU, the part that needs no GPU: the float32 stand-in of k_bind_rows against the direct circular sum, the binder's
planner against dft_checks.plan, wrong binders, the untouched NumPy paths, the C ABI's errors and harness.vector_query in NumPy."""
import copy
import ctypes as C
import pickle

import numpy as np
import pytest

import bind_checks as bc
import dft_checks as dc
from sspslam_amd import SSPBinder, _lib, harness as H
from sspslam_amd.binding import backend_dtype
from sspslam_amd.sspspace import HexagonalSSPSpace, SPSpace


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# -- the stand-in and its constants ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", bc.LENGTHS)
def test_stand_in_stays_under_half_a_bar(d):
    route = bc.plan(d)
    A, B = bc.pairs(d, bc.n_rows(d))
    ref = bc.direct(A, B)
    out = bc.standin(route, A, B)
    r = bc.worst(out, ref, bc.bar32(A, B, bc.C[route.cls]))
    print(f"d {d} {route!r}: stand-in at {r:.3f} of the bar (c = {bc.C[route.cls]}, first-order worst case {bc.analytic_c(route):.0f})")
    assert r <= 0.5
    assert bc.C[route.cls] < bc.analytic_c(route) or d <= 3          # (d = 2, 3: one pass of 1 or 2 additions; the bound has no slack there)
    zero = (np.abs(A).sum(1) == 0) | (np.abs(B).sum(1) == 0)
    assert zero.any() and not np.any(out[zero])
    for floor in (1e-8, 1e-6):
        Bs = B * np.where(np.arange(len(B)) % 5 == 4, 2.0 ** -40, 1.0)[:, None]          # every fifth product lies under both floors
        refs = bc.direct(A, Bs)
        nb = bc.bar_normalized(refs, bc.bar32(A, Bs, bc.C[route.cls]), floor, bc.U32)
        rn = bc.worst(bc.standin(route, A, Bs, normalize=True, floor=floor), bc.normalized(refs, floor), nb)
        assert rn <= 0.5, (floor, rn)


def test_constants_are_twice_the_measured_worst_case():
    worst = {}
    for d in bc.LENGTHS:
        route = bc.plan(d)
        worst[route.cls] = max(worst.get(route.cls, 0.0), bc.standin_ratio(route, *bc.pairs(d, bc.n_rows(d))))
    for cls, r in worst.items():
        assert 0.9 * bc.C0[cls] <= r <= bc.C0[cls] and bc.C[cls] == 2.0 * bc.C0[cls], (cls, r)


# -- the planner ----------------------------------------------------------------------------------------------------------------
def test_planner_is_plan_dft_without_the_in_place_engine():
    for d in list(range(8, 257)) + [n for n, *_ in dc.LONG] + list(bc.LENGTHS[4:]) + [3200, 6400]:
        p, r = dc.plan(d, 1, False, True), bc.plan(d)
        assert (p.N, p.M, p.radices) == r.key() and not p.inplace and not p.N1, (d, p, r)
    assert bc.plan(2).key() == (2, 0, (2,)) and bc.plan(3).key() == (3, 0, (3,)) and bc.plan(7).key() == (7, 0, (7,))
    assert bc.plan(1) is None and bc.plan(6401) is None and bc.plan(3203) is None and bc.plan(3199).M == 6400
    assert bc.plan(55).radices == (11, 5) and bc.plan(1015).radices == (29, 7, 5) and bc.plan(3751).M == 0
    assert bc.plan(97).M and bc.plan(151).M and 3645 <= bc.plan(1801).M <= 4096
    assert bc.plan(3751).threads == 960 and bc.plan(6400).threads == 1024 and bc.plan(16).threads == 64


# -- wrong binders --------------------------------------------------------------------------------------------------------------
def _ratio(d, mut, rows=slice(None), **kw):
    route = bc.plan(d)
    A, B = bc.pairs(d)
    A, B = A[rows], B[rows]
    return bc.worst(bc.standin(route, A, B, mut=(mut,), **kw), bc.direct(A, B), bc.bar32(A, B, bc.C[route.cls]))


@pytest.mark.parametrize("name", bc.MUTANTS)
def test_wrong_binders_fail(name):
    assert name in bc.MUTANTS
    if name in ("mirror", "no-1-over-d", "no-conj-back"):
        assert _ratio(55, name) > 1 and _ratio(58, name) > 1 and _ratio(151, name) > 1
    elif name == "nyquist-complex":
        assert _ratio(58, name) > 1 and _ratio(16, name) > 1
        assert _ratio(55, name) <= 0.5              # an odd d has no such bin
    elif name == "invert-index":
        for d in (55, 58):
            route = bc.plan(d)
            A, B = bc.pairs(d)
            ref, bar = bc.direct(bc.invert(A), B), bc.bar32(A, B, bc.C[route.cls])
            assert bc.worst(bc.standin(route, A, B, invert_a=True), ref, bar) <= 0.5
            assert bc.worst(bc.standin(route, A, B, invert_a=True, mut=(name,)), ref, bar) > 1
            assert bc.worst(bc.standin(route, B, A, invert_b=True, mut=(name,)), bc.direct(B, bc.invert(A)), bar) > 1
    elif name == "pairing-mod":
        route = bc.plan(55)
        A, B = bc.pairs(55, 15)
        P = A[:3]                                   # S = 3 pose rows, L = 5 landmark rows each
        ref, bar = bc.direct(P[bc.pair_index(15, 3)], B), bc.bar32(P[bc.pair_index(15, 3)], B, bc.C["direct"])
        assert bc.worst(bc.standin(route, P[bc.pair_index(15, 3)], B), ref, bar) <= 0.5
        assert bc.worst(bc.standin(route, P[bc.pair_index(15, 3, (name,))], B), ref, bar) > 1
    elif name == "no-balance":
        for d in (55, 151, 1015):
            assert _ratio(d, name, [1]) > 1 and _ratio(d, name, [3]) > 1          # |b| = 2^-20 |a| and the reverse
            assert _ratio(d, name, [0, 2, 5, 7]) <= 0.5                          # rows of like norms do not need it
    elif name == "floor-ignored":
        route = bc.plan(55)
        A, B = bc.pairs(55)
        A, B = A[:1], B[:1] * 2.0 ** -30            # |a (*) b| ~ 1e-8, under the floor of the vector queries
        ref = bc.direct(A, B)
        assert np.linalg.norm(ref) < 1e-6
        bar = bc.bar_normalized(ref, bc.bar32(A, B, bc.C["direct"]), 1e-6, bc.U32)
        assert bc.worst(bc.standin(route, A, B, normalize=True, floor=1e-6), bc.normalized(ref, 1e-6), bar) <= 0.5
        assert bc.worst(bc.standin(route, A, B, normalize=True, floor=1e-6, mut=(name,)), bc.normalized(ref, 1e-6), bar) > 1
    else:
        assert name == "chirp-phase"
        assert _ratio(1801, name, slice(0, 3)) > 1 and _ratio(151, name) > 1
        assert _ratio(1015, name, slice(0, 3)) <= 0.5          # a direct route has no chirp


# -- the NumPy paths are what they were -----------------------------------------------------------------------------------------
def test_numpy_backend_is_byte_identical():
    rng = np.random.RandomState(5)
    s = H.make_ssp_space(2, ssp_dim=55)
    v = SPSpace(6, 32, seed=1)
    for space, d in ((s, s.ssp_dim), (v, v.dim)):
        for a, b in ((rng.randn(4, d), rng.randn(4, d)), (rng.randn(d), rng.randn(3, d)), (rng.randn(d), rng.randn(d))):
            want = np.fft.ifft(np.fft.fft(np.atleast_2d(a), axis=1) * np.fft.fft(np.atleast_2d(b), axis=1), axis=1).real
            for got in (space.bind(a, b), space.bind(a, b, backend=None), space.bind(a, b, backend="numpy")):
                assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
        a = rng.randn(3, d)
        assert space.invert(a).tobytes() == a[:, (-np.arange(d)) % d].tobytes()
    assert np.array_equal(v.inverse_vectors, v.invert(v.vectors))


def test_wrong_backend_names_and_arguments(lib):
    s = H.make_ssp_space(2, ssp_dim=7)
    v = SPSpace(3, 8, seed=0)
    for bad in ("cuda", "HIP", "", 3):
        with pytest.raises(ValueError, match="unknown bind backend"):
            s.bind(np.ones(7), np.ones(7), backend=bad)
        with pytest.raises(ValueError, match="unknown bind backend"):
            v.bind(np.ones(8), np.ones(8), backend=bad)
        with pytest.raises(ValueError, match="unknown bind backend"):
            H.vector_query(s, np.ones((2, 7)), np.ones((2, 3, 7)), 10, backend=bad)
    assert backend_dtype("hip") == "f32" and backend_dtype("hip-f64") == "f64" and backend_dtype(None) is None
    with pytest.raises(ValueError, match="dtype"):
        SSPBinder(7, dtype="bf16")
    with pytest.raises(ValueError, match="width or a space"):
        SSPBinder("seven")
    with pytest.raises(ValueError, match="pose_rows must be"):
        H.vector_query(s, np.ones((2, 7)), np.ones((3, 3, 7)), 10)
    with pytest.raises(ValueError, match="SSN_EUNSUPPORTED"):
        SSPBinder(3203)
    with pytest.raises(ValueError, match="SSN_EUNSUPPORTED"):
        SSPBinder(10001, dtype="f64")
    if lib.ssn_device_count() == 0:
        for space, d in ((s, 7), (v, 8)):
            for backend in ("hip", "hip-f64"):
                with pytest.raises(ValueError, match="no CPU fallback"):
                    space.bind(np.ones(d), np.ones(d), backend=backend)
        with pytest.raises(ValueError, match="no CPU fallback"):
            SSPBinder(s)
        with pytest.raises(ValueError, match="no CPU fallback"):
            H.vector_query(s, np.ones((2, 7)), np.ones((2, 3, 7)), 10, backend="hip")


def test_binder_cache_is_dropped_and_not_copied():
    class Handle:
        closed = False

        def close(self):
            self.closed = True

    s = HexagonalSSPSpace(2, ssp_dim=7, domain_bounds=np.array([[-1.0, 1.0], [-1.0, 1.0]]), length_scale=0.2)
    h = Handle()
    s._binder_cache = {("f32", 0): h}
    t = copy.deepcopy(s)
    assert "_binder_cache" not in t.__dict__ and t.ssp_dim == s.ssp_dim
    s.update_lengthscale(0.3)
    assert h.closed and "_binder_cache" not in s.__dict__
    v = SPSpace(3, 8, seed=0)
    v._binder_cache = {("f32", 0): Handle()}
    w = pickle.loads(pickle.dumps(v))
    assert "_binder_cache" not in w.__dict__ and np.array_equal(w.vectors, v.vectors)


# -- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_prototypes_and_abi_errors_need_no_gpu(lib):
    for name in ("ssn_binder_create", "ssn_binder_destroy", "ssn_binder_bind", "ssn_binder_bind_device", "ssn_binder_get_info"):
        assert name in _lib.EXPORTS and getattr(lib, name).argtypes == _lib.EXPORTS[name][1]
    assert b"ABI 11" in lib.ssn_version() and _lib.SSN_ABI_VERSION == 11
    assert C.sizeof(_lib.BinderInfo) == 8 * 24
    assert (_lib.SSN_BIND_INVERT_A, _lib.SSN_BIND_INVERT_B, _lib.SSN_BIND_NORMALIZE) == (1, 2, 4)
    h = C.c_void_p()

    def create(dtype=0, d=55, scratch=0, out=C.byref(h)):
        return lib.ssn_binder_create(dtype, 0, d, scratch, out)

    assert create(out=None) == -1 and b"null handle" in lib.ssn_last_error()
    assert create(dtype=7) == -1 and b"dtype" in lib.ssn_last_error()
    assert create(d=1) == -1 and b"d 1 below 2" in lib.ssn_last_error()
    assert create(scratch=-1) == -1 and b"negative scratch_bytes" in lib.ssn_last_error()
    assert create(scratch=100) == -1 and b"too small for one row" in lib.ssn_last_error()
    assert create(d=3203) == -5 and b"SSN_EUNSUPPORTED" in lib.ssn_last_error() and b"d 3203" in lib.ssn_last_error()
    assert create(d=6401) == -5 and b"SSN_EUNSUPPORTED" in lib.ssn_last_error()
    assert create(dtype=1, d=10001) == -5 and b"SSN_EUNSUPPORTED" in lib.ssn_last_error() and b"d 10001" in lib.ssn_last_error()
    assert not h.value
    x, out = np.zeros((4, 55)), np.zeros((4, 55))
    assert lib.ssn_binder_bind(None, x.ctypes.data, 4, x.ctypes.data, 4, 4, 0, 1e-8, out.ctypes.data) == -1 and b"null binder" in lib.ssn_last_error()
    assert lib.ssn_binder_bind_device(None, x.ctypes.data, 0, 1, 55, 4, x.ctypes.data, 0, 1, 55, 4, 4, 0, 1e-8, None, 55) == -1
    assert b"null binder" in lib.ssn_last_error()
    assert lib.ssn_binder_get_info(None, 4, None) == -1
    lib.ssn_binder_destroy(None)                           # like free(NULL)
    if lib.ssn_device_count() == 0:
        assert create() == -2 and b"no HIP device available (there is no CPU fallback)" in lib.ssn_last_error()
        assert create(dtype=1, d=10000) == -2 and b"no CPU fallback" in lib.ssn_last_error()
    assert not h.value


# -- harness.vector_query in NumPy -------------------------------------------------------------------------------------------
def test_vector_query_numpy_is_the_scripts_four_lines():
    n = 41
    s = H.make_ssp_space(2, ssp_dim=55)
    lo, hi = s.domain_bounds[:, 0], s.domain_bounds[:, 1]
    pitch = (hi - lo) / (n - 1)
    rng = np.random.RandomState(11)
    item = rng.uniform(-0.4, 0.4, (3, 2))
    path = rng.uniform(-0.4, 0.4, (4, 2))
    frames = np.repeat(s.encode(item)[None], 4, axis=0)              # encode(item), bound with nothing
    poses = s.encode(path) + 0.01 * rng.randn(4, 55)                 # a noisy pose estimate: clean-up has something to do
    res = H.vector_query(s, poses, frames, num_samples=n)
    true = item[None, :, :] - path[:, None, :]
    assert res["vec_ssps"].shape == (4, 3, 55) and res["vec_est"].shape == (4, 3, 2)
    # (clean-up snaps the pose to the grid, the decode snaps the vector: within a pitch each)
    assert np.all(np.abs(res["vec_est"] - true) <= 2 * pitch * (1 + 1e-9))
    cos_err, dist_err = H.vector_query_errors(s, res, true)
    assert cos_err.shape == dist_err.shape == (4, 3) and np.all(dist_err <= 2 * np.linalg.norm(pitch)) and np.all(cos_err < 0.2)
    # the script, written out (slam_map_new.py:432-441, 453, 480-484)
    sample_ssps, sample_points = s.get_sample_pts_and_ssps(n)
    inv_ssps = s.invert(sample_ssps[np.argmax(sample_ssps @ poses.T, axis=0), :])
    for j in range(3):
        res1 = s.bind(inv_ssps, frames[:, j])
        res1 = res1 / np.maximum(1e-6, np.sqrt(np.sum(res1 ** 2, axis=1))).reshape(-1, 1)
        np.testing.assert_allclose(res["vec_ssps"][:, j], res1, rtol=0, atol=1e-14)
        dec = sample_points[np.argmax(sample_ssps @ res1.T, axis=0), :]
        assert np.array_equal(res["vec_est"][:, j], dec)
    # exact poses, no clean-up: item - path to within one pitch
    res = H.vector_query(s, s.encode(path), frames, num_samples=n, clean_up=False)
    assert np.all(np.abs(res["vec_est"] - true) <= 0.5 * pitch * (1 + 1e-9) + 1e-12)
    assert H.vector_query(s, np.zeros((0, 55)), np.zeros((0, 3, 55)))["vec_est"].shape == (0, 3, 2)
