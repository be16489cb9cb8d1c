"""The encoder without a GPU: the instrument of tests/encode_checks.py (its stand-ins pass, every wrong encoder fails, C comes from
the stand-in), SSPSpace.encode(backend=None) byte for byte what it was, the argument errors of the Python layer and the prototypes."""
import copy
import ctypes as C

import numpy as np
import pytest

import encode_checks as ec
from sspslam_amd import _lib
from sspslam_amd.sspspace import HexagonalSSPSpace, SSPSpace

B2 = np.array([[-1.0, 1.0], [-1.0, 1.0]])


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# -- the instrument -----------------------------------------------------------------------------------------------------------
def test_identity_reproduces_encode_and_c_comes_from_the_stand_in():
    c0, per = ec.measure_c0()
    print("worst |error| / (REL S_c) of the f32 stand-in per case:", {k: round(v, 3) for k, v in per.items()}, "c0 =", round(c0, 4))
    assert 0.9 * ec.C0 <= c0 <= ec.C0 and ec.C == 2 * ec.C0 and ec.REL == 1.5e-7 + 2 * 2.0 ** -24
    for name in ec.CASES:
        ref = ec.reference(name)
        assert ref.x.shape[0] == 130 and 2 * ref.K <= 1024          # the range REL is stated for
        ref.check(ec.f64_stand_in(ref.space, ref.x), "f64", label=f"stand-in {name}")
        ref.check(ec.f32_stand_in(ref.space, ref.x), "f32", label=f"stand-in {name}")
        for n in ec.NS:                                             # a prefix is held to the same bars
            assert ref.ratio(ec.f64_stand_in(ref.space, ref.x[:n]), "f64", slice(0, n)).max() <= 1.0
        sp = ec.special_reference(name)
        sp.check(ec.f64_stand_in(sp.space, sp.x), "f64", label=f"stand-in, special points {name}")
        sp.check(ec.f32_stand_in(sp.space, sp.x), "f32-format", label=f"stand-in, special points {name}")
    assert [ec.reference(n).K for n in ec.CASES] == [2, 49, 64, 65, 101, 64, 508]


def test_far_case_separates_f32_phases():
    ref = ec.reference(ec.FAR)
    _, M, _ = ref.space.refine_tables()
    th = np.abs(ref.x @ M.T).max()
    assert 900 < th < 1500 and np.all(ref.space.length_scale == 0.2) and np.abs(ref.x).max() <= 50
    ref.check(ec.f32_stand_in(ref.space, ref.x), "f32", label="stand-in far")
    ref.check(ec.f64_stand_in(ref.space, ref.x), "f64", label="stand-in far", phases=True)
    wrong = ref.ratio(ec.f32_stand_in(ref.space, ref.x, f32_phases=True), "f32").max()
    print(f"far case: |th| up to {th:.0f} rad, f32 phases miss the f32 bar by {wrong:.1f}")
    assert wrong >= 3.0
    # and the reference's own phase rounding is why the far case carries the phase term in f64
    print(f"far case: the float64 stand-in sits at {ref.ratio(ec.f64_stand_in(ref.space, ref.x), 'f64').max():.2f} of the plain f64 bar")


@pytest.mark.parametrize("name", list(ec.MUTANTS))
def test_wrong_encoders_fail(name):
    wrong = ec.MUTANTS[name]
    for case in ("d97-2d", "d201-3d", "d64-full"):
        ref = ec.reference(case)
        got = wrong(ref.space, ref.x[:16])
        for mode in ("f64", "f32"):
            worst = ref.ratio(got, mode, slice(0, 16)).max()
            assert worst > 100.0, (name, case, mode, worst)
            with pytest.raises(AssertionError):
                ref.check(got, mode, slice(0, 16))
    ref = ec.reference("d97-2d")
    np.testing.assert_array_less(ref.ratio(ec._mutant(ref.space, ref.x), "f64"), 1.0)      # unmutated, it is the identity


def test_w0_doubled_in_unit_bars():
    ref = ec.reference("d1015-2d")
    r = np.abs(ec.MUTANTS["w0 doubled"](ref.space, ref.x[:8]) - ref.want[:8]) / (ec.REL * ref.S[:8])
    assert r.min() > 1000                                           # 1 / d on every entry against REL S_c


# -- SSPSpace.encode ----------------------------------------------------------------------------------------------------------
def old_encode(s, x):
    x = np.atleast_2d(np.asarray(x, dtype=float))
    return np.fft.ifft(np.exp(1j * ((x / s.length_scale.reshape(1, -1)) @ s.phase_matrix.T)), axis=1).real


def test_numpy_backend_is_byte_identical(golden):
    g = golden("ssp_spaces.npz")
    spaces = [(HexagonalSSPSpace(2, ssp_dim=55, domain_bounds=B2, length_scale=0.2), g["hex2_55_decoded"]),
              (HexagonalSSPSpace(1, ssp_dim=37, domain_bounds=np.array([[-2.0, 2.0]]), length_scale=0.5), np.linspace(-2, 2, 9)[:, None]),
              (SSPSpace(3, 1801, g["hex3_phase"], domain_bounds=np.tile([-1.0, 1.0], (3, 1)), length_scale=0.2), g["hex3_pts"]),
              (ec.case_space("d64-full"), ec.case_points("d64-full"))]
    for s, x in spaces:
        want = old_encode(s, x)
        for kw in ({}, {"backend": None}, {"backend": "numpy"}):
            got = s.encode(x, **kw)
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    s, x = spaces[0]
    assert s.clean_up(g["hex2_55_noisy"], "from-set", "grid", 31).tobytes() == old_encode(s, g["hex2_55_decoded_31"]).tobytes()
    assert s.clean_up(g["hex2_55_noisy"], "from-set", "grid", 31, encode_backend=None).tobytes() == old_encode(s, g["hex2_55_decoded_31"]).tobytes()
    # and the golden rows of the reference project's own encode are still met
    np.testing.assert_allclose(s.get_sample_pts_and_ssps(100, "grid")[0][[0, 1, 99, 100, 5050, 9999]], g["hex2_55_grid_ssps_rows"], atol=1e-12)


def test_argument_errors_of_the_python_layer(lib):
    from sspslam_amd import SSPEncoder, harness as H
    from sspslam_amd.decoding import GridDecoder
    s = H.make_ssp_space(2, ssp_dim=7)
    rows = np.ones((2, 7))
    for bad in ("cuda", "HIP", "", 3):
        with pytest.raises(ValueError, match="unknown encode backend"):
            s.encode(np.zeros((1, 2)), backend=bad)
        with pytest.raises(ValueError, match="unknown encode backend"):
            s.clean_up(rows, "from-set", "grid", 10, encode_backend=bad)
    with pytest.raises(ValueError, match="dtype"):
        SSPEncoder(s, dtype="bf16")
    with pytest.raises(ValueError, match="SSPSpace"):
        SSPEncoder(None)
    with pytest.raises(ValueError, match="table must be"):
        GridDecoder(s, 10, table="gpu")
    with pytest.raises(ValueError, match="already holds the SSPs"):
        GridDecoder(s, samples=(np.eye(3), np.eye(3)), table="device")
    with pytest.raises(ValueError, match="table must be"):
        s.decode(rows, "from-set", "grid", 10, table="gpu")
    with pytest.raises(ValueError, match="needs a hip backend"):
        s.decode(rows, "from-set", "grid", 10, table="device")
    with pytest.raises(ValueError, match="needs a hip backend"):
        H.pathint_metrics(s, rows, rows, np.zeros((2, 2)), 10, table="device")
    # defaults: the harness hands no table= on, and the host decode is what it was
    np.testing.assert_array_equal(H.pathint_metrics(s, rows, rows, np.zeros((2, 2)), 10)[0], s.decode(rows, "from-set", "grid", 10))
    np.testing.assert_array_equal(H.pathint_metrics(s, rows, rows, np.zeros((2, 2)), 10, table="host")[0], s.decode(rows, "from-set", "grid", 10))
    if lib.ssn_device_count() == 0:
        with pytest.raises(ValueError, match="no CPU fallback"):
            SSPEncoder(s)
        with pytest.raises(ValueError, match="no CPU fallback"):
            s.encode(np.zeros((1, 2)), backend="hip")
        with pytest.raises(ValueError, match="no CPU fallback"):
            GridDecoder(s, 10, table="device")
        with pytest.raises(ValueError, match="no CPU fallback"):
            s.decode(rows, "from-set", "grid", 10, backend="hip", table="device")
        with pytest.raises(ValueError, match="no CPU fallback"):
            s.clean_up(rows, "from-set", "grid", 10, encode_backend="hip-f64")


def test_encoder_cache_is_dropped_and_not_copied():
    s = HexagonalSSPSpace(2, ssp_dim=7, domain_bounds=B2, length_scale=0.2)

    class Handle:
        closed = False

        def close(self):
            self.closed = True

    h = Handle()
    s._encoder_cache = {("f64", 0): h}
    t = copy.deepcopy(s)
    assert "_encoder_cache" not in t.__dict__ and t.ssp_dim == s.ssp_dim
    s.update_lengthscale(0.3)
    assert h.closed and "_encoder_cache" not in s.__dict__


# -- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_prototypes_and_abi_errors_need_no_gpu(lib):
    for name in ("ssn_encoder_create", "ssn_encoder_destroy", "ssn_encoder_encode", "ssn_encoder_encode_device", "ssn_encoder_get_info",
                 "ssn_decoder_create_from_points"):
        assert name in _lib.EXPORTS and getattr(lib, name).argtypes == _lib.EXPORTS[name][1]
    assert b"ABI 11" in lib.ssn_version() and _lib.SSN_ABI_VERSION == 11
    assert C.sizeof(_lib.EncoderInfo) == 80
    K, M, w = ec.case_space("d97-2d").refine_tables()
    M, w = np.ascontiguousarray(M), np.ascontiguousarray(w)
    h = C.c_void_p()

    def create(dtype=1, d=97, K=K, dim=2, M=M.ctypes.data, w=w.ctypes.data, scratch=0, out=C.byref(h)):
        return lib.ssn_encoder_create(dtype, 0, d, K, dim, M, w, scratch, out)

    assert create(out=None) == -1 and b"null handle" in lib.ssn_last_error()
    assert create(M=None) == -1 and b"null argument" in lib.ssn_last_error()
    assert create(w=None) == -1 and b"null argument" in lib.ssn_last_error()
    assert create(dim=0) == -1 and b"dim 0 below 1" in lib.ssn_last_error()
    assert create(K=0) == -1 and b"K 0 outside" in lib.ssn_last_error()
    assert create(K=98) == -1 and b"K 98 outside" in lib.ssn_last_error()
    assert create(d=0) == -1 and b"d 0 outside 1 .. 2^20" in lib.ssn_last_error()
    assert create(d=2 ** 20 + 1, K=1) == -1 and b"outside 1 .. 2^20" in lib.ssn_last_error()
    assert create(dtype=7) == -1 and b"dtype" in lib.ssn_last_error()
    assert create(scratch=1000) == -1 and b"too small for one" in lib.ssn_last_error()
    assert not h.value
    x, out = np.zeros((4, 2)), np.zeros((4, 97))
    assert lib.ssn_encoder_encode(None, x.ctypes.data, 4, out.ctypes.data) == -1 and b"null encoder" in lib.ssn_last_error()
    assert lib.ssn_encoder_encode_device(None, x.ctypes.data, 0, 1, 2, 4, None, 97) == -1 and b"null encoder" in lib.ssn_last_error()
    assert lib.ssn_encoder_get_info(None, 4, None) == -1
    lib.ssn_encoder_destroy(None)                           # like free(NULL)
    pts = np.zeros((9, 2))

    def from_points(points=pts.ctypes.data, n=9, M=M.ctypes.data, w=w.ctypes.data, out=C.byref(h), width=97, scratch=0):
        return lib.ssn_decoder_create_from_points(0, 0, points, n, width, K, 2, M, w, scratch, 0, out)

    assert from_points(out=None) == -1 and b"null handle" in lib.ssn_last_error()
    assert from_points(points=None) == -1 and b"null argument" in lib.ssn_last_error()
    assert from_points(M=None) == -1 and b"null argument" in lib.ssn_last_error()
    assert from_points(n=0) == -1 and b"n_samples" in lib.ssn_last_error()
    assert from_points(width=0) == -1 and b"width" in lib.ssn_last_error()
    assert from_points(scratch=1000) == -1 and b"too small for one" in lib.ssn_last_error()
    if lib.ssn_device_count() == 0:
        assert create() == -2 and b"no CPU fallback" in lib.ssn_last_error()
        assert from_points() == -2 and b"no CPU fallback" in lib.ssn_last_error()
    assert not h.value
