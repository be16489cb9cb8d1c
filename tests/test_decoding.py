"""Grid decoder, the parts that need no GPU: the instrument of the GPU tests (tests/decoding_checks.py) accepts an exact f32 product
and rejects the mistakes a tiled argmax kernel can make; the C ABI and the Python surface fail loudly without a device; the NumPy
path of SSPSpace.decode is what it was."""
import ctypes as C
import os

import numpy as np
import pytest

import decoding_checks as dc
from sspslam_amd import _lib
from sspslam_amd.sspspace import HexagonalSSPSpace

B2 = np.tile([-1.0, 1.0], (2, 1))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.mark.parametrize("case", [(2, 97, 32, 4000), (3, 151, 20, 3000)])
def test_instrument_accepts_an_exact_f32_product(case):
    """The f32 product's indices equal the float64 ones on every row, and the winner's similarity, accumulated in float64 over the
    f32 operands as the decoder's finish kernel does, is within B / 2.  (The f32 chain's own value is not: a row against its own
    best sample is a sum of K same-sign products, and its f32 running sum was measured up to 1.9 x B / 2 off at d = 97 and
    2.75 x B / 2 at d = 201 on these inputs - why the decoder does not report it.)"""
    space, rows, table, _ = dc.standard_case(*case)
    assert space.ssp_dim == (97 if case[0] == 2 else 201) and table.shape[0] == case[2] ** case[0]
    ref = dc.standard_reference(*case)
    print(f"case {case}: smallest top-two gap {ref.gap.min():.3e}, largest bar {ref.bar.max():.3e}")
    assert ref.guard()
    idx, sims = dc.f32_stand_in(table, rows)
    chain = dc.f32_stand_in(table, rows, chain_sims=True)[1]
    t = np.arange(idx.shape[0])
    print(f"  similarity error / (B / 2): f64 over f32 operands {np.max(np.abs(sims - ref.sims[t, idx]) / (ref.bar / 2)):.3f}, "
          f"f32 chain {np.max(np.abs(chain - ref.sims[t, idx]) / (ref.bar / 2)):.3f}")
    assert ref.index_ok(idx).all() and ref.sims_ok(idx, sims).all()
    np.testing.assert_array_equal(idx, ref.jstar)           # the guard holds, so equality on every row
    assert ref.f64_ok(ref.jstar).all()
    np.testing.assert_array_equal(space.decode(rows, "from-set", "grid", case[2]), space.get_sample_points(case[2], "grid")[ref.jstar])


def test_instrument_rejects_mutated_answers():
    _, rows, table, _ = dc.standard_case(2, 97, 32, 4000)
    ref = dc.standard_reference(2, 97, 32, 4000)
    n = table.shape[0]
    # an index off by one tile width (128 columns, either way)
    assert not ref.index_ok((ref.jstar + 128) % n).any()
    assert not ref.index_ok((ref.jstar - 128) % n).any()
    # one row wrong among right ones is found
    one = ref.jstar.copy()
    one[1234] = (one[1234] + 128) % n
    ok = ref.index_ok(one)
    assert not ok[1234] and ok.sum() == ok.size - 1
    # a padded column winning: any index outside [0, n)
    for bad in (n, n + 127, -1, 2 ** 31 - 1):
        assert not ref.index_ok(np.full(ref.jstar.shape, bad)).any()
    # a similarity off by more than half the bar
    idx, sims = dc.f32_stand_in(table, rows)
    assert not ref.sims_ok(idx, sims + ref.bar).any() and not ref.sims_ok(idx, sims - ref.bar).any()
    # f64: a neighbouring column is no answer
    assert not ref.f64_ok((ref.jstar + 1) % n).any()


def test_instrument_rejects_the_highest_index_on_a_tie():
    rng = np.random.RandomState(5)
    table = rng.randn(300, 33)
    lo, hi = np.array([3, 40, 100]), np.array([77, 41, 299])
    table[hi] = table[lo]
    rows = table[lo] * 2.5
    ref = dc.Reference(table, rows)
    np.testing.assert_array_equal(ref.jstar, lo)
    assert ref.guard()                                      # the copy is no second candidate: the gap is to the next other row
    assert ref.index_ok(lo).all() and ref.f64_ok(lo).all()
    assert not ref.index_ok(hi).any() and not ref.f64_ok(hi).any()
    idx, _ = dc.f32_stand_in(table, rows)
    assert ref.index_ok(idx).all()


def test_scaling_matches_the_host_rule():
    rows = np.array([[0.0, 0.0, 0.0], [3e-10, 4e-10, 0.0], [3e-6, 4e-6, 0.0], [3.0, 4.0, 0.0]])
    u = dc.scale_rows(rows)
    np.testing.assert_array_equal(u[0], 0.0)
    np.testing.assert_array_equal(u[1], rows[1])            # norm 5e-10 < 1e-6: left as it is
    np.testing.assert_allclose(u[2:], [[0.6, 0.8, 0.0]] * 2, rtol=1e-15)


def test_abi_argument_errors_need_no_gpu(lib):
    table = np.ascontiguousarray(np.random.RandomState(0).randn(40, 9))
    h = C.c_void_p()

    def create(dtype=0, tab=table.ctypes.data, n=40, w=9, scratch=0, out=C.byref(h)):
        return lib.ssn_decoder_create(dtype, 0, tab, n, w, scratch, out)

    assert create(out=None) == -1 and b"null handle" in lib.ssn_last_error()
    assert create(tab=None) == -1 and b"null" in lib.ssn_last_error()
    assert create(w=0) == -1 and b"width" in lib.ssn_last_error()
    assert create(n=0) == -1 and b"n_samples" in lib.ssn_last_error()
    assert create(n=2 ** 31) == -1 and b"n_samples" in lib.ssn_last_error()
    assert create(dtype=7) == -1 and b"dtype" in lib.ssn_last_error()
    assert create(scratch=1000) == -1 and b"too small for one" in lib.ssn_last_error()
    assert not h.value
    best = np.zeros(4, dtype=np.int32)
    rows = np.zeros((4, 9))
    assert lib.ssn_decoder_rows(None, rows.ctypes.data, 4, best.ctypes.data, None) == -1 and b"null decoder" in lib.ssn_last_error()
    assert lib.ssn_decoder_rows_device(None, None, 0, 9, 4, best.ctypes.data, None) == -1 and b"null decoder" in lib.ssn_last_error()
    assert lib.ssn_decoder_get_info(None, 4, None) == -1
    assert lib.ssn_decoder_rows_composed(None, rows.ctypes.data, 4, best.ctypes.data) == -1
    lib.ssn_decoder_destroy(None)                           # like free(NULL)
    assert b"ABI 11" in lib.ssn_version() and _lib.SSN_ABI_VERSION == 11
    if lib.ssn_device_count() == 0:
        assert create() == -2 and b"no CPU fallback" in lib.ssn_last_error()       # SSN_EHIP, the wording of ssn_create
        assert not h.value


def test_griddecoder_raises_without_a_gpu(lib):
    from sspslam_amd.decoding import GridDecoder
    from sspslam_amd import harness as H
    with pytest.raises(ValueError, match="dtype"):
        GridDecoder(samples=(np.eye(3), np.eye(3)), dtype="bf16")
    with pytest.raises(ValueError, match="ssp_space or samples"):
        GridDecoder()
    if lib.ssn_device_count() == 0:
        space = H.make_ssp_space(2, ssp_dim=7)
        with pytest.raises(ValueError, match="no CPU fallback"):
            GridDecoder(space, 10)
        with pytest.raises(ValueError, match="no CPU fallback"):
            GridDecoder(samples=(np.eye(3), np.eye(3)))
        with pytest.raises(ValueError, match="no CPU fallback"):
            space.decode(np.ones((2, 7)), "from-set", "grid", 10, backend="hip")
        with pytest.raises(ValueError, match="no CPU fallback"):
            H.pathint_metrics(space, np.ones((2, 7)), np.ones((2, 7)), np.zeros((2, 2)), 10, backend="hip-f64")


def test_numpy_backend_is_unchanged_and_unknown_backends_are_refused(golden):
    g = golden("ssp_spaces.npz")
    s = HexagonalSSPSpace(2, ssp_dim=55, domain_bounds=B2, length_scale=0.2)
    rows = g["hex2_55_noisy"]
    for backend in (None, "numpy"):
        np.testing.assert_array_equal(s.decode(rows, "from-set", "grid", 100, backend=backend), g["hex2_55_decoded"])
        np.testing.assert_array_equal(s.decode(rows, "from-set", "grid", 31, backend=backend), g["hex2_55_decoded_31"])
    np.testing.assert_array_equal(s.clean_up(rows, "from-set", "grid", 31, backend=None), s.encode(g["hex2_55_decoded_31"]))
    samples = s.get_sample_pts_and_ssps(31)
    np.testing.assert_array_equal(s.decode(rows, samples=samples, backend=None), g["hex2_55_decoded_31"])
    for bad in ("cuda", "HIP", "", 3):
        with pytest.raises(ValueError, match="unknown decode backend"):
            s.decode(rows, "from-set", "grid", 31, backend=bad)
        with pytest.raises(ValueError, match="unknown decode backend"):
            s.clean_up(rows, "from-set", "grid", 31, backend=bad)
    with pytest.raises(NotImplementedError):                # other methods raise what they raised, whatever the backend
        s.decode(rows, "direct-optim", backend="hip")
    with pytest.raises(NotImplementedError):
        s.decode(rows, "network", backend="nonsense")


def test_space_with_a_decoder_cache_still_copies():
    import copy
    s = HexagonalSSPSpace(2, ssp_dim=7, domain_bounds=B2, length_scale=0.2)
    s._decoder_cache = {"key": object()}                    # stands for a live device handle
    t = copy.deepcopy(s)
    assert "_decoder_cache" not in t.__dict__ and t.ssp_dim == s.ssp_dim
    np.testing.assert_array_equal(t.phase_matrix, s.phase_matrix)
    del s._decoder_cache
