"""'grid-refine' on the GPU (k_decode_refine of csrc/ssn_decode.hip behind decoding.GridDecoder.refine), held to the instrument of
tests/refine_checks.py: every guarded row within B_x of the instrument's own float64 maximiser, f32 and f64 alike.

Worst |x - x*| / B_x measured on the MI355X (printed by every test): see the table there."""
import numpy as np
import pytest

import decoding_checks as dc
import refine_checks as rc

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f64"]
STANDARD = [(1, 63, 100, 70), (2, 97, 32, 1), (2, 97, 32, 65), (2, 97, 32, 130), (3, 151, 20, 130)]
EXPLICIT = [("sym", 1, 3, 32, 70, 0.05), ("sym", 2, 97, 32, 70, 0.5), ("sym", 2, 127, 32, 70, 0.5), ("sym", 2, 129, 32, 70, 0.5),
            ("sym", 2, 1027, 32, 70, 0.5), ("full", 2, 97, 32, 70, 0.5), ("full", 2, 64, 32, 70, 0.5)]


@pytest.fixture(scope="module")
def GridDecoder():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from sspslam_amd.decoding import GridDecoder
    return GridDecoder


def same_bits(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


# -- 1. standard inputs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STANDARD)
def test_standard_inputs(GridDecoder, case, dtype):
    space, rows, table, points = dc.standard_case(*case)
    ref = rc.standard_reference(*case)
    n = case[2]
    with GridDecoder(space, n, dtype=dtype) as dec:
        before = dec.info(len(rows))
        x, f, status, best = dec.refine(rows, return_info=True)
        assert x.dtype == np.float64 and x.shape == (case[3], case[0]) and best.dtype == np.int64
        np.testing.assert_array_equal(best, ref.best)
        ref.check(x, status, dtype, f"device {case}")
        assert np.all(np.abs(f - ref.f(x)) <= ref.bar_fx(dtype, x)), np.max(np.abs(f - ref.f(x)) / ref.bar_fx(dtype, x))
        if dtype == "f64":
            assert not np.any(status[ref.guarded] & 6)                       # converged, at a maximum
        assert not np.any(status[ref.guarded] & 2)
        np.testing.assert_array_equal(dec.refine(rows), x)
        np.testing.assert_array_equal(dec.decode(rows, refine=True), x)
        # iterations = 0 is the grid decode, exactly; the plain decode and the plan are what they were
        np.testing.assert_array_equal(dec.refine(rows, iterations=0), points[ref.best])
        np.testing.assert_array_equal(dec.decode(rows), points[ref.best])
        after = dec.info(len(rows))
        assert {k: v for k, v in after.items() if not k.startswith("last_")} == {k: v for k, v in before.items() if not k.startswith("last_")}


# -- 2. bin counts: K = 2, 49, 64, 65, one above the register cap, the full spectrum ---------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", EXPLICIT)
def test_bin_count_edges(GridDecoder, case, dtype):
    space, rows, path, ref = rc.explicit_case(*case)
    n = case[3]
    with GridDecoder(space, n, dtype=dtype) as dec:
        x, f, status, best = dec.refine(rows, return_info=True)
    np.testing.assert_array_equal(best, ref.best)
    ref.check(x, status, dtype, f"device {case}")
    assert np.all(np.abs(f - ref.f(x)) <= ref.bar_fx(dtype, x)), np.max(np.abs(f - ref.f(x)) / ref.bar_fx(dtype, x))


# -- 3. noise-free rows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim,ssp_dim,n", [(1, 63, 100), (2, 97, 32), (3, 151, 20)])
def test_noise_free_rows(GridDecoder, dim, ssp_dim, n, dtype):
    space, _, table, points = dc.standard_case(dim, ssp_dim, n, 130)
    rng = np.random.RandomState(4)
    y = np.concatenate([rng.uniform(-0.9, 0.9, (20, dim)), points[rng.randint(0, len(points), 5)], points[[0, -1]]])
    rows = space.encode(y)
    ref = rc.reference_for(space, rows, n)
    with GridDecoder(space, n, dtype=dtype) as dec:
        x, f, status, _ = dec.refine(rows, return_info=True)
    r = ref.ratio(x, dtype, at=y)
    print(f"noise-free {dim}-D {dtype}: worst |x - y| / B_x = {r.max():.3f}, B_x at most {ref.bar_x(dtype, at=y).max():.2e}")
    assert (r <= 1.0).all() and ref.in_box(x).all()
    assert not (status & 2).any()


# -- 4. bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_chunks_device_rows_and_repeats_change_no_bit(GridDecoder, dtype):
    import torch
    space, rows, _, _ = dc.standard_case(2, 97, 32, 130)
    rows = np.concatenate([rows, rows[:85] * 1.7, rows[40:125] * 0.3])       # 300 rows
    with GridDecoder(space, 32, dtype=dtype) as dec:
        base = dec.info(300)
        want = dec.refine(rows, return_info=True)
        assert same_bits(dec.refine(rows, return_info=True), want)           # two calls
        for tdtype in ("float32", "float64"):
            host = rows.astype(tdtype).astype(np.float64)                     # what the tensor holds
            wide = torch.full((300, 97 + 13), float("nan"), dtype=getattr(torch, tdtype), device="cuda:0")
            wide[:, :97] = torch.from_numpy(host).to(wide.dtype)
            view = wide[:, :97]
            assert view.stride(0) == 110 and not view.is_contiguous()
            assert same_bits(dec.refine(view, return_info=True), dec.refine(host, return_info=True))
    assert base["n_chunks"] == 1
    with GridDecoder(space, 32, dtype=dtype, scratch_bytes=base["min_scratch_bytes"]) as dec:
        assert dec.info(300)["n_chunks"] == 3                                # one 128-row tile at a time
        assert same_bits(dec.refine(rows, return_info=True), want)
        assert same_bits(dec.refine(rows[:130], return_info=True), [a[:130] for a in want])


# -- 5. degenerate rows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_degenerate_rows(GridDecoder, dtype):
    space, rows, table, points = dc.standard_case(2, 97, 32, 65)
    with GridDecoder(space, 32, dtype=dtype) as dec:
        x, f, status, best = dec.refine(np.zeros((3, 97)), return_info=True)
        np.testing.assert_array_equal(best, 0)
        np.testing.assert_array_equal(x, np.tile(points[0], (3, 1)))          # x0 itself
        np.testing.assert_array_equal(f, 0.0)
        assert (status & 2).all()
        tiny = dc.scale_rows(rows[:20]) * 1e-9                                # norm below 1e-6: not normalised, as decode treats it
        ref = rc.reference_for(space, tiny, 32)
        xt, ft, st, bt = dec.refine(tiny, return_info=True)
        np.testing.assert_array_equal(bt, ref.best)
        assert ref.in_box(xt).all() and np.all(np.abs(ft) < 2e-9) and np.all((st >= 0) & (st < 8))
        one = dec.refine(rows[3])                                             # a single 1-D row
        assert one.shape == (1, 2)
        np.testing.assert_array_equal(one, dec.refine(rows)[3:4])
        x0, f0, s0, b0 = dec.refine(np.zeros((0, 97)), return_info=True)
        assert x0.shape == (0, 2) and f0.shape == s0.shape == b0.shape == (0,)


# -- 6. ties -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_either_neighbour_of_a_tie_refines_to_the_same_point(GridDecoder, dtype):
    """Rows that encode the midpoint of two neighbouring grid points: whichever of the two the grid decode starts from (the table
    without the other one, through samples= and trust=), the refined points agree."""
    space, _, table, points = dc.standard_case(2, 97, 32, 65)
    n, pitch = 32, 2.0 / 31
    rng = np.random.RandomState(6)
    a = rng.randint(0, n * n - 1, 40)
    a = a[(a % n) != n - 1]                                                   # a and a + 1 are neighbours along one axis (C order)
    a = a[np.all(np.abs(points[a]) < 1, axis=1) & np.all(np.abs(points[a + 1]) < 1, axis=1)]      # and off the domain's edge
    assert a.size >= 20
    assert np.allclose(np.linalg.norm(points[a + 1] - points[a], axis=1), pitch)
    mid = 0.5 * (points[a] + points[a + 1])
    rows = space.encode(mid)
    xs = []
    for drop in (a + 1, a):
        keep = np.ones(n * n, dtype=bool)
        keep[drop] = False
        with GridDecoder(space, samples=(table[keep], points[keep]), dtype=dtype, trust=pitch) as dec:
            x, f, status, best = dec.refine(rows, return_info=True)
        xs.append(x)
        assert not (status & 3).any()
    ref = rc.reference_for(space, rows, n)
    bx = ref.bar_x(dtype, at=mid)
    starts = np.linalg.norm(points[a] - points[a + 1], axis=1)
    gap = np.linalg.norm(xs[0] - xs[1], axis=1)
    print(f"ties {dtype}: starts {starts.min():.3f} apart, refined points at most {np.max(gap / bx):.3f} B_x apart, "
          f"{max(np.max(np.linalg.norm(x - mid, axis=1) / bx) for x in xs):.3f} B_x from the midpoint")
    assert (gap <= 2 * bx).all()
    assert all((np.linalg.norm(x - mid, axis=1) <= bx).all() for x in xs)
    with pytest.raises(ValueError, match="trust"):
        with GridDecoder(space, samples=(table, points), dtype=dtype) as dec:
            dec.refine(rows)


# -- 7. best effort on a grid too coarse for the basin assumption -------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_coarse_grid_is_best_effort(GridDecoder, dtype):
    """8 samples per axis over [-1, 1] at length scale 0.2: the pitch exceeds the basin of the maximum, so no accuracy is claimed -
    the points are finite and inside the box, and the status words say what happened."""
    space, rows, _, _ = dc.standard_case(2, 97, 32, 130)
    ref = rc.reference_for(space, rows, 8)
    with GridDecoder(space, 8, dtype=dtype) as dec:
        x, f, status, best = dec.refine(rows, return_info=True)
    np.testing.assert_array_equal(best, ref.best)
    assert ref.in_box(x).all() and np.all(np.isfinite(f)) and np.all((status >= 0) & (status < 8))
    face = (status & 1) != 0
    assert ref.on_face(x)[face].all()
    print(f"coarse grid {dtype}: status counts {np.bincount(status, minlength=8).tolist()}")


# -- 8. the C ABI ------------------------------------------------------------------------------------------------------------
def test_abi_errors(GridDecoder):
    from sspslam_amd import _lib
    lib = _lib.load()
    space, rows, _, _ = dc.standard_case(2, 97, 32, 65)
    rows = np.ascontiguousarray(rows)
    x = np.zeros((65, 2))
    with GridDecoder(space, 32) as dec:
        h, p = dec._h, x.ctypes.data
        assert lib.ssn_decoder_refine_rows(h, rows.ctypes.data, 65, 8, p, None, None, None) == -1
        assert b"ssn_decoder_set_refine first" in lib.ssn_last_error()
        assert lib.ssn_decoder_refine_rows_device(h, None, 0, 97, 0, 8, p, None, None, None) == -1
        assert lib.ssn_decoder_set_refine(h, p, 49, p, p, 4, p, p, p, p) == -1 and b"dim 4" in lib.ssn_last_error()
        assert lib.ssn_decoder_set_refine(h, p, 49, None, p, 2, p, p, p, p) == -1 and b"null argument" in lib.ssn_last_error()
        assert lib.ssn_decoder_set_refine(h, p, 98, p, p, 2, p, p, p, p) == -1 and b"bins" in lib.ssn_last_error()
        want = dec.refine(rows)                                               # uploads the tables
        assert lib.ssn_decoder_refine_rows(h, rows.ctypes.data, 0, 8, None, None, None, None) == 0        # n_rows == 0 succeeds
        assert lib.ssn_decoder_refine_rows(h, None, 65, 8, p, None, None, None) == -1 and b"null argument" in lib.ssn_last_error()
        assert lib.ssn_decoder_refine_rows(h, rows.ctypes.data, 65, -1, p, None, None, None) == -1 and b"iterations" in lib.ssn_last_error()
        assert lib.ssn_decoder_refine_rows_device(h, None, 7, 97, 4, 8, p, None, None, None) == -1 and b"rows_dtype" in lib.ssn_last_error()
        assert lib.ssn_decoder_refine_rows_device(h, None, 0, 96, 4, 8, p, None, None, None) == -1 and b"leading dimension" in lib.ssn_last_error()
        assert lib.ssn_decoder_refine_rows(h, rows.ctypes.data, 65, 8, p, None, None, None) == 0          # best, f, status may be NULL
        np.testing.assert_array_equal(x, want)


# -- 9. the public calls -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["hip", "hip-f64"])
def test_public_calls(GridDecoder, backend):
    from sspslam_amd import harness as H
    case = (2, 97, 32, 130)
    space, rows, table, points = dc.standard_case(*case)
    ref = rc.standard_reference(*case)
    dtype = "f32" if backend == "hip" else "f64"
    path = np.random.RandomState(1).uniform(-0.9, 0.9, (130, 2))              # the points standard_case encoded
    x = space.decode(rows, "grid-refine", "grid", 32, backend=backend)
    assert ref.position_ok(x, dtype).all() and ref.in_box(x).all()
    cached = space.__dict__["_decoder_cache"]
    np.testing.assert_array_equal(space.decode(rows, "from-set", "grid", 32, backend=backend), points[ref.best])
    assert space.__dict__["_decoder_cache"] is cached                        # one decoder serves both methods
    np.testing.assert_array_equal(space.decode(rows, "grid-refine", "grid", 32, backend=backend, iterations=0), points[ref.best])
    xi, f, status, best = space.decode(rows, "grid-refine", "grid", 32, backend=backend, return_info=True)
    np.testing.assert_array_equal(xi, x)
    np.testing.assert_array_equal(space.decode(rows, "grid-refine", samples=(table, points), trust=2.0 / 31, backend=backend), x)
    np.testing.assert_array_equal(space.clean_up(rows[:5], "grid-refine", "grid", 32, backend=backend), space.encode(x[:5]))
    real = space.encode(path)
    est, sims, err = H.pathint_metrics(space, rows, real, path, 32, backend=backend)
    est_r, sims_r, err_r = H.pathint_metrics(space, rows, real, path, 32, backend=backend, refine=True)
    np.testing.assert_array_equal(est_r, x)
    np.testing.assert_array_equal(sims_r, sims)
    print(f"{backend}: median position error, grid {np.median(err):.4f}, refined {np.median(err_r):.4f}")
    assert np.median(err_r) < np.median(err)
    space._drop_decoders()
