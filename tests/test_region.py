"""Region SSPs without a GPU: the instrument of tests/region_checks.py (its references agree with themselves, its stand-ins pass under
half their bars, every wrong encoder fails, C comes from the stand-in), the NumPy ``SSPSpace.encode_region`` against both references,
the argument errors, ``normalize`` and ``harness.region_ssps``."""
import ctypes as C

import numpy as np
import pytest

import encode_checks as ec
import region_checks as rg
from sspslam_amd import _lib
from sspslam_amd import harness as H
from sspslam_amd.sspspace import HexagonalSSPSpace

B2 = np.array([[-1.0, 1.0], [-1.0, 1.0]])


def package(ref):
    return ref.space.encode_region(ref.boxes, samples=ref.samples, mean=ref.mode == "mean")


# -- the instrument -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.CASES)
def test_references_and_stand_ins(name):
    space = ec.case_space(name)
    boxes = rg.case_boxes(name)
    span = space.domain_bounds[:, 1] - space.domain_bounds[:, 0]
    L = boxes[:, :, 1] - boxes[:, :, 0]
    assert boxes.shape == (130, space.domain_dim, 2) and np.all(boxes[:, :, 0] >= space.domain_bounds[:, 0]) and np.all(boxes[:, :, 1] <= space.domain_bounds[:, 1])
    assert L.min() < 2e-3 * span.max() and np.all(L[0] == span) and np.all(L >= 0.99e-3 * span)
    for mode, samples in rg.variants(space):
        ref = rg.reference(name, mode, samples)
        if mode != "mesh":                                           # the rule is converged: twice the nodes move it by under 1/8 of the bar
            moved = ref.check(rg.gl_reference(space, boxes, mode == "mean", split=2), "f64", label=f"{name} Gauss-Legendre, nodes doubled", limit=0.125)
            assert moved <= 0.125
        ref.check(rg.f64_stand_in(space, boxes, mode, samples), "f64", label=f"stand-in {name}", limit=0.5)
        ref.check(rg.f32_stand_in(space, boxes, mode, samples), "f32", label=f"stand-in {name}", limit=0.5)
        ref.check(package(ref), "f64", label=f"SSPSpace.encode_region {name}")
        for n in rg.NS:                                              # a prefix is held to the same bars
            assert ref.ratio(space.encode_region(boxes[:n], samples=samples, mean=mode == "mean"), "f64", slice(0, n)).max() <= 1.0


def test_special_and_far_boxes():
    labels = list(rg.special_boxes())
    assert len(labels) == 15
    for label in labels:
        ref = rg.special_reference(label)
        ref.check(rg.f64_stand_in(ref.space, ref.boxes, ref.mode, ref.samples), "f64", label=f"stand-in, {label}:", limit=0.5)
        ref.check(rg.f32_stand_in(ref.space, ref.boxes, ref.mode, ref.samples), "f32", label=f"stand-in, {label}:", limit=0.5)
        ref.check(package(ref), "f64", label=f"SSPSpace.encode_region, {label}:")
    # the pi boxes are where they claim to be: y of the chosen bin on axis 0 is pi to a few ulp, and 1e-9 to either side
    _, M, _ = ec.case_space("d97-2d").refine_tables()
    for n in (2, 3):
        boxes = rg.special_boxes()[f"y = pi and pi +- 1e-9, n = {n}"][0]
        y = abs(M[rg.PI_BIN, 0]) * (boxes[:, 0, 1] - boxes[:, 0, 0]) / (2 * (n - 1))
        np.testing.assert_allclose(y - np.pi, [0.0, 1e-9, -1e-9], atol=1e-14)
    # a zero-width box: its mean is the point encode of its centre, its integral zero
    zero = rg.special_boxes()["zero width, mean"][0]
    space = ec.case_space("d97-2d")
    np.testing.assert_allclose(space.encode_region(zero[1:], mean=True), space.encode(zero[1:, :, 0]), atol=1e-15)
    assert not np.any(space.encode_region(zero))
    far = ec.case_space(ec.FAR)
    _, M, _ = far.refine_tables()
    assert np.abs(rg.far_boxes()).max() == 50.0 and np.abs(rg.far_boxes()[:, :, 0] @ M.T).max() > 900
    for mode, samples in rg.variants(far):
        ref = rg.far_reference(mode, samples)
        ref.check(rg.f64_stand_in(far, ref.boxes, mode, samples), "f64", label="stand-in, far:", limit=0.5)
        ref.check(rg.f32_stand_in(far, ref.boxes, mode, samples), "f32", label="stand-in, far:", limit=0.5)
        ref.check(package(ref), "f64", label="SSPSpace.encode_region, far:")
        live = ref.V > 0
        plain = np.abs(package(ref) - ref.want)[live] / (ref.bar("f64") - ref.phase)[live]
        print(f"far {mode} {samples}: without the phase term the NumPy closed form sits at {plain.max():.2f} of the f64 bar")


def test_c_comes_from_the_stand_in():
    c0, per = rg.measure_c0()
    print("worst |error| / (REL Sbar_c) of the f32 stand-in:", {k: round(v, 3) for k, v in per.items()}, "c0 =", round(c0, 4))
    assert 0.9 * rg.C0 <= c0 <= rg.C0 and rg.C == 2 * rg.C0 and rg.REL == ec.REL


@pytest.mark.parametrize("fault", list(rg.MUTANTS))
def test_wrong_encoders_fail(fault):
    """Each fails the f64 bar by a factor of 100 at least, and the f32 bar too - but for two that the f32 bar cannot see: the amplitude
    computed in f32 (an f32 encoder rounds A cos th to f32 in any case) and the missing guard at y = pi (1e-9 from pi the unguarded
    ratio of one bin is off by 1e-6 of itself, less than the f32 rounding of the K bins together)."""
    mode, samples = rg.MUTANTS[fault]
    if mode == "pi":
        refs = [rg.special_reference(f"y = pi and pi +- 1e-9, n = {samples}")]
    elif fault == "no guard at y = 0":                              # bin 0 of a symmetric space, and a zero-width axis for any bin
        refs = [rg.reference("d97-2d", mode), rg.reference("d201-3d", mode), rg.special_reference("zero width, mean")]
    else:
        refs = [rg.reference(case, mode, rg.counts_for(ec.case_space(case))[-1] if samples == 20 else samples) for case in ("d97-2d", "d201-3d", "d64-full")]
    for ref in refs:
        rows = slice(0, min(16, len(ref.boxes)))
        got = rg.f64_stand_in(ref.space, ref.boxes[rows], ref.mode, ref.samples, fault)
        for dtype in ("f64", "f32"):
            worst = ref.ratio(got, dtype, rows).max()
            if dtype == "f32" and fault in ("amplitude in f32", "no guard at y = pi"):
                assert worst < 1.0
                continue
            assert worst > 100.0, (fault, ref.mode, dtype, worst)
            with pytest.raises(AssertionError):
                ref.check(got, dtype, rows)
        np.testing.assert_array_less(ref.ratio(rg.f64_stand_in(ref.space, ref.boxes[rows], ref.mode, ref.samples), "f64", rows), 0.5)


# -- the Python layer -----------------------------------------------------------------------------------------------------------
def test_argument_errors_and_normalize():
    s = H.make_ssp_space(2, ssp_dim=7)
    box = np.array([[-0.5, 0.25], [0.0, 0.5]])
    assert s.encode_region(box).shape == (1, 7) and s.encode_region(box[None], samples=[2, 5]).shape == (1, 7)
    with pytest.raises(ValueError, match="mean given together with samples"):
        s.encode_region(box, samples=20, mean=True)
    for bad in (1, 0, [20, 1]):
        with pytest.raises(ValueError, match="below 2"):
            s.encode_region(box, samples=bad)
    for bad in ([20, 20, 20], 2.5):
        with pytest.raises(ValueError, match="samples must be"):
            s.encode_region(box, samples=bad)
    with pytest.raises(ValueError, match=r"boxes must be \(N, 2, 2\)"):
        s.encode_region(np.zeros((3, 3, 2)))
    with pytest.raises(ValueError, match="box 1 has hi < lo"):
        s.encode_region(np.stack([box, box[:, ::-1]]))
    with pytest.raises(ValueError, match="unknown encode backend"):
        s.encode_region(box, backend="cuda")
    # normalize: SSPSpace.normalize's rule, row by row; a zero row stays zero
    boxes = np.stack([box, 0.5 * box, np.array([[0.1, 0.1], [0.2, 0.2]])])
    raw, unit = s.encode_region(boxes), s.encode_region(boxes, normalize=True)
    assert not np.any(raw[2]) and not np.any(unit[2])
    for i in range(2):
        assert unit[i].tobytes() == s.normalize(raw[i]).tobytes()
    mesh = s.encode_region(boxes, samples=20, normalize=True)
    np.testing.assert_allclose(np.linalg.norm(mesh, axis=1), 1.0, atol=1e-15)
    lib = _lib.load()
    if lib.ssn_device_count() == 0:
        from sspslam_amd import SSPEncoder
        with pytest.raises(ValueError, match="no CPU fallback"):
            s.encode_region(box, backend="hip")
        with pytest.raises(ValueError, match="no CPU fallback"):
            SSPEncoder(s)


def test_prototypes_and_abi_errors_need_no_gpu():
    lib = _lib.load()
    for name in ("ssn_encoder_encode_boxes", "ssn_encoder_encode_boxes_device"):
        assert name in _lib.EXPORTS and getattr(lib, name).argtypes == _lib.EXPORTS[name][1]
    assert b"ABI 11" in lib.ssn_version() and _lib.SSN_ABI_VERSION == 11 and C.sizeof(_lib.EncoderInfo) == 80
    x, out = np.zeros((4, 4)), np.zeros((4, 97))
    assert lib.ssn_encoder_encode_boxes(None, x.ctypes.data, 4, None, 0, out.ctypes.data) == -1 and b"ssn_encoder_encode_boxes: null encoder" in lib.ssn_last_error()
    assert lib.ssn_encoder_encode_boxes_device(None, x.ctypes.data, 0, 1, 4, 4, None, 0, 0, None, 97) == -1 and b"boxes_device: null encoder" in lib.ssn_last_error()


# -- the harness ----------------------------------------------------------------------------------------------------------------
def test_region_ssps_against_a_midpoint_rule():
    """``wall_ssps`` of slam_map_new.py:73-80: the script integrates every entry with dblquad at epsabs=1e-4; a 200 x 200 midpoint rule
    stands in for it here."""
    s = HexagonalSSPSpace(2, ssp_dim=55, domain_bounds=B2, length_scale=0.2)
    walls = np.array([[[-1.1, -0.95], [0.2, 1.1]], [[-0.95, -0.0], [0.95, 1.1]]])          # its wall_boundaries
    want = np.empty((2, s.ssp_dim))
    for j, w in enumerate(walls):
        axes = [w[a, 0] + (np.arange(200) + 0.5) * (w[a, 1] - w[a, 0]) / 200 for a in range(2)]
        mid = s.encode(np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 2)).mean(axis=0) * np.prod(w[:, 1] - w[:, 0])
        np.testing.assert_allclose(s.encode_region(w)[0], mid, atol=1e-4)                    # the integral itself, at the script's epsabs
        want[j] = s.normalize(mid)
    got = H.region_ssps(s, walls)
    assert got.shape == (2, s.ssp_dim)
    np.testing.assert_allclose(got, want, atol=1e-3)
    np.testing.assert_allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-15)
