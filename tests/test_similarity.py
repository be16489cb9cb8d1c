"""Similarity maps without a GPU: the NumPy paths against the reference's expressions written out, the instrument of
tests/map_checks.py on its own CPU stand-in (which yields the factors ``C`` of the f32 bar), the argument errors, and wrong devices
that the bars have to catch."""
import numpy as np
import pytest

import map_checks as mc
from sspslam_amd import harness as H

CASES = list(mc.C)


# -- 1. the NumPy paths are the reference's expressions ---------------------------------------------------------------------
def test_path_maps_are_the_reference_sim_grid():
    space, rows, table, _ = mc.case("s144")
    n = 12
    rows = rows[:40]
    sim_grid = (table.reshape(n, n, -1) @ rows.T) ** 2                 # run_pathint_gif.py:231-232
    out = H.similarity_frames(space, rows, n)
    assert out.shape == (40, n, n) and out.dtype == np.float64
    np.testing.assert_allclose(np.moveaxis(out, 0, -1), sim_grid, rtol=1e-15, atol=1e-15 * np.abs(sim_grid).max())
    flat = space.similarity_map(rows, n)                               # SSPSpace.similarity_plot: the unsquared product
    np.testing.assert_array_equal(flat, rows @ table.T)
    np.testing.assert_array_equal(space.similarity_map(rows, n, power=2), (rows @ table.T) ** 2)
    np.testing.assert_array_equal(space.similarity_map(rows, samples=(table, None)), flat)
    np.testing.assert_array_equal(space.similarity_map(rows[3], n), flat[3:4])
    assert space.similarity_map(np.zeros((0, table.shape[1])), n).shape == (0, n * n)


def test_frame_maps_are_the_reference_q_sims():
    space, rows, table, _ = mc.case("cube")
    n = 6
    frames = np.array(rows[3:15]).reshape(3, 4, -1)                     # MapProbe frames: (samples, L, d), no degenerate row
    out = H.similarity_frames(space, frames, n, normalize=True)
    assert out.shape == (3, 4, n, n, n)
    for s in range(3):
        for l in range(4):
            q = frames[s, l] / np.linalg.norm(frames[s, l])              # run_slam_map_gif.py:366-368
            q_sims = ((table @ q) ** 2).reshape(n, n, n)
            np.testing.assert_allclose(out[s, l], q_sims, rtol=1e-15, atol=1e-15 * q_sims.max())
    # the documented quirk: a landmark not yet seen recalls a near-zero row; it stays as it is, its map is ~0 and not NaN
    frames[1, 2] = 1e-9 * frames[0, 0]
    frames[2, 3] = 0.0
    out = H.similarity_frames(space, frames, n, normalize=True)
    assert np.isfinite(out).all() and out[1, 2].max() < 1e-15 and not out[2, 3].any()
    assert H.similarity_frames(space, frames[:0], n).shape == (0, 4, n, n, n)


@pytest.mark.parametrize("normalize", [False, True])
def test_similarity_map_scales_rows_as_decode_does(normalize):
    space, rows, table, _ = mc.case("s400")
    ref = mc.MapReference(table, rows, normalize, mc.C["s400"])
    for power in (1, 2):
        got = space.similarity_map(rows, 20, power=power, normalize=normalize)
        assert ref.ok(got, "f64", power).all(), ref.worst(got, "f64", power)
    if normalize:
        np.testing.assert_array_equal(np.argmax(space.similarity_map(rows, 20, normalize=True), axis=1),
                                      space._best_samples(rows, table)[1])


# -- 2. the stand-in passes the bars and yields c ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_stand_in_passes_the_bars_and_yields_c(name):
    _, rows, table, _ = mc.case(name)
    K = table.shape[1]
    ratios = []
    for normalize in (False, True):
        ref = mc.MapReference(table, rows, normalize, mc.C[name])
        chain = mc.f32_chain(table, rows, normalize)
        ratios.append(ref.chain_ratio(chain))
        assert ref.ok(chain, "f32").all() and ref.ok(chain, "f32", cap=True).all()
        sq = mc.f32_chain(table, rows, normalize, power=2)
        assert sq.tobytes() == (chain * chain).tobytes()
        assert ref.ok(sq, "f32", 2).all()
        print(f"{name} normalize={normalize}: chain at {ratios[-1]:.3f} REL A, its square at {ref.worst(sq, 'f32', 2):.2f} of the power-2 bar")
        assert ref.worst(sq, "f32", 2) <= 0.75
        # float64 NumPy against the f64 bar, and the f64 bar is far below the f32 one
        assert ref.ok(mc.scaled(rows, normalize) @ table.T, "f64").all()
        assert np.all(ref.bar("f64") <= ref.bar("f32") * 1e-6)
    c = 2 * max(ratios)
    print(f"{name}: K = {K}, c = 2 x {max(ratios):.3f} = {c:.3f}, map_checks.C holds {mc.C[name]}, hard cap {(K + 8) * 2.0 ** -24 / mc.REL:.1f} REL A")
    assert c <= mc.C[name] <= 1.1 * c + 0.1                            # C is twice the worst ratio, rounded up - not a loose number
    assert mc.C[name] * mc.REL <= (K + 8) * 2.0 ** -24
    assert max(ratios) > 1 or name in ("t1", "w7")                     # REL bare does not hold for a k-ordered chain


def test_bar_factor_must_stay_below_the_cap():
    _, rows, table, _ = mc.case("w7")
    with pytest.raises(AssertionError):
        mc.MapReference(table, rows, False, 4.0)                       # 4 REL > (7 + 8) 2^-24


# -- 3. argument errors -----------------------------------------------------------------------------------------------------
def test_argument_errors():
    space, rows, table, _ = mc.case("s144")
    for power in (0, 3, 1.5, True, None):
        with pytest.raises(ValueError, match="power must be 1 or 2"):
            space.similarity_map(rows, 12, power=power)
        with pytest.raises(ValueError, match="power must be 1 or 2"):
            H.similarity_frames(space, rows, 12, power=power)
    with pytest.raises(ValueError, match="unknown decode backend"):
        space.similarity_map(rows, 12, backend="cuda")
    with pytest.raises(ValueError, match="needs a hip backend"):
        space.similarity_map(rows, 12, table="device")
    with pytest.raises(ValueError, match="table must be"):
        space.similarity_map(rows, 12, table="gpu")
    with pytest.raises(ValueError, match=r"ssp must be \(T, 97\)"):
        space.similarity_map(rows[:, :50], 12)
    with pytest.raises(ValueError, match="sampling_method must be 'grid'"):
        H.similarity_frames(space, rows, 12, sampling_method="length-scale")
    with pytest.raises(ValueError, match=r"rows must be \(T, d\) or frames"):
        H.similarity_frames(space, rows[0], 12)
    with pytest.raises(ValueError, match=r"rows must be \(T, d\) or frames"):
        H.similarity_frames(space, np.zeros((2, 2, 2, 97)), 12)


# -- 4. wrong devices fail ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def s144():
    _, rows, table, _ = mc.case("s144")
    refs = {nz: mc.MapReference(table, rows, nz, mc.C["s144"]) for nz in (False, True)}
    chains = {nz: mc.f32_chain(table, rows, nz) for nz in (False, True)}
    return rows, table, refs, chains


def test_wrong_columns_shifted_by_one(s144):
    _, _, refs, chains = s144
    assert not refs[True].ok(np.roll(chains[True], 1, axis=1), "f32").all()
    assert not refs[True].ok(chains[True][:, 1:], "f32").any()          # a wrong shape fails everywhere


def test_wrong_last_k_slab_dropped(s144):
    rows, table, refs, _ = s144
    assert table.shape[1] == 97                                        # slabs of 32: the fourth holds k = 96 alone
    short = mc.f32_chain(table, rows, True, slabs=3)
    assert not refs[True].ok(short, "f32").all()
    _, rows_k, table_k, _ = mc.case("fullk")
    ref = mc.MapReference(table_k, rows_k, True, mc.C["fullk"])
    assert not ref.ok(mc.f32_chain(table_k, rows_k, True, slabs=31), "f32").all()


def test_wrong_row_scaling(s144):
    _, _, refs, chains = s144
    assert not refs[False].ok(chains[True], "f32").all()               # scaled when it should be raw
    assert not refs[True].ok(chains[False], "f32").all()               # raw when it should be scaled
    # the rows below 1e-6 are the same either way: only a device that scales them too is wrong there
    rows, table, _, _ = s144
    tiny = np.array(chains[True])
    tiny[2] = mc.f32_chain(table, rows[2:3] / np.linalg.norm(rows[2]), False)[0]
    assert refs[True].ok(chains[True], "f32")[2].all() and not refs[True].ok(tiny, "f32")[2].all()


def test_wrong_square_missing(s144):
    _, _, refs, chains = s144
    for nz in (False, True):
        assert refs[nz].ok(chains[nz] * chains[nz], "f32", 2).all()
        assert not refs[nz].ok(chains[nz], "f32", 2).all()
        assert not refs[nz].ok(chains[nz] * chains[nz], "f32", 1).all()


def test_wrong_last_ragged_row_tile_left_at_its_sentinel(s144):
    _, _, refs, chains = s144
    for sentinel in (np.nan, 0.0, -7.0):
        left = np.array(chains[True])
        left[256:] = sentinel                                          # 257 rows: the third row tile holds one
        ok = refs[True].ok(left, "f32")
        assert ok[:256].all() and not ok[256].any()


def test_wrong_padded_column_written(s144):
    _, _, _, chains = s144
    T, S = chains[True].shape
    parent = np.full((T + 3, S + 16), -7.0, dtype=np.float32)
    parent[:T, :S] = chains[True]
    assert mc.padding_ok(parent, T, S, -7.0)
    for r, c in ((0, S), (T - 1, S + 15), (T, 0), (T + 2, S - 1)):
        bad = parent.copy()
        bad[r, c] = 0.0                                                # what a padded table column or a padded row computes
        assert not mc.padding_ok(bad, T, S, -7.0)


def test_wrong_operands_rounded_to_ten_bits(s144):
    rows, table, refs, _ = s144
    for nz in (False, True):
        half = mc.f32_chain(table, rows, nz, mantissa=10)
        assert not refs[nz].ok(half, "f32").all()
        bad = np.mean(~refs[nz].ok(half, "f32"))
        print(f"normalize={nz}: {bad:.2f} of the entries of a 10-bit-operand device miss the bar, {np.mean(~refs[nz].ok(half, 'f32', cap=True)):.2f} the cap")
        assert bad > 0.5


def test_wrong_grid_axes_transposed():
    space, rows, table, _ = mc.case("s144")
    n = 12
    rows = rows[:16]
    ref = mc.MapReference(table, rows, False, mc.C["s144"])
    good = H.similarity_frames(space, rows, n, power=1)
    assert ref.ok(good.reshape(16, -1), "f64").all()
    swapped = np.swapaxes(good, 1, 2)
    assert not ref.ok(swapped.reshape(16, -1), "f32").all()
    # and in 3-D, any two of the axes
    space3, rows3, table3, _ = mc.case("cube")
    ref3 = mc.MapReference(table3, rows3[:8], False, mc.C["cube"])
    good3 = H.similarity_frames(space3, rows3[:8], 6, power=1)
    assert ref3.ok(good3.reshape(8, -1), "f64").all()
    for a, b in ((1, 2), (1, 3), (2, 3)):
        assert not ref3.ok(np.swapaxes(good3, a, b).reshape(8, -1), "f32").all()
