"""Grid decoder on the GPU (csrc/ssn_decode.hip behind decoding.GridDecoder), held to the instrument of tests/decoding_checks.py:
on inputs whose top-two gap exceeds the bar the device index must equal the float64 host index on EVERY row, f32 and f64 alike."""
import numpy as np
import pytest

import decoding_checks as dc
from helpers import small_pathint

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f64"]


@pytest.fixture(scope="module")
def GridDecoder():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from sspslam_amd.decoding import GridDecoder
    return GridDecoder


def check(ref, dtype, idx, sims):
    """Guard first, then equality on every row and the similarity bar."""
    assert ref.guard(), (ref.gap.min(), ref.bar.max())
    idx = np.asarray(idx)
    assert idx.dtype == np.int64 and idx.min() >= 0 and idx.max() < ref.n_samples
    bad = np.flatnonzero(idx != ref.jstar)
    assert bad.size == 0, (dtype, bad[:8], idx[bad[:8]], ref.jstar[bad[:8]])
    assert ref.index_ok(idx).all() and (dtype != "f64" or ref.f64_ok(idx).all())
    t = np.arange(idx.shape[0])
    worst = np.max(np.abs(sims - ref.sims[t, idx]) / np.maximum(ref.bar / 2, 1e-300))
    print(f"{dtype}: {idx.shape[0]} rows, smallest gap {ref.gap.min():.2e}, similarity error / (B / 2) at most {worst:.3f}")
    assert ref.sims_ok(idx, sims).all(), worst


# -- 1. standard inputs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [(2, 97, 32, 1), (2, 97, 32, 63), (2, 97, 32, 65), (2, 97, 32, 130), (3, 151, 20, 130)])
def test_standard_inputs(GridDecoder, case, dtype):
    space, rows, table, points = dc.standard_case(*case)
    ref = dc.standard_reference(*case)
    n = case[2]
    with GridDecoder(space, n, dtype=dtype) as dec:
        assert dec.n_samples == n ** case[0] and dec.width == space.ssp_dim == (97 if case[0] == 2 else 201)
        idx, sims = dec.indices(rows, return_sims=True)
        check(ref, dtype, idx, sims)
        np.testing.assert_array_equal(dec.indices(rows), idx)
        est, sims2 = dec.decode(rows, return_sims=True)
        np.testing.assert_array_equal(est, points[ref.jstar])
        np.testing.assert_array_equal(sims2, sims)
        np.testing.assert_array_equal(dec.decode(rows), est)
        np.testing.assert_array_equal(dec.clean_up(rows), space.encode(points[ref.jstar]))
        assert dec.info()["last_launches"] > 0
    host = space.decode(rows, "from-set", "grid", n)
    backend = "hip" if dtype == "f32" else "hip-f64"
    np.testing.assert_array_equal(space.decode(rows, "from-set", "grid", n, backend=backend), host)
    cached = space.__dict__["_decoder_cache"]
    np.testing.assert_array_equal(space.decode(rows, "from-set", "grid", n, backend=backend), host)
    assert space.__dict__["_decoder_cache"] is cached                  # the second call found the decoder of the first
    np.testing.assert_array_equal(space.clean_up(rows[:5], "from-set", "grid", n, backend=backend), space.encode(host[:5]))
    np.testing.assert_array_equal(space.decode(rows, samples=(table, points), backend=backend), host)
    space._drop_decoders()
    assert "_decoder_cache" not in space.__dict__ and next(iter(cached.values())).closed


# -- 2. ragged and tiny shapes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [1, 7, 97, 201])
@pytest.mark.parametrize("S", [1, 31, 100, 1027])
def test_ragged_shapes_through_samples(GridDecoder, S, K, dtype):
    rng = np.random.RandomState(1000 * S + K)
    table = rng.randn(S, K)
    points = rng.uniform(-1, 1, (S, 2))
    rows = rng.randn(70, K)
    ref = dc.Reference(table, rows)
    with GridDecoder(samples=(table, points), dtype=dtype) as dec:
        idx, sims = dec.indices(rows, return_sims=True)
        check(ref, dtype, idx, sims)
        np.testing.assert_array_equal(dec.decode(rows), points[ref.jstar])
        one = dec.indices(rows[3])                                    # a single 1-D row
        assert one.shape == (1,) and one[0] == ref.jstar[3]
        assert dec.indices(np.zeros((0, K))).shape == (0,)


# -- 3. seams ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_chunk_and_strip_seams_change_nothing(GridDecoder, dtype):
    case = (2, 97, 32, 130)
    space, rows, table, points = dc.standard_case(*case)
    ref = dc.standard_reference(*case)
    with GridDecoder(space, 32, dtype=dtype) as dec:
        base = dec.info(130)
        idx0, sims0 = dec.indices(rows, return_sims=True)
    check(ref, dtype, idx0, sims0)
    assert base["n_chunks"] == 1 and base["tile"] == 128 and base["scratch_bytes"] == 64 << 20
    smallest, slot = base["min_scratch_bytes"], base["slot_bytes"]
    seen = []
    for scratch in (smallest, smallest + 2 * slot):
        with GridDecoder(space, 32, dtype=dtype, scratch_bytes=scratch) as dec:
            info = dec.info(130)
            seen.append((info["n_chunks"], info["n_strips"], info["tiles_per_strip"]))
            idx, sims = dec.indices(rows, return_sims=True)
        np.testing.assert_array_equal(idx, idx0)
        assert sims.tobytes() == sims0.tobytes()                      # bit for bit
    assert seen[0] == (2, 1, 8), seen                                 # one row tile, one strip over all 8 column tiles
    assert seen[1][0] == 2 and seen[1][1] >= 3, seen                  # two row chunks, three column strips
    from sspslam_amd import frontend as fe
    with pytest.raises(fe.BuildError, match="too small for one"):
        GridDecoder(space, 32, dtype=dtype, scratch_bytes=smallest - 1)


# -- 4. exact ties ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_ties_go_to_the_lowest_column(GridDecoder, dtype):
    rng = np.random.RandomState(11)
    S, K = 1100, 33                                                   # 9 column tiles of 128
    table = rng.randn(S, K)
    # (i, j > i): same 32-column block, same tile across the two waves, different tiles of a strip, different strips
    lo = np.array([10, 5, 130, 200, 640])
    hi = np.array([20, 100, 300, 900, 1099])
    table[hi] = table[lo]
    points = np.arange(S, dtype=np.float64)[:, None]
    rows = np.repeat(table[lo], 3, axis=0) * np.array([1.0, 0.37, 41.0] * len(lo))[:, None]
    want = np.repeat(lo, 3)
    ref = dc.Reference(table, rows)
    np.testing.assert_array_equal(ref.jstar, want)
    with GridDecoder(samples=(table, points), dtype=dtype) as dec:
        base = dec.info(len(rows))
        idx0, sims0 = dec.indices(rows, return_sims=True)
    check(ref, dtype, idx0, sims0)
    np.testing.assert_array_equal(idx0, want)
    plans = [(base["n_strips"], base["tiles_per_strip"])]
    for extra in (0, 2):                                              # one strip of 9 tiles; three strips of 3 tiles
        with GridDecoder(samples=(table, points), dtype=dtype, scratch_bytes=base["min_scratch_bytes"] + extra * base["slot_bytes"]) as dec:
            info = dec.info(len(rows))
            plans.append((info["n_strips"], info["tiles_per_strip"]))
            idx, sims = dec.indices(rows, return_sims=True)
        np.testing.assert_array_equal(idx, want)
        assert sims.tobytes() == sims0.tobytes()
    assert plans[1] == (1, 9) and plans[2] == (3, 3), plans            # (130, 300) share strip 0, (200, 900) and (640, 1099) do not
    assert plans[0][1] < 3, plans                                     # default: more strips than that - 130 and 300 are apart


# -- 5. padding must not win ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_padded_columns_never_win(GridDecoder, dtype):
    rng = np.random.RandomState(12)
    S, K = 100, 33                                                    # no multiple of any tile; 28 padded columns of zeros
    table = rng.uniform(0.1, 1.0, (S, K))
    rows = -rng.uniform(0.1, 1.0, (70, K))
    ref = dc.Reference(table, rows)
    assert (ref.sims < 0).all()                                       # a padded column's similarity, 0, would beat them all
    with GridDecoder(samples=(table, np.arange(S)[:, None]), dtype=dtype) as dec:
        idx, sims = dec.indices(rows, return_sims=True)
    assert idx.max() < S and (sims < 0).all()
    check(ref, dtype, idx, sims)


# -- 6. degenerate rows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_degenerate_rows(GridDecoder, dtype):
    space, rows, table, points = dc.standard_case(2, 97, 32, 63)
    unit = dc.scale_rows(rows[:20])
    with GridDecoder(space, 32, dtype=dtype) as dec:
        idx, sims = dec.indices(np.zeros((3, 97)), return_sims=True)
        np.testing.assert_array_equal(idx, 0)                         # every similarity is 0: the lowest column
        np.testing.assert_array_equal(sims, 0.0)
        # norm 1e-9 < 1e-6: not normalised, on the device as on the host
        tiny = unit * 1e-9
        ref = dc.Reference(table, tiny)
        idx, sims = dec.indices(tiny, return_sims=True)
        check(ref, dtype, idx, sims)
        assert np.all(np.abs(sims) < 2e-9)
        np.testing.assert_array_equal(dec.decode(tiny), space.decode(tiny, "from-set", "grid", 32))
        # a row scaled by 1e6 decodes like its unit version
        iu, su = dec.indices(unit, return_sims=True)
        ib, sb = dec.indices(unit * 1e6, return_sims=True)
        check(dc.Reference(table, unit), dtype, iu, su)
        check(dc.Reference(table, unit * 1e6), dtype, ib, sb)
        np.testing.assert_array_equal(ib, iu)
        np.testing.assert_allclose(sb, su, rtol=0, atol=1e-6)


# -- 7. device input --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tdtype", ["float32", "float64"])
def test_device_tensors_with_a_leading_dimension(GridDecoder, dtype, tdtype):
    import torch
    space, rows, table, points = dc.standard_case(2, 97, 32, 130)
    host_rows = rows.astype(tdtype).astype(np.float64)               # what the tensor holds
    wide = torch.full((130, 97 + 13), float("nan"), dtype=getattr(torch, tdtype), device="cuda:0")
    wide[:, :97] = torch.from_numpy(host_rows).to(wide.dtype)
    view = wide[:, :97]
    assert view.stride(0) == 110 and not view.is_contiguous()
    with GridDecoder(space, 32, dtype=dtype, scratch_bytes=None) as dec:
        want_i, want_s = dec.indices(host_rows, return_sims=True)
        got_i, got_s = dec.indices(view, return_sims=True)
        np.testing.assert_array_equal(got_i, want_i)
        assert got_s.tobytes() == want_s.tobytes()
        np.testing.assert_array_equal(dec.decode(view), points[want_i])
        np.testing.assert_array_equal(dec.indices(view.contiguous()), want_i)
        np.testing.assert_array_equal(dec.indices(view[7]), want_i[7:8])
        np.testing.assert_array_equal(dec.indices(torch.from_numpy(host_rows)), want_i)     # a CPU tensor is a host array
    check(dc.Reference(table, host_rows), dtype, got_i, got_s)


# -- 8. isolation -----------------------------------------------------------------------------------------------------------
def test_a_decoder_leaves_a_running_simulator_alone(GridDecoder):
    from sspslam_amd.builder import build
    from sspslam_amd.simulator import Simulator
    pm = small_pathint(ssp_dim=7, n=64)
    model = build(pm.model)
    space, rows, _, _ = dc.standard_case(2, 97, 32, 63)
    outs = []
    for with_decoder in (False, True):
        dec = GridDecoder(space, 32) if with_decoder else None       # a decoder may precede the simulator ...
        with Simulator(None, model=model, dtype="f32") as sim:
            sim.run_steps(60)
            if with_decoder:
                dec.indices(rows)
                dec.close()
                with GridDecoder(space, 32, dtype="f64") as other:     # ... or come and go while it exists
                    other.indices(rows)
            sim.run_steps(60)
            outs.append(np.array(sim.data[pm.probe]))
    assert outs[0].shape == (120, 7)
    np.testing.assert_array_equal(outs[1], outs[0])


# -- 9. the harness ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["hip", "hip-f64"])
def test_pathint_metrics_backend(GridDecoder, backend):
    from sspslam_amd import harness as H
    from sspslam_amd.builder import build
    from sspslam_amd.simulator import Simulator
    pm = small_pathint(ssp_dim=7, n=64)
    with Simulator(None, model=build(pm.model), dtype="f32") as sim:
        sim.run_steps(200)
        out = np.array(sim.data[pm.probe])
    want = H.pathint_metrics(pm.ssp_space, out, pm.real_ssp, pm.path)
    got = H.pathint_metrics(pm.ssp_space, out, pm.real_ssp, pm.path, backend=backend)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    pm.ssp_space._drop_decoders()


def test_example_script_decodes_on_the_gpu(GridDecoder, capsys):
    """examples/run_pathint.py --decode-backend hip: the same result line, the decode on the GPU and timed next to the run."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("run_pathint_example", os.path.join(root, "examples", "run_pathint.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = {}
    for backend in ("numpy", "hip"):
        out = mod.main(["--ssp-dim", "7", "--pi-n-neurons", "64", "--T", "2.0", "--limit", "0.5", "--decode-backend", backend])
        assert out.shape == (2000, 7)
        lines[backend] = capsys.readouterr().out.strip().splitlines()[-1]
        assert ("s (%s); similarity" % backend) in lines[backend] and ", decode " in lines[backend]
    assert lines["hip"].split("similarity")[1] == lines["numpy"].split("similarity")[1]      # same similarity, same final error
