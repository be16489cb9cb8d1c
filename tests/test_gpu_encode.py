"""SSP encoding on the GPU (csrc/ssn_encode.hip behind encoding.SSPEncoder, SSPSpace.encode(backend=...), GridDecoder(table="device") and
clean_up(encode="device")), held to the instrument of tests/encode_checks.py: every entry of every row under its bar, f32 and f64.

Worst |error| / bar measured on the MI355X (printed by every test): DESIGN.md 3.14."""
import ctypes as C

import numpy as np
import pytest

import decoding_checks as dc
import encode_checks as ec
import refine_checks as rc

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f64"]
SMALL = [c for c in ec.CASES if c != "d1015-2d"]


@pytest.fixture(scope="module")
def SSPEncoder():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from sspslam_amd import SSPEncoder
    return SSPEncoder


def bits(a):
    return np.ascontiguousarray(a).tobytes()


# -- 1. every entry under its bar: N = 1, 63, 64, 65, 130 over every K seam -----------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", SMALL)
def test_entries_under_the_bar(SSPEncoder, case, dtype):
    ref = ec.reference(case)
    with SSPEncoder(ref.space, dtype=dtype) as enc:
        info = enc.info(130)
        assert info["padded_2k"] == -(-2 * ref.K // 32) * 32 and info["n_chunks"] == 1 and info["tile"] == 64
        full = None
        for n in ec.NS:
            got = enc.encode(ref.x[:n])
            assert got.dtype == np.float64 and got.shape == (n, ref.space.ssp_dim)
            ref.check(got, dtype, slice(0, n), label=f"device {case} N={n}")
            full = got
        for n in ec.NS[:-1]:                                        # a row's bits do not depend on how many rows come with it
            assert bits(enc.encode(ref.x[:n])) == bits(full[:n])
        assert enc.info()["last_launches"] >= 2 and enc.info()["last_kernel_ms"] > 0
        assert enc.encode(np.zeros((0, ref.space.domain_dim))).shape == (0, ref.space.ssp_dim)
        one = enc.encode(ref.x[3])                                  # a single 1-D point
        assert one.shape == (1, ref.space.ssp_dim) and bits(one) == bits(full[3:4])
        sp = ec.special_reference(case)
        sp.check(enc.encode(sp.x), "f64" if dtype == "f64" else "f32-format", label=f"device {case} special points")


@pytest.mark.parametrize("dtype", DTYPES)
def test_d1015_once(SSPEncoder, dtype):
    ref = ec.reference("d1015-2d")
    with SSPEncoder(ref.space, dtype=dtype) as enc:
        assert enc.info()["padded_2k"] == 1024
        ref.check(enc.encode(ref.x), dtype, label="device d1015-2d N=130")
        sp = ec.special_reference("d1015-2d")
        sp.check(enc.encode(sp.x), "f64" if dtype == "f64" else "f32-format", label="device d1015-2d special points")


# -- 2. the far case: |th| near 1000 rad ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_far_points(SSPEncoder, dtype):
    ref = ec.reference(ec.FAR)
    with SSPEncoder(ref.space, dtype=dtype) as enc:
        ref.check(enc.encode(ref.x), dtype, label="device far", phases=dtype == "f64")


# -- 3. inputs, outputs and the scratch size change no bit ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_inputs_outputs_and_chunks_change_no_bit(SSPEncoder, dtype):
    import torch
    ref = ec.reference("d97-2d")
    tdt = torch.float32 if dtype == "f32" else torch.float64
    with SSPEncoder(ref.space, dtype=dtype) as enc:
        base = enc.info(130)
        want = enc.encode(ref.x)
        assert bits(enc.encode(ref.x)) == bits(want)                                  # two calls
        dev = enc.encode(ref.x, out="device")
        assert dev.dtype == tdt and dev.is_cuda and tuple(dev.shape) == (130, 97)
        assert bits(dev.cpu().double().numpy()) == bits(want)
        for pdt in ("float32", "float64"):
            host = ref.x.astype(pdt)                                                 # what the tensor holds
            want_p = enc.encode(host.astype(np.float64))
            assert bits(enc.encode(host)) == bits(want_p)                            # f32 host points are read as they are
            wide = torch.full((130, 2 + 5), float("nan"), dtype=getattr(torch, pdt), device="cuda:0")
            wide[:, :2] = torch.from_numpy(host)
            view = wide[:, :2]
            assert view.stride(0) == 7 and not view.is_contiguous()
            assert bits(enc.encode(view)) == bits(want_p)
            out = enc.encode(view, out="device")
            assert out.dtype == tdt and bits(out.cpu().double().numpy()) == bits(want_p)
            ec.Reference(ref.space, host.astype(np.float64)).check(want_p, dtype, label=f"device d97-2d {pdt} points")
    assert base["n_chunks"] == 1
    with SSPEncoder(ref.space, dtype=dtype, scratch_bytes=base["min_scratch_bytes"]) as enc:
        assert enc.info(130)["n_chunks"] == 3 and enc.info(130)["row_chunk"] == 64    # one 64-point tile at a time
        assert bits(enc.encode(ref.x)) == bits(want)
        assert bits(enc.encode(ref.x, out="device").cpu().double().numpy()) == bits(want)
        assert bits(enc.encode(ref.x[:65])) == bits(want[:65])
    from sspslam_amd import frontend as fe
    with pytest.raises(fe.BuildError, match="too small for one"):
        SSPEncoder(ref.space, dtype=dtype, scratch_bytes=base["min_scratch_bytes"] - 1)


# -- 4. a decoder whose table is made on the device -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [(2, 97, 32, 130), (3, 151, 20, 130)])
def test_device_table_decoder(SSPEncoder, case, dtype):
    from sspslam_amd.decoding import GridDecoder
    space, rows, table, points = dc.standard_case(*case)
    ref = dc.standard_reference(*case)
    n = case[2]
    calls = []
    orig = space.get_sample_pts_and_ssps
    space.get_sample_pts_and_ssps = lambda *a, **k: calls.append(a) or orig(*a, **k)
    try:
        with GridDecoder(space, n, dtype=dtype, table="device") as dec:
            assert not calls and dec.table_source == "device" and dec.n_samples == n ** case[0] and dec.width == space.ssp_dim
            np.testing.assert_array_equal(dec.sample_points, points)
            idx, sims = dec.indices(rows, return_sims=True)
            info = dec.info(len(rows))
    finally:
        del space.get_sample_pts_and_ssps
    with GridDecoder(space, n, dtype=dtype) as host_dec:
        hidx, hsims = host_dec.indices(rows, return_sims=True)
        hinfo = host_dec.info(len(rows))
    # the existing instrument, exactly as the host-table decoder is held to it
    assert ref.guard(), (ref.gap.min(), ref.bar.max())
    assert idx.dtype == np.int64 and ref.index_ok(idx).all() and (dtype != "f64" or ref.f64_ok(idx).all())
    assert ref.sims_ok(idx, sims).all()
    assert ref.index_ok(hidx).all() and ref.sims_ok(hidx, hsims).all()
    clear = ref.gap > ref.bar
    assert clear.all()
    np.testing.assert_array_equal(idx[clear], hidx[clear])
    np.testing.assert_array_equal(idx[clear], ref.jstar[clear])
    print(f"device table {case} {dtype}: similarities at most {np.max(np.abs(sims - hsims)):.2e} from the host-table decoder's")
    assert {k: v for k, v in info.items() if not k.startswith("last_")} == {k: v for k, v in hinfo.items() if not k.startswith("last_")}


@pytest.mark.parametrize("dtype", DTYPES)
def test_refine_on_a_device_table_decoder(SSPEncoder, dtype):
    from sspslam_amd.decoding import GridDecoder
    case = (2, 97, 32, 130)
    space, rows, table, points = dc.standard_case(*case)
    ref = rc.standard_reference(*case)
    with GridDecoder(space, 32, dtype=dtype, table="device") as dec:
        x, f, status, best = dec.refine(rows, return_info=True)
        np.testing.assert_array_equal(best, ref.best)
        ref.check(x, status, dtype, f"device table {case}")
        assert np.all(np.abs(f - ref.f(x)) <= ref.bar_fx(dtype, x))
        np.testing.assert_array_equal(dec.refine(rows, iterations=0), points[ref.best])


# -- 5. clean_up with the encode on the device --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("refine", [False, True])
def test_clean_up_encodes_on_the_device(SSPEncoder, dtype, refine):
    import torch
    from sspslam_amd.decoding import GridDecoder
    space, rows, table, points = dc.standard_case(2, 97, 32, 130)
    with GridDecoder(space, 32, dtype=dtype) as dec:
        pts = dec.decode(rows, refine=refine)
        got = dec.clean_up(rows, refine=refine, encode="device")
        ref = ec.Reference(space, pts)
        assert got.dtype == np.float64
        ref.check(got, dtype, label=f"clean_up refine={refine}")
        dev = dec.clean_up(rows, refine=refine, encode="hip", out="device")
        assert dev.is_cuda and dev.dtype == (torch.float32 if dtype == "f32" else torch.float64)
        assert bits(dev.cpu().double().numpy()) == bits(got)
        np.testing.assert_array_equal(dec.clean_up(rows, refine=refine), space.encode(pts))          # the default is the host encode
        with pytest.raises(ValueError, match="encode must be"):
            dec.clean_up(rows, encode="gpu")
        with pytest.raises(ValueError, match="needs encode='device'"):
            dec.clean_up(rows, out="device")


# -- 6. the public calls --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["hip", "hip-f64"])
def test_public_calls(SSPEncoder, backend):
    from sspslam_amd import harness as H
    dtype = "f32" if backend == "hip" else "f64"
    case = (2, 97, 32, 130)
    space, rows, table, points = dc.standard_case(*case)
    dref = dc.standard_reference(*case)
    path = np.random.RandomState(1).uniform(-0.9, 0.9, (130, 2))
    ref = ec.Reference(space, path)
    got = space.encode(path, backend=backend)
    ref.check(got, dtype, label=f"SSPSpace.encode backend={backend}")
    cache = space.__dict__["_encoder_cache"]
    assert bits(space.encode(path, backend=backend)) == bits(got) and space.__dict__["_encoder_cache"] is cache and len(cache) == 1
    assert bits(space.encode(path)) == bits(ref.want)                                   # the default is untouched
    est = space.decode(rows, "from-set", "grid", 32, backend=backend, table="device")
    np.testing.assert_array_equal(est, points[dref.jstar])
    key = next(iter(space.__dict__["_decoder_cache"]))
    assert key[-1] == "device" and space.__dict__["_decoder_cache"][key].table_source == "device"
    space.decode(rows, "from-set", "grid", 32, backend=backend)
    assert next(iter(space.__dict__["_decoder_cache"])) == (32, "grid", dtype)          # the host-table decoder is another key
    cu = space.clean_up(rows, "from-set", "grid", 32, backend=backend, encode_backend=backend, table="device")
    ec.Reference(space, points[dref.jstar]).check(cu, dtype, label=f"SSPSpace.clean_up encode_backend={backend}")
    real = space.encode(path)
    a = H.pathint_metrics(space, rows, real, path, 32, backend=backend, table="device")
    b = H.pathint_metrics(space, rows, real, path, 32, backend=backend)
    assert all(bits(u) == bits(v) for u, v in zip(a, b))
    frames = rows[:120].reshape(12, 10, 97)
    np.testing.assert_array_equal(H.map_over_time(space, frames, 32, backend=backend, table="device"), H.map_over_time(space, frames, 32, backend=backend))
    enc = next(iter(cache.values()))
    space._drop_decoders()                                                              # drops both caches
    assert enc.closed and "_encoder_cache" not in space.__dict__ and "_decoder_cache" not in space.__dict__


# -- 7. the C ABI with a live handle ----------------------------------------------------------------------------------------------
def test_abi_errors(SSPEncoder):
    import torch
    from sspslam_amd import _lib
    lib = _lib.load()
    ref = ec.reference("d97-2d")
    x = np.ascontiguousarray(ref.x[:4])
    out = torch.zeros((4, 97), dtype=torch.float64, device="cuda:0")
    with SSPEncoder(ref.space) as enc:
        h = enc._h
        assert lib.ssn_encoder_encode_device(h, x.ctypes.data, 0, 1, 1, 4, out.data_ptr(), 97) == -1 and b"below dim" in lib.ssn_last_error()
        assert lib.ssn_encoder_encode_device(h, x.ctypes.data, 0, 1, 2, 4, out.data_ptr(), 96) == -1 and b"below the width" in lib.ssn_last_error()
        assert lib.ssn_encoder_encode_device(h, x.ctypes.data, 0, 7, 2, 4, out.data_ptr(), 97) == -1 and b"points_dtype" in lib.ssn_last_error()
        assert lib.ssn_encoder_encode_device(h, None, 0, 1, 2, 4, out.data_ptr(), 97) == -1 and b"null argument" in lib.ssn_last_error()
        assert lib.ssn_encoder_encode_device(h, x.ctypes.data, 0, 1, 2, 4, None, 97) == -1 and b"null argument" in lib.ssn_last_error()
        assert lib.ssn_encoder_encode_device(h, None, 0, 1, 2, 0, None, 97) == 0                          # n == 0 succeeds
        assert lib.ssn_encoder_encode(h, None, 4, None) == -1 and b"null argument" in lib.ssn_last_error()
        assert lib.ssn_encoder_encode(h, x.ctypes.data, -1, None) == -1 and b"negative" in lib.ssn_last_error()
        assert lib.ssn_encoder_get_info(h, 4, None) == -1
        assert lib.ssn_encoder_encode_device(h, x.ctypes.data, 0, 1, 2, 4, out.data_ptr(), 97) == 0
        assert bits(out.cpu().numpy()) == bits(enc.encode(x))
        info = enc.info(10 ** 6)
        assert info["n_chunks"] == -(-10 ** 6 // info["row_chunk"]) and info["row_chunk"] % 64 == 0
        enc.close()
        from sspslam_amd import frontend as fe
        with pytest.raises(fe.SimulationError, match="closed"):
            enc.encode(x)


# -- 8. the example script's flags ------------------------------------------------------------------------------------------------
def test_example_script_flags(SSPEncoder, capsys):
    """examples/run_pathint.py --decode-table / --encode-backend: one more line with the encode and decoder-creation seconds, the
    same result; without the flags the output is what it was."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("run_pathint_example", os.path.join(root, "examples", "run_pathint.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = ["--ssp-dim", "7", "--pi-n-neurons", "64", "--T", "2.0", "--limit", "0.5", "--decode-backend", "hip"]
    mod.main(base)
    plain = capsys.readouterr().out.strip().splitlines()
    assert not any("decoder creation" in line for line in plain)
    mod.main(base + ["--decode-table", "device", "--encode-backend", "hip"])
    lines = capsys.readouterr().out.strip().splitlines()
    extra = [line for line in lines if "decoder creation" in line]
    assert len(extra) == 1 and "(hip); decoder creation" in extra[0] and "(table: device)" in extra[0] and len(lines) == len(plain) + 1
    assert lines[-1].split("final position error")[1] == plain[-1].split("final position error")[1]
    with pytest.raises(SystemExit, match="needs --decode-backend hip"):
        mod.main(base[:-1] + ["numpy", "--decode-table", "device"])
