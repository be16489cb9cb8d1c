"""Region SSPs on the GPU (k_encode_phase_box / k_encode_rownorm of csrc/ssn_encode.hip behind SSPEncoder.encode_region,
SSPSpace.encode_region(backend=...) and harness.area_query), held to the instrument of tests/region_checks.py: every entry of every box
under its bar, f32 and f64, in the three amplitude modes.

Worst |error| / bar measured on the MI355X (printed by every test): DESIGN.md 3.16."""
import numpy as np
import pytest

import encode_checks as ec
import recall_checks as rc
import region_checks as rg

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f64"]


@pytest.fixture(scope="module")
def SSPEncoder():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from sspslam_amd import SSPEncoder
    return SSPEncoder


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def region(enc, ref, boxes=None, **kw):
    return enc.encode_region(ref.boxes if boxes is None else boxes, samples=ref.samples, mean=ref.mode == "mean", **kw)


# -- 1. every entry under its bar: every case, dtype and mode at N = 130 --------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ec.CASES)
def test_entries_under_the_bar(SSPEncoder, case, dtype):
    space = ec.case_space(case)
    with SSPEncoder(space, dtype=dtype) as enc:
        for mode, samples in rg.variants(space):
            ref = rg.reference(case, mode, samples)
            got = region(enc, ref)
            assert got.dtype == np.float64 and got.shape == (130, space.ssp_dim)
            ref.check(got, dtype, label=f"device {case} N=130")
            assert enc.info()["last_launches"] >= 2 and enc.info()["last_kernel_ms"] > 0
        assert enc.encode_region(np.zeros((0, space.domain_dim, 2))).shape == (0, space.ssp_dim)


# -- 2. N = 1, 63, 64, 65: a row's bits do not depend on how many rows come with it ---------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_counts(SSPEncoder, dtype):
    space = ec.case_space("d97-2d")
    with SSPEncoder(space, dtype=dtype) as enc:
        for mode, samples in (("integral", None), ("mean", None), ("mesh", 20)):
            ref = rg.reference("d97-2d", mode, samples)
            full = region(enc, ref)
            for n in rg.NS:
                got = region(enc, ref, ref.boxes[:n])
                ref.check(got, dtype, slice(0, n), label=f"device d97-2d N={n}")
                assert bits(got) == bits(full[:n])
            one = region(enc, ref, ref.boxes[3])                      # a single (dim, 2) box
            assert one.shape == (1, 97) and bits(one) == bits(full[3:4])


# -- 3. inputs, outputs and the scratch size change no bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_inputs_outputs_and_chunks_change_no_bit(SSPEncoder, dtype):
    import torch
    from sspslam_amd import frontend as fe
    space = ec.case_space("d97-2d")
    tdt = torch.float32 if dtype == "f32" else torch.float64
    ref = rg.reference("d97-2d", "mesh", 20)
    with SSPEncoder(space, dtype=dtype) as enc:
        point_info = enc.info(130)
        smallest = enc.region_min_scratch
        assert smallest == point_info["min_scratch_bytes"] + 64 * 8 * 2
        want = region(enc, ref)
        per_chunk = enc.info()["last_launches"]
        assert bits(region(enc, ref)) == bits(want)                                    # two calls
        dev = region(enc, ref, out="device")
        assert dev.dtype == tdt and dev.is_cuda and tuple(dev.shape) == (130, 97) and bits(dev.cpu().double().numpy()) == bits(want)
        for bdt in ("float32", "float64"):
            host = ref.boxes.astype(bdt)                                                # what the tensor holds
            want_b = region(enc, ref, host.astype(np.float64))
            assert bits(region(enc, ref, host)) == bits(want_b)                         # f32 host boxes are read as they are
            wide = torch.full((130, 4 + 5), float("nan"), dtype=getattr(torch, bdt), device="cuda:0")
            wide[:, :4] = torch.from_numpy(host.reshape(130, 4))
            view = wide[:, :4].unflatten(1, (2, 2))
            assert tuple(view.shape) == (130, 2, 2) and view.stride(0) == 9 and not view.is_contiguous()
            assert bits(region(enc, ref, view)) == bits(want_b)
            out = region(enc, ref, view, out="device")
            assert out.dtype == tdt and bits(out.cpu().double().numpy()) == bits(want_b)
            rg.Reference(space, host.astype(np.float64), "mesh", 20).check(want_b, dtype, label=f"device d97-2d {bdt} boxes")
        # out="device" of the C ABI into a strided buffer: nothing outside [:N, :d] is touched
        lib = enc._lib
        buf = torch.full((133, 97 + 7), float("nan"), dtype=tdt, device="cuda:0")
        flat = np.ascontiguousarray(ref.boxes.reshape(130, 4))
        counts = np.array([20, 20], dtype=np.int32)
        torch.cuda.synchronize()
        assert lib.ssn_encoder_encode_boxes_device(enc._h, flat.ctypes.data, 0, 1, 4, 130, counts.ctypes.data, 0, 0, buf.data_ptr(), 104) == 0
        got = buf.cpu().double().numpy()
        assert bits(got[:130, :97]) == bits(want) and np.isnan(got[130:]).all() and np.isnan(got[:, 97:]).all()
    # three chunks at the smallest accepted scratch: the same bits as one chunk
    with SSPEncoder(space, dtype=dtype, scratch_bytes=smallest) as enc:
        assert bits(region(enc, ref)) == bits(want) and enc.info()["last_launches"] == 3 * per_chunk
        assert bits(region(enc, ref, out="device").cpu().double().numpy()) == bits(want)
        assert bits(region(enc, ref, ref.boxes[:65])) == bits(want[:65]) and enc.info()["last_launches"] == 2 * per_chunk
    with SSPEncoder(space, dtype=dtype, scratch_bytes=smallest - 1) as enc:            # enough for points, not for boxes
        assert enc.encode(ec.case_points("d97-2d")[:3]).shape == (3, 97)
        with pytest.raises(fe.SimulationError, match=f"too small for one 64-box tile.*{smallest} bytes"):
            region(enc, ref)


# -- 4. the point path is where it was, and a zero-width mean is the point encode -------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_width_mean_is_the_point_encode(SSPEncoder, dtype):
    for case in ("d97-2d", "d201-3d", ec.FAR):
        space = ec.case_space(case)
        x = ec.case_points(case)[:65]
        with SSPEncoder(space, dtype=dtype) as enc:
            got = enc.encode_region(np.stack([x, x], axis=2), mean=True)
            assert bits(got) == bits(enc.encode(x))
            assert not np.any(enc.encode_region(np.stack([x, x], axis=2)))           # and its integral is zero


# -- 5. normalize on the device against the host rule -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_normalize_on_the_device(SSPEncoder, dtype):
    from sspslam_amd.encoding import unit_rows
    space = ec.case_space("d201-3d")                                  # d = 201: three full strides of the wave and a ragged one
    ref = rg.reference("d201-3d", "integral")
    boxes = ref.boxes.copy()
    boxes[5, 1, 1] = boxes[5, 1, 0]                                   # a zero-volume box: its row is zero and stays zero
    u = 2.0 ** -24 if dtype == "f32" else 2.0 ** -53
    with SSPEncoder(space, dtype=dtype) as enc:
        raw = enc.encode_region(boxes, out="device").cpu().double().numpy()
        dev = enc.encode_region(boxes, normalize=True, out="device")
        got = dev.cpu().double().numpy()
        want = unit_rows(raw)
        # the sum of squares (d terms, another order), the square root, the division and the rounding of the result
        err = np.abs(got - want)
        assert np.all(err <= (space.ssp_dim / 2 + 4) * u * np.abs(want)), float(np.max(err / np.maximum(np.abs(want), 1e-300)))
        assert not np.any(got[5]) and np.allclose(np.linalg.norm(np.delete(got, 5, axis=0), axis=1), 1.0, atol=8 * u)
        assert bits(enc.encode_region(boxes, normalize=True, out="device").cpu().double().numpy()) == bits(got)
        host = enc.encode_region(boxes, normalize=True)                # the host result is normalised on the host
        assert bits(host) == bits(unit_rows(raw))
        for i in (0, 7):
            assert bits(host[i]) == bits(space.normalize(raw[i]))
        assert bits(enc.encode_region(boxes, out="device").cpu().double().numpy()) == bits(raw)


# -- 6. the special boxes and the far space --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_special_and_far_boxes(SSPEncoder, dtype):
    with SSPEncoder(ec.case_space("d97-2d"), dtype=dtype) as enc:
        for label in rg.special_boxes():
            ref = rg.special_reference(label)
            ref.check(region(enc, ref), dtype, label=f"device, {label}:")
    with SSPEncoder(ec.case_space(ec.FAR), dtype=dtype) as enc:
        for mode, samples in rg.variants(ec.case_space(ec.FAR)):
            ref = rg.far_reference(mode, samples)
            ref.check(region(enc, ref), dtype, label="device, far:")


# -- 7. the refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(SSPEncoder):
    import torch
    from sspslam_amd import frontend as fe
    space = ec.case_space("d97-2d")
    boxes = rg.case_boxes("d97-2d")[:4].copy()
    flat = np.ascontiguousarray(boxes.reshape(4, 4))
    out = torch.zeros((4, 97), dtype=torch.float64, device="cuda:0")
    host_out = np.zeros((4, 97))
    two, one = np.array([2, 2], dtype=np.int32), np.array([20, 1], dtype=np.int32)
    with SSPEncoder(space) as enc:
        lib, h = enc._lib, enc._h
        dev = lambda **k: lib.ssn_encoder_encode_boxes_device(h, k.get("boxes", flat.ctypes.data), 0, k.get("dtype", 1), k.get("ld", 4), k.get("n", 4),      # noqa: E731
                                                              k.get("samples"), k.get("mean", 0), 0, k.get("out", out.data_ptr()), k.get("out_ld", 97))
        assert dev(ld=3) == -1 and b"below 2 dim = 4" in lib.ssn_last_error()
        assert dev(out_ld=96) == -1 and b"below the width" in lib.ssn_last_error()
        assert dev(dtype=7) == -1 and b"boxes_dtype" in lib.ssn_last_error()
        assert dev(boxes=None) == -1 and b"null argument" in lib.ssn_last_error()
        assert dev(out=None) == -1 and b"null argument" in lib.ssn_last_error()
        assert dev(n=-1) == -1 and b"negative" in lib.ssn_last_error()
        assert dev(n=0, boxes=None, out=None) == 0                                      # n == 0 succeeds
        assert dev(samples=one.ctypes.data) == -1 and b"samples[1] = 1 below 2" in lib.ssn_last_error()
        assert dev(samples=two.ctypes.data, mean=1) == -1 and b"mean given together with samples" in lib.ssn_last_error()
        assert lib.ssn_encoder_encode_boxes(h, flat.ctypes.data, 4, one.ctypes.data, 0, host_out.ctypes.data) == -1 and b"below 2" in lib.ssn_last_error()
        assert lib.ssn_encoder_encode_boxes(h, flat.ctypes.data, 4, two.ctypes.data, 1, host_out.ctypes.data) == -1 and b"together with samples" in lib.ssn_last_error()
        assert lib.ssn_encoder_encode_boxes(h, None, 4, None, 0, host_out.ctypes.data) == -1 and b"null argument" in lib.ssn_last_error()
        assert dev(samples=two.ctypes.data) == 0
        assert bits(out.cpu().numpy()) == bits(enc.encode_region(boxes, samples=2))
        # hi < lo: host boxes by row, device boxes by the kernel's flag
        bad = boxes.copy()
        bad[2, 1] = bad[2, 1, ::-1]
        with pytest.raises(fe.SimulationError, match="box 2 has hi < lo"):
            enc.encode_region(bad)
        with pytest.raises(fe.SimulationError, match="box 2 has hi < lo"):
            enc.encode_region(bad.astype(np.float32), out="device")
        with pytest.raises(fe.SimulationError, match="a box has hi < lo"):
            enc.encode_region(torch.from_numpy(bad).to("cuda:0"), samples=3)
        assert bits(enc.encode_region(torch.from_numpy(boxes).to("cuda:0"), samples=3)) == bits(enc.encode_region(boxes, samples=3))      # the flag is cleared
        # the Python layer's own
        with pytest.raises(ValueError, match="mean given together with samples"):
            enc.encode_region(boxes, samples=20, mean=True)
        with pytest.raises(ValueError, match="below 2"):
            enc.encode_region(boxes, samples=[20, 1])
        with pytest.raises(ValueError, match=r"boxes must be \(N, 2, 2\)"):
            enc.encode_region(np.zeros((3, 3, 2)))
        with pytest.raises(ValueError, match="out must be"):
            enc.encode_region(boxes, out="gpu")
        enc.close()
        with pytest.raises(fe.SimulationError, match="closed"):
            enc.encode_region(boxes)


# -- 8. the public calls ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["hip", "hip-f64"])
def test_public_calls(SSPEncoder, backend):
    from sspslam_amd import harness as H
    dtype = "f32" if backend == "hip" else "f64"
    space = H.make_ssp_space(2, ssp_dim=97)
    boxes = rg.case_boxes("d97-2d")
    for mode, samples in (("integral", None), ("mean", None), ("mesh", 20)):
        ref = rg.Reference(space, boxes[:16], mode, samples)
        ref.check(space.encode_region(boxes[:16], samples=samples, mean=mode == "mean", backend=backend), dtype, label=f"SSPSpace.encode_region backend={backend}")
    cache = space.__dict__["_encoder_cache"]
    assert len(cache) == 1
    got = H.region_ssps(space, boxes[:16], backend=backend)
    want = H.region_ssps(space, boxes[:16])
    u = 2.0 ** -24 if dtype == "f32" else 2.0 ** -53
    np.testing.assert_allclose(np.linalg.norm(got, axis=1), 1.0, atol=8 * u)
    # a unit row moves by at most the relative error of the raw row, measured against its norm
    raw = rg.Reference(space, boxes[:16], "integral")
    slack = 2 * np.linalg.norm(raw.bar(dtype), axis=1) / np.linalg.norm(raw.want, axis=1)
    assert np.all(np.linalg.norm(got - want, axis=1) <= slack + 8 * u)
    space._drop_decoders()
    assert "_encoder_cache" not in space.__dict__


# -- 9. the example script's flags -----------------------------------------------------------------------------------------------------
def test_example_script_flags(SSPEncoder, capsys):
    """examples/run_slam.py --inverse-memory --area-query: the inverse memory builds beside the SLAM network, one line per box with a
    similarity per landmark; the flags' argument errors."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("run_slam_example", os.path.join(root, "examples", "run_slam.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = ["--ssp-dim", "7", "--pi-n-neurons", "64", "--mem-n-neurons", "70", "--circonv-n-neurons", "20", "--n-landmarks", "4", "--view-rad", "0.6",
            "--T", "2.0", "--limit", "0.5", "--decode-backend", "hip"]
    with pytest.raises(SystemExit, match="needs --inverse-memory"):
        mod.main(base + ["--area-query", "0", "1", "0", "1"])
    with pytest.raises(SystemExit, match="lo hi per axis: 4 numbers"):
        mod.main(base + ["--inverse-memory", "--area-query", "0", "1", "0"])
    capsys.readouterr()
    mod.main(base + ["--inverse-memory", "--area-query", "-1", "0", "-1", "0", "--area-query", "0", "1", "0", "1"])
    lines = capsys.readouterr().out.strip().splitlines()
    head = [line for line in lines if line.startswith("area queries: 2 boxes")]
    rows = [line for line in lines if line.startswith("  box [")]
    assert len(head) == 1 and "region encode" in head[0] and "recall" in head[0]
    assert len(rows) == 2 and rows[0].startswith("  box [-1, 0] x [-1, 0]: 0") and all(len(r.split(": ")[1].split("  ")) == 4 for r in rows)


# -- 10. area queries -------------------------------------------------------------------------------------------------------------------
_area = {}


def area():
    if not _area:
        from sspslam_amd.builder import build
        net, o = rg.area_network()
        _area["model"], _area["o"] = build(net), o
    return _area["model"], _area["o"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_area_query(SSPEncoder, dtype):
    """harness.area_query against the host formula on the two learned matrices read back, under the bound of recall_checks; the box
    that holds one trained location ranks that location's SP first."""
    from sspslam_amd import harness as H
    from sspslam_amd.simulator import Simulator
    model, o = area()
    mem, space, vocab, boxes = o["memory"], o["space"], o["vocab"], o["boxes"]
    backend = "hip" if dtype == "f32" else "hip-f64"
    u = rc.U32 if dtype == "f32" else rc.U64
    inside = np.all((rg.AREA_LOCATIONS[None, :, :] >= boxes[:, None, :, 0]) & (rg.AREA_LOCATIONS[None, :, :] <= boxes[:, None, :, 1]), axis=2)
    assert np.array_equal(inside, np.eye(3, dtype=bool))              # box i holds location i and no other
    with Simulator(None, model=model, dtype=dtype) as sim:
        sim.run_steps(rg.AREA_STEPS)
        be, bc = model.params[mem.memory], model.params[mem.conn_out]
        E, W = sim.read_buffer(be.encoder_buffer), sim.read_buffer(bc.learned_buffer)
        q = space.encode_region(boxes, samples=20, normalize=True, backend=backend)   # the keys area_query recalls with
        mesh = rg.Reference(space, boxes, "mesh", 20)
        mesh.check(space.encode_region(boxes, samples=20, backend=backend), dtype, label="area query keys")
        np.testing.assert_allclose(np.linalg.norm(q, axis=1), 1.0, atol=1e-15)
        for mode in ("reference", "network"):
            sims = H.area_query(sim, mem, space, boxes, vocab, samples=20, mode=mode, backend=backend)
            assert sims.shape == (3, 3) and sims.dtype == np.float64
            rc.check(sim.recall(mem, q, mode), q, E, W, be.gain, be.bias, be.neuron, mode, u, f"area query {dtype}")
            val, B = rc.bound(q, E, W, be.gain, be.bias, be.neuron, mode, u)
            host = val @ vocab.T
            err = np.abs(sims - host)
            allowed = B @ np.abs(vocab).T + (vocab.shape[1] + 2) * rc.U64 * (np.abs(val) @ np.abs(vocab).T)
            print(f"area query {dtype} {mode}: similarities\n{sims}\nworst err / allowed = {np.max(err / allowed):.3e}")
            assert np.all(err <= allowed)
            assert np.array_equal(np.argmax(sims, axis=1), np.arange(3)), sims
        assert bits(H.area_query(sim, mem, space, boxes[1], vocab, backend=backend)) == bits(H.area_query(sim, mem, space, boxes, vocab, backend=backend)[1:2])
    space._drop_decoders()
