"""Similarity maps on the GPU (k_decode_map of csrc/ssn_decode.hip behind GridDecoder.similarity), held to the instrument of
tests/map_checks.py: every entry of every row within the f32 bar (f64 bar in f64), the map bit for bit consistent with the decode
of the same decoder, and the same bits however the call is made."""
import ctypes as C

import numpy as np
import pytest

import map_checks as mc

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f64"]
CASES = list(mc.C)
NP = {"f32": np.float32, "f64": np.float64}


@pytest.fixture(scope="module")
def GridDecoder():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from sspslam_amd.decoding import GridDecoder
    return GridDecoder


def make(GridDecoder, name, dtype, **kw):
    space, rows, table, points = mc.case(name)
    if space is None:
        return GridDecoder(samples=(table, points), dtype=dtype, **kw)
    return GridDecoder(space, mc.STANDARD[name][0][2], dtype=dtype, **kw)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# -- 1. every entry within the bars -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", CASES)
def test_every_entry_within_the_bars(GridDecoder, name, dtype):
    _, rows, table, _ = mc.case(name)
    with make(GridDecoder, name, dtype) as dec:
        assert (dec.n_samples, dec.width) == table.shape
        for normalize in (False, True):
            ref = mc.MapReference(table, rows, normalize, mc.C[name])
            m1 = dec.similarity(rows, power=1, normalize=normalize)
            info = dec.info(rows.shape[0])
            m2 = dec.similarity(rows, power=2, normalize=normalize)
            assert m1.shape == m2.shape == (rows.shape[0], table.shape[0]) and m1.dtype == m2.dtype == np.float64
            print(f"{name} {dtype} normalize={normalize}: worst error / bar {ref.worst(m1, dtype):.3f} (power 1), {ref.worst(m2, dtype, 2):.3f} (power 2)")
            assert ref.ok(m1, dtype).all(), ref.worst(m1, dtype)
            assert ref.ok(m2, dtype, 2).all(), ref.worst(m2, dtype, 2)
            # the square is one multiply in the decoder's dtype (the host map of an f32 decoder is that f32 value widened)
            narrow = m1.astype(NP[dtype])
            assert same_bits(narrow.astype(np.float64), m1)
            assert same_bits((narrow * narrow).astype(np.float64), m2)
            assert info["last_launches"] == 2 and info["last_kernel_ms"] > 0      # prepare + k_decode_map, one chunk
        assert dec.similarity(np.zeros((0, table.shape[1]))).shape == (0, table.shape[0])


# -- 2. the map is the decode's own similarities --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", CASES)
def test_argmax_of_the_map_is_indices(GridDecoder, name, dtype):
    _, rows, _, _ = mc.case(name)
    with make(GridDecoder, name, dtype) as dec:
        m = dec.similarity(rows, normalize=True)
        np.testing.assert_array_equal(np.argmax(m, axis=1), dec.indices(rows))


@pytest.mark.parametrize("dtype", DTYPES)
def test_argmax_on_exact_ties_and_near_ties(GridDecoder, dtype):
    _, rows, table, points = mc.case("s144")
    table = np.array(table)
    table[100] = table[30]                                             # bit-equal columns of the map: the lower index wins
    table[143] = table[129]                                            # and inside the ragged second column tile
    between = table[40] + table[41]                                    # equidistant between two samples
    probe = np.vstack([table[30] * 2.5, table[129], between, 0.3 * between, rows[:60]])
    with GridDecoder(samples=(table, points), dtype=dtype) as dec:
        m = dec.similarity(probe, normalize=True)
        idx = dec.indices(probe)
    assert same_bits(m[:, 100], m[:, 30]) and same_bits(m[:, 143], m[:, 129])
    np.testing.assert_array_equal(np.argmax(m, axis=1), idx)
    assert idx[0] == 30 and idx[1] == 129 and idx[2] in (40, 41) and idx[3] in (40, 41)


# -- 3. the same bits however it is called --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_same_bits_however_it_is_called(GridDecoder, dtype):
    import torch
    space, rows, table, _ = mc.case("s144")
    T, S, d = rows.shape[0], table.shape[0], table.shape[1]
    rows = rows.astype(np.float32).astype(np.float64)                  # f32-representable: a float32 tensor holds the same values
    kw = dict(power=2, normalize=True)
    with GridDecoder(space, 12, dtype=dtype) as dec:
        info = dec.info(T)
        base = dec.similarity(rows, **kw)
        assert dec.info(T)["last_launches"] == 2
        assert same_bits(dec.similarity(rows, **kw), base)                                       # two runs
        dev = dec.similarity(rows, out="device", **kw)
        assert dev.is_cuda and dev.shape == (T, S) and dev.dtype == (torch.float32 if dtype == "f32" else torch.float64)
        assert same_bits(dev.cpu().numpy().astype(np.float64), base)
        into = torch.full((T, S + 9), -7.0, dtype=dev.dtype, device="cuda:0")[:, :S]
        assert dec.similarity(rows, into=into, **kw) is into and into.stride(0) == S + 9
        assert same_bits(into.cpu().numpy().astype(np.float64), base)
        r64 = torch.from_numpy(rows).to("cuda:0")
        r32 = r64.to(torch.float32)
        wide = torch.full((T, d + 13), float("nan"), dtype=torch.float64, device="cuda:0")
        wide[:, :d] = r64
        for t in (r64, r32, wide[:, :d]):
            assert same_bits(dec.similarity(t, **kw), base)
        assert same_bits(dec.similarity(wide[:, :d], out="device", **kw).cpu().numpy().astype(np.float64), base)
        # the map stage at its minimum (one 128-row tile of the host dtype): three chunks instead of one
        dec.set_map_stage(128 * S * 8)
        assert same_bits(dec.similarity(rows, **kw), base) and dec.info(T)["last_launches"] == 6
        assert same_bits(dec.similarity(r32, **kw), base)
        dec.set_map_stage(0)
        assert same_bits(dec.similarity(rows, **kw), base) and dec.info(T)["last_launches"] == 2
        raw = dec.similarity(rows)
    with GridDecoder(space, 12, dtype=dtype, scratch_bytes=info["min_scratch_bytes"]) as small:      # one row tile per chunk
        assert small.info(T)["n_chunks"] == 3
        assert same_bits(small.similarity(rows, **kw), base) and small.info(T)["last_launches"] == 6
        assert same_bits(small.similarity(rows, out="device", **kw).cpu().numpy().astype(np.float64), base)
        small.set_map_stage(128 * S * 8)
        assert same_bits(small.similarity(rows), raw)


# -- 4. nothing but the map is written ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["s144", "line", "w7"])
def test_into_a_slice_leaves_the_parent_alone(GridDecoder, name, dtype):
    import torch
    _, rows, table, _ = mc.case(name)
    T, S = rows.shape[0], table.shape[0]
    with make(GridDecoder, name, dtype) as dec:
        want = dec.similarity(rows, normalize=True)
        parent = torch.full((T + 130, S + 140), -7.0, dtype=torch.float32 if dtype == "f32" else torch.float64, device="cuda:0")
        got = dec.similarity(rows, normalize=True, into=parent[:T, :S])
    host = parent.cpu().numpy()
    assert mc.padding_ok(host, T, S, -7.0)                             # columns >= S and rows >= T keep the sentinel
    assert same_bits(host[:T, :S].astype(np.float64), want) and same_bits(got.cpu().numpy(), host[:T, :S])


def test_f32_host_maps_are_the_float64_ones_narrowed(GridDecoder):
    _, rows, table, _ = mc.case("s400")
    with make(GridDecoder, "s400", "f32") as dec:
        for power in (1, 2):
            m64 = dec.similarity(rows, power=power, normalize=True)
            m32 = dec.similarity(rows, power=power, normalize=True, out_dtype="f32")
            assert m32.dtype == np.float32 and same_bits(m32, m64.astype(np.float32)) and same_bits(m32.astype(np.float64), m64)
        dec.set_map_stage(128 * table.shape[0] * 4)                    # one tile of float32: two chunks for 129 rows
        assert same_bits(dec.similarity(rows, power=2, normalize=True, out_dtype="f32"), m32) and dec.info()["last_launches"] == 4


# -- 5. the space and the harness -----------------------------------------------------------------------------------------------
def test_space_and_harness_backends(GridDecoder):
    space, rows, table, _ = mc.case("s144")
    n, c = 12, mc.C["s144"]
    for backend, dtype, kw in (("hip", "f32", {"table": "device"}), ("hip", "f32", {}), ("hip-f64", "f64", {})):
        for normalize in (False, True):
            ref = mc.MapReference(table, rows, normalize, c)
            host = space.similarity_map(rows, n, power=2, normalize=normalize)
            got = space.similarity_map(rows, n, power=2, normalize=normalize, backend=backend, **kw)
            assert got.dtype == np.float64 and ref.ok(host, "f64", 2).all()
            assert ref.ok(got, dtype, 2).all(), (backend, kw, ref.worst(got, dtype, 2))
    frames = np.array(rows[3:15]).reshape(3, 4, -1)
    ref = mc.MapReference(table, frames.reshape(12, -1), True, c)
    from sspslam_amd import harness as H
    host = H.similarity_frames(space, frames, n, normalize=True)
    got = H.similarity_frames(space, frames, n, normalize=True, backend="hip")
    assert got.shape == host.shape == (3, 4, n, n)
    assert ref.ok(host.reshape(12, -1), "f64", 2).all() and ref.ok(got.reshape(12, -1), "f32", 2).all()
    got = space.similarity_map(rows, samples=(table, None), backend="hip")
    assert mc.MapReference(table, rows, False, c).ok(got, "f32").all()
    space._drop_decoders()


# -- 6. the decoder is what it was ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_decoding_after_maps_is_a_fresh_decoders(GridDecoder, dtype):
    space, rows, _, _ = mc.case("s144")
    with GridDecoder(space, 12, dtype=dtype) as fresh:
        want = (fresh.decode(rows), *fresh.indices(rows, return_sims=True), *fresh.refine(rows, return_info=True))
    with GridDecoder(space, 12, dtype=dtype) as dec:
        dec.similarity(rows, power=2)
        dec.similarity(rows, normalize=True, out="device")
        dec.set_map_stage(128 * 144 * 8)
        dec.similarity(rows)
        got = (dec.decode(rows), *dec.indices(rows, return_sims=True), *dec.refine(rows, return_info=True))
        dec.similarity(rows[:5])
        again = dec.indices(rows, return_sims=True)
    for g, w in zip(got, want):
        assert same_bits(g, w)
    assert same_bits(again[0], want[1]) and same_bits(again[1], want[2])


# -- 7. rejected arguments ------------------------------------------------------------------------------------------------------
def test_rejected_arguments(GridDecoder):
    import torch
    from sspslam_amd import _lib
    from sspslam_amd import frontend as fe
    space, rows, table, _ = mc.case("s144")
    T, S, d = rows.shape[0], table.shape[0], table.shape[1]
    lib = _lib.load()
    rows = np.array(rows)                                              # a writable, contiguous copy
    out = np.full((T, S), -7.0)
    dev_rows = torch.from_numpy(rows).to("cuda:0")

    def call(dec, rows_p=rows.ctypes.data, on_dev=0, rdt=0, rld=d, n=T, flags=0, out_p=out.ctypes.data, out_dev=0, odt=_lib.SSN_F64, old=S):
        rc = lib.ssn_decoder_map(dec, rows_p, on_dev, rdt, rld, n, flags, out_p, out_dev, odt, old)
        return rc, _lib.last_error()

    EINVAL = -1
    assert _lib.STATUS[EINVAL] == "SSN_EINVAL"
    with GridDecoder(space, 12, dtype="f32") as dec, GridDecoder(space, 12, dtype="f64") as dec64:
        h = dec._h
        for kwargs, msg in ((dict(dec=None), "null decoder"), (dict(flags=4), "unknown flags"), (dict(flags=-1), "unknown flags"),
                            (dict(rows_p=None), "null argument"), (dict(out_p=None), "null argument"), (dict(n=-1), "negative n_rows"),
                            (dict(old=S - 1), "below n_samples"), (dict(odt=7), "unknown out_dtype"),
                            (dict(rows_p=dev_rows.data_ptr(), on_dev=1, rdt=_lib.SSN_F64, rld=d - 1), "below the width"),
                            (dict(rows_p=dev_rows.data_ptr(), on_dev=1, rdt=5), "unknown rows_dtype")):
            rc, err = call(**{"dec": h, **kwargs})
            assert rc == EINVAL and msg in err, (kwargs, rc, err)
        rc, err = call(dec64._h, odt=_lib.SSN_F32)
        assert rc == EINVAL and "narrower" in err
        # a stage below one tile: of the decoder's dtype when it is set, of the output's dtype when a host map needs it
        assert lib.ssn_decoder_set_map_stage(None, 0) == EINVAL
        assert lib.ssn_decoder_set_map_stage(h, 128 * S * 4 - 1) == EINVAL and "too small for one" in _lib.last_error()
        assert lib.ssn_decoder_set_map_stage(h, -1) == EINVAL
        assert lib.ssn_decoder_set_map_stage(h, 128 * S * 4) == 0
        rc, err = call(h)                                              # float64 host output: one tile is 128 S 8 bytes
        assert rc == EINVAL and "too small for one" in err
        with pytest.raises(fe.SimulationError, match="SSN_EINVAL.*too small for one"):
            dec.similarity(rows)
        assert dec.similarity(rows, out_dtype="f32").shape == (T, S)   # float32 fits
        with pytest.raises(fe.SimulationError, match="too small for one"):
            dec.set_map_stage(5)
        assert (out == -7.0).all()                                     # no rejected call wrote anything
        rc, _ = call(h, n=0)
        assert rc == 0 and (out == -7.0).all()                         # n_rows == 0 succeeds and writes nothing
        rc, _ = call(h, n=0, rows_p=None, out_p=None)
        assert rc == 0
        # Python: ValueError before any launch
        launches = dec.info()["last_launches"]
        for kw, msg in ((dict(power=3), "power must be 1 or 2"), (dict(power=0), "power must be 1 or 2"), (dict(out="gpu"), "out must be"),
                        (dict(out_dtype="f16"), "out_dtype must be"), (dict(out="device", out_dtype="f64"), "decoder's dtype"),
                        (dict(into=torch.zeros((T, S), dtype=torch.float64, device="cuda:0")), "decoder's dtype"),
                        (dict(into=torch.zeros((T, S), dtype=torch.float32)), "decoder's device"),
                        (dict(into=torch.zeros((T, S + 1), dtype=torch.float32, device="cuda:0")), "into= must be"),
                        (dict(into=torch.zeros((S, T), dtype=torch.float32, device="cuda:0").T), "unit column stride"),
                        (dict(into=torch.zeros((T, 2 * S), dtype=torch.float32, device="cuda:0")[:, ::2]), "unit column stride")):
            with pytest.raises(ValueError, match=msg):
                dec.similarity(rows, **kw)
        with pytest.raises(ValueError, match=r"rows must be \(T, 97\)"):
            dec.similarity(rows[:, :50])
        with pytest.raises(ValueError, match="not offered"):
            dec64.similarity(rows, out_dtype="f32")
        assert dec.info()["last_launches"] == launches
    with pytest.raises(fe.SimulationError, match="closed"):
        dec.similarity(rows)
