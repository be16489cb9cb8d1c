"""service.rows_operand and service.backend_dtype - the one marshal and the one backend table of GridDecoder, SSPEncoder and
SSPBinder - on host data: NumPy arrays and CPU tensors.  No GPU and no library."""
import ctypes as C

import numpy as np
import pytest
import torch

from sspslam_amd import _lib, binding, decoding, encoding, service
from sspslam_amd.service import rows_operand

WHO = {"decoder": dict(what="rows", count="T"), "encoder": dict(what="points"), "binder": dict(what="a", ndim=(1, 2, 3))}


def operand(x, width, who="encoder", **kw):
    args = dict(WHO[who], **kw)
    return rows_operand(x, width, args.pop("what"), 0, who=who, **args)


def behind(op, dtype, width):
    """The values behind an operand's pointer, read the way the ABI reads them: n rows of ``width``, ``ld`` apart."""
    flat = np.ctypeslib.as_array(C.cast(op.ptr, C.POINTER(C.c_float if dtype == np.float32 else C.c_double)), shape=(op.n * op.ld,))
    return flat.reshape(op.n, op.ld)[:, :width].copy()


@pytest.mark.parametrize("width", [3, 5])
@pytest.mark.parametrize("tensor", [False, True], ids=["numpy", "cpu-tensor"])
def test_one_row_and_a_block_of_rows(width, tensor):
    rows = np.arange(4.0 * width).reshape(4, width) / 7.0
    for x, lead in ((rows[1], ()), (rows, (4,)), (rows[:1], (1,))):
        kept, got_lead, op = operand(torch.from_numpy(x) if tensor else x, width)
        assert got_lead == lead and op.n == int(np.prod(lead)) and op.ld == width and not op.on_device and op.code == _lib.SSN_F64
        assert kept.flags.c_contiguous and kept.shape == (op.n, width) and op.ptr == kept.ctypes.data
        assert np.array_equal(behind(op, np.float64, width), np.atleast_2d(x))


@pytest.mark.parametrize("width", [3, 5])
def test_three_axes_only_where_the_service_takes_them(width):
    x = np.arange(2.0 * 3 * width).reshape(2, 3, width)
    kept, lead, op = operand(x, width, "binder")
    assert lead == (2, 3) and op.n == 6 and op.ld == width and np.array_equal(behind(op, np.float64, width), x.reshape(6, width))
    with pytest.raises(ValueError, match=rf"points must be \(N, {width}\), got \(2, 3, {width}\)"):
        operand(x, width, "encoder")
    with pytest.raises(ValueError, match=rf"rows must be \(T, {width}\)"):
        operand(x, width, "decoder")


def test_float32_is_kept_or_widened_and_everything_else_is_widened():
    x32 = (np.arange(12.0).reshape(4, 3) / 3.0).astype(np.float32)
    kept, _, op = operand(x32, 3)
    assert kept.dtype == np.float32 and op.code == _lib.SSN_F32 and np.array_equal(behind(op, np.float32, 3), x32)
    kept, _, op = operand(x32, 3, "decoder", keep_f32=False)          # ssn_decoder_rows takes doubles
    assert kept.dtype == np.float64 and op.code == _lib.SSN_F64 and np.array_equal(behind(op, np.float64, 3), x32.astype(np.float64))
    for other in (np.arange(12).reshape(4, 3), x32.astype(np.float16), [[1, 2, 3], [4, 5, 6]], torch.arange(12).reshape(4, 3)):
        kept, _, op = operand(other, 3)
        assert kept.dtype == np.float64 and op.code == _lib.SSN_F64 and np.array_equal(kept, np.asarray(other, dtype=np.float64))


@pytest.mark.parametrize("who", sorted(WHO))
def test_no_rows_give_no_pointer(who):
    for dtype in (np.float32, np.float64):
        _, lead, op = operand(np.empty((0, 5), dtype=dtype), 5, who)
        assert lead == (0,) and op.n == 0 and op.ptr is None and op.ld == 5
    _, lead, op = operand(np.empty((0, 2, 5)), 5, "binder")
    assert lead == (0, 2) and op.n == 0 and op.ptr is None and op.ld == 5


def test_wrong_width_and_rank_raise_in_the_service_s_words():
    with pytest.raises(ValueError, match=r"rows must be \(T, 97\), got \(4, 96\)"):
        operand(np.zeros((4, 96)), 97, "decoder")
    with pytest.raises(ValueError, match=r"points must be \(N, 3\), got \(4, 5\)"):
        operand(np.zeros((4, 5)), 3, "encoder")
    with pytest.raises(ValueError, match=r"boxes must be \(N, 4\)"):
        operand(np.zeros((4, 5)), 4, "encoder", what="boxes")
    with pytest.raises(ValueError, match=r"b must be \(5,\), \(N, 5\) or \(S, L, 5\), got \(4, 3\)"):
        operand(np.zeros((4, 3)), 5, "binder", what="b")
    for who in WHO:
        with pytest.raises(ValueError, match="must be"):
            operand(np.float64(1.0), 3, who)                      # no axis at all
        with pytest.raises(ValueError, match="must be"):
            operand(np.zeros((2, 2, 2, 3)), 3, who)


@pytest.mark.parametrize("width", [3, 5])
def test_strided_host_rows_arrive_contiguous(width):
    wide = np.arange(4.0 * 2 * width).reshape(4, 2 * width)
    for x in (wide[:, ::2], wide[::2, :width], np.asfortranarray(wide[:, :width]), torch.from_numpy(wide)[:, ::2]):
        kept, _, op = operand(x, width)
        assert kept.flags.c_contiguous and op.ld == width and np.array_equal(behind(op, np.float64, width), np.asarray(x))


@pytest.mark.parametrize("module, what", [(decoding, "decode"), (encoding, "encode"), (binding, "bind")])
def test_backend_names(module, what):
    assert module.BACKENDS is service.BACKENDS
    for name, dtype in ((None, None), ("numpy", None), ("hip", "f32"), ("hip-f32", "f32"), ("hip-f64", "f64")):
        assert module.backend_dtype(name) == dtype and service.backend_dtype(name, what) == dtype
    for wrong in ("cuda", "f32", 0, ["hip"]):
        with pytest.raises(ValueError, match=f"unknown {what} backend"):
            module.backend_dtype(wrong)
