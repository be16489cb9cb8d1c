"""One strided device tensor through GridDecoder, SSPEncoder and SSPBinder (service.rows_operand on the GPU): the leading dimension
a service is handed, and the contiguous copy where a tensor cannot be read in place, against the same values passed contiguous."""
import numpy as np
import pytest

from sspslam_amd import SSPBinder, SSPEncoder
from sspslam_amd.decoding import GridDecoder
from sspslam_amd.sspspace import SSPSpace, conjsym

pytestmark = pytest.mark.gpu
N, W = 5, 12


def views(torch, tdtype):
    """(name, a (5, 12) view of a larger device tensor): rows 16 apart with unit column stride - read in place with ld = 16 - and
    rows 12 apart with columns 2 apart, which no leading dimension describes."""
    rng = np.random.RandomState(5)
    wide = torch.tensor(rng.uniform(-1, 1, (8, 16)), dtype=tdtype, device="cuda")
    long = torch.tensor(rng.uniform(-1, 1, 12 * (N - 1) + 2 * W), dtype=tdtype, device="cuda")
    return (("ld 16", wide[:N, :W]), ("column stride 2", long.as_strided((N, W), (12, 2))))


@pytest.mark.parametrize("dtype", ("f32", "f64"))
@pytest.mark.parametrize("tensor_dtype", ("float32", "float64"))
def test_strided_device_rows_equal_their_contiguous_copy(dtype, tensor_dtype):
    import torch
    rng = np.random.RandomState(11)
    space = SSPSpace(W, 13, conjsym(rng.uniform(-2, 2, (6, W))))          # points of 12 axes: the encoder's rows are 12 wide too
    table, points = rng.uniform(-1, 1, (40, W)), rng.uniform(-1, 1, (40, 2))
    with GridDecoder(samples=(table, points), dtype=dtype) as dec, SSPEncoder(space, dtype=dtype) as enc, SSPBinder(W, dtype=dtype) as binder:
        for name, view in views(torch, getattr(torch, tensor_dtype)):
            assert view.shape == (N, W) and not view.is_contiguous()
            dense = view.contiguous()
            assert dense.data_ptr() != view.data_ptr() and torch.equal(dense, view)
            for what, call in (("indices", lambda x: dec.indices(x, return_sims=True)[1]),
                               ("similarity", lambda x: dec.similarity(x, normalize=True)),
                               ("similarity on the device", lambda x: dec.similarity(x, power=2, out="device").cpu().numpy()),
                               ("encode", enc.encode),
                               ("encode on the device", lambda x: enc.encode(x, out="device").cpu().numpy()),
                               ("bind", lambda x: binder.bind(x, x, invert_b=True)),
                               ("bind with host rows", lambda x: binder.bind(dense.cpu().numpy()[::-1].copy(), x, out="device").cpu().numpy())):
                got, want = call(view), call(dense)
                assert got.shape == want.shape and got.shape[0] == N and np.any(want != 0), (name, what)
                assert got.tobytes() == want.tobytes(), (name, what)
            assert np.array_equal(dec.indices(view), dec.indices(dense)), name
