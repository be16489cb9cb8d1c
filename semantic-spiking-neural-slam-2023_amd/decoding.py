"""Grid decoding of SSP trajectories on the device: ``SSPSpace.decode(rows, 'from-set', 'grid', n)`` as one HIP call.

Every experiment of the reference ends with ``ssp_space.decode(sim.data[probe], 'from-set', 'grid', n)``
(``run_pathint.py:171-179``, ``run_slam.py:242-268``, ``run_slamview.py:167-192``): a ``(n^dim x d) . (d x T)`` product and an
argmax per row.  ``GridDecoder`` holds the sample table on the GPU and runs that as a product on the f32 matrix cores whose epilogue
keeps only each row's best column (``csrc/ssn_decode.hip`` behind ``ssn_decoder_*`` of ``include/ssn.h``); the ``T x n^dim``
similarity matrix never exists.  There is no CPU fallback: without a GPU the constructor raises.

    with GridDecoder(space, 100) as dec:
        est = dec.decode(sim.data[probe])              # == space.decode(sim.data[probe], 'from-set', 'grid', 100)

``SSPSpace.decode(..., backend="hip")`` does the same through a decoder cached on the space.
"""
import ctypes as C

import numpy as np

from . import _lib
from . import frontend as fe

__all__ = ["GridDecoder", "BACKENDS", "backend_dtype"]

# decode backends of SSPSpace.decode / clean_up and the harness: None is the NumPy path
BACKENDS = {None: None, "numpy": None, "hip": "f32", "hip-f32": "f32", "hip-f64": "f64"}


def backend_dtype(backend):
    """dtype of the GridDecoder behind a backend name, None for the NumPy path; ValueError for an unknown name."""
    try:
        return BACKENDS[backend]
    except (KeyError, TypeError):
        raise ValueError(f"unknown decode backend {backend!r}: one of None, 'numpy', 'hip', 'hip-f64'") from None


class GridDecoder:
    """Best sample per row, on the GPU.

    ``GridDecoder(ssp_space, num_samples, sampling_method)`` takes its table from ``ssp_space.get_sample_pts_and_ssps``;
    ``GridDecoder(samples=(sample_ssps, sample_points))`` takes it as ``SSPSpace.decode(samples=...)`` does (with ``ssp_space`` only
    needed for ``clean_up``).  ``dtype``: "f32" (matrix cores; the index agrees with the float64 host answer wherever the two best
    similarities differ by more than the f32 error of the product) or "f64" (parity mode).  ``scratch_bytes``: size of the device
    work area (default 64 MB); a smaller one only means more row chunks and fewer column strips, never another answer.

    Rows are scaled as the host scales them (divided by their norm when it is >= 1e-6).  Non-finite rows are out of contract: their
    index is some value inside ``[0, n_samples)``.
    """

    def __init__(self, ssp_space=None, num_samples=100, sampling_method="grid", samples=None, dtype="f32", device=0,
                 scratch_bytes=None):
        if dtype not in ("f32", "f64"):
            raise ValueError(f"dtype must be 'f32' or 'f64', got {dtype!r}")
        if samples is None:
            if ssp_space is None:
                raise ValueError("GridDecoder needs an ssp_space or samples=(sample_ssps, sample_points)")
            sample_ssps, sample_points = ssp_space.get_sample_pts_and_ssps(num_samples, sampling_method)
        else:
            sample_ssps, sample_points = samples
        table = np.ascontiguousarray(np.asarray(sample_ssps, dtype=np.float64))
        if table.ndim != 2:
            raise ValueError(f"sample_ssps must be (n_samples, width), got shape {table.shape}")
        self.ssp_space = ssp_space
        self.sample_points = np.asarray(sample_points)
        self.n_samples, self.width = int(table.shape[0]), int(table.shape[1])
        self.dtype, self.device = dtype, int(device)
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.closed = True
        rc = self._lib.ssn_decoder_create(_lib.SSN_F32 if dtype == "f32" else _lib.SSN_F64, self.device, table.ctypes.data,
                                          self.n_samples, self.width, int(scratch_bytes or 0), C.byref(self._h))
        if rc != 0:
            raise fe.BuildError(f"{_lib.STATUS.get(rc, rc)}: {_lib.last_error()}")
        self.closed = False

    # -- plumbing ------------------------------------------------------------------------------
    def _check(self, rc):
        if rc != 0:
            raise fe.SimulationError(f"{_lib.STATUS.get(rc, rc)}: {_lib.last_error()}")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if not self.closed:
            self._lib.ssn_decoder_destroy(self._h)
            self.closed = True

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self, n_rows=0):
        """How a call with ``n_rows`` rows is cut (row_chunk, n_chunks, n_strips, tiles_per_strip), the scratch sizes, and the
        launches / device milliseconds of the last call, as a dict."""
        if self.closed:
            raise fe.SimulationError("the decoder is closed")
        out = _lib.DecoderInfo()
        self._check(self._lib.ssn_decoder_get_info(self._h, int(n_rows), C.byref(out)))
        return {name: getattr(out, name) for name, _ in _lib.DecoderInfo._fields_}

    # -- decoding ------------------------------------------------------------------------------
    def indices(self, rows, return_sims=False):
        """Index of the best sample of every row (int64, lowest index on ties); with ``return_sims`` also the similarity of the
        scaled row to it.  ``rows``: array-like ``(T, width)`` (or one row), or a torch tensor on the decoder's device (float32 /
        float64, any row stride), which is read in place."""
        if self.closed:
            raise fe.SimulationError("the decoder is closed")
        tensor = hasattr(rows, "is_cuda") and hasattr(rows, "data_ptr")
        if tensor and not rows.is_cuda:
            rows, tensor = rows.detach().numpy(), False
        if tensor:
            import torch
            if rows.device.index != self.device:
                raise ValueError(f"rows live on {rows.device}, the decoder on device {self.device}")
            rows = rows.detach()
            if rows.dim() == 1:
                rows = rows[None, :]
            if rows.dtype not in (torch.float32, torch.float64):
                rows = rows.to(torch.float64)
            if rows.dim() != 2 or rows.shape[1] != self.width:
                raise ValueError(f"rows must be (T, {self.width}), got {tuple(rows.shape)}")
            n = int(rows.shape[0])
            if rows.stride(1) != 1 or (n > 1 and rows.stride(0) < self.width):
                rows = rows.contiguous()
            ld = max(int(rows.stride(0)), self.width) if n > 1 else self.width
            torch.cuda.current_stream(rows.device).synchronize()          # the rows are complete before the decoder's stream reads them
        else:
            rows = np.ascontiguousarray(np.atleast_2d(np.asarray(rows, dtype=np.float64)))
            if rows.ndim != 2 or rows.shape[1] != self.width:
                raise ValueError(f"rows must be (T, {self.width}), got {rows.shape}")
            n = int(rows.shape[0])
        best = np.empty(n, dtype=np.int32)
        sims = np.empty(n, dtype=np.float64) if return_sims else None
        sims_p = sims.ctypes.data if return_sims else None
        if tensor:
            code = _lib.SSN_F32 if rows.dtype == torch.float32 else _lib.SSN_F64
            self._check(self._lib.ssn_decoder_rows_device(self._h, rows.data_ptr() if n else None, code, ld, n, best.ctypes.data, sims_p))
        else:
            self._check(self._lib.ssn_decoder_rows(self._h, rows.ctypes.data, n, best.ctypes.data, sims_p))
        best = best.astype(np.int64)
        return (best, sims) if return_sims else best

    def indices_composed(self, rows):
        """Measurement aid (tools/bench_decode.py): the same indices from the composition this decoder replaces - the similarity
        matrix written out by ``k_gemm_nt_mfma_f32``, then ``k_argmax_partial`` over it.  f32, host rows, one chunk, at most 2 GB
        of similarities; ``info()["last_kernel_ms"]`` is its device time afterwards."""
        if self.closed:
            raise fe.SimulationError("the decoder is closed")
        rows = np.ascontiguousarray(np.atleast_2d(np.asarray(rows, dtype=np.float64)))
        if rows.ndim != 2 or rows.shape[1] != self.width:
            raise ValueError(f"rows must be (T, {self.width}), got {rows.shape}")
        best = np.empty(rows.shape[0], dtype=np.int32)
        self._check(self._lib.ssn_decoder_rows_composed(self._h, rows.ctypes.data, rows.shape[0], best.ctypes.data))
        return best.astype(np.int64)

    def decode(self, rows, return_sims=False):
        """``sample_points[best]``: what ``SSPSpace.decode(rows, 'from-set', ..., samples=...)`` returns."""
        if return_sims:
            best, sims = self.indices(rows, True)
            return self.sample_points[best], sims
        return self.sample_points[self.indices(rows)]

    def clean_up(self, rows):
        """The SSPs of the decoded points: ``ssp_space.encode(decode(rows))``."""
        if self.ssp_space is None:
            raise ValueError("clean_up needs the decoder's ssp_space")
        return self.ssp_space.encode(self.decode(rows))
