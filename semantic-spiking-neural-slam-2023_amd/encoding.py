"""SSP encoding of points on the device: ``SSPSpace.encode(x)`` as a phase kernel and one product.

With ``(K, M, w) = space.refine_tables()`` and ``th = x @ M.T``

    encode(x)[c] = sum_{k<K} w_k ( cos th_k cos(2 pi k c / d) - sin th_k sin(2 pi k c / d) )

so the SSPs of N points are ``P = [cos th, sin th]`` (N x 2K) times a fixed (2K x d) table.  ``SSPEncoder`` keeps that table on the GPU
(``csrc/ssn_encode.hip`` behind ``ssn_encoder_*`` of ``include/ssn.h``): the phases and their sincos are float64 in both dtypes, the
product runs on the f32 matrix cores ("f32") or as an ordered float64 chain ("f64", the parity mode).  There is no CPU fallback:
without a GPU the constructor raises.

    with SSPEncoder(space) as enc:
        ssps = enc.encode(path)                        # ~ space.encode(path), (N, d) float64
        dev = enc.encode(path, out="device")           # a torch tensor of the encoder's dtype, left on the GPU

``SSPSpace.encode(x, backend="hip")`` does the same through an encoder cached on the space.
"""
import ctypes as C

import numpy as np

from . import _lib
from . import frontend as fe

__all__ = ["SSPEncoder", "BACKENDS", "backend_dtype"]

# encode backends of SSPSpace.encode / clean_up: None is the NumPy path
BACKENDS = {None: None, "numpy": None, "hip": "f32", "hip-f32": "f32", "hip-f64": "f64"}


def backend_dtype(backend):
    """dtype of the SSPEncoder behind a backend name, None for the NumPy path; ValueError for an unknown name."""
    try:
        return BACKENDS[backend]
    except (KeyError, TypeError):
        raise ValueError(f"unknown encode backend {backend!r}: one of None, 'numpy', 'hip', 'hip-f64'") from None


def tables(space):
    """``(K, M, w)`` of ``space.refine_tables()`` as C-contiguous float64 arrays."""
    K, M, w = space.refine_tables()
    return int(K), np.ascontiguousarray(M, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64)


class SSPEncoder:
    """SSPs of points, on the GPU.

    ``SSPEncoder(space, dtype="f64", device=0, scratch_bytes=None)`` takes the phase matrix and length scale the space has at that
    moment.  ``dtype``: "f64" (every entry an ordered float64 sum) or "f32" (f32 matrix cores; the phases stay float64).
    ``scratch_bytes``: size of the device work area (default 64 MB); a smaller one only means more chunks, never another bit.
    """

    def __init__(self, space, dtype="f64", device=0, scratch_bytes=None):
        if dtype not in ("f32", "f64"):
            raise ValueError(f"dtype must be 'f32' or 'f64', got {dtype!r}")
        if space is None or not hasattr(space, "refine_tables"):
            raise ValueError("SSPEncoder needs an SSPSpace")
        K, M, w = tables(space)
        self.dim, self.width = int(space.domain_dim), int(space.ssp_dim)
        self.dtype, self.device = dtype, int(device)
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.closed = True
        rc = self._lib.ssn_encoder_create(_lib.SSN_F32 if dtype == "f32" else _lib.SSN_F64, self.device, self.width, K, self.dim,
                                          M.ctypes.data, w.ctypes.data, int(scratch_bytes or 0), C.byref(self._h))
        if rc != 0:
            raise fe.BuildError(f"{_lib.STATUS.get(rc, rc)}: {_lib.last_error()}")
        self.closed = False

    def _check(self, rc):
        if rc != 0:
            raise fe.SimulationError(f"{_lib.STATUS.get(rc, rc)}: {_lib.last_error()}")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if not self.closed:
            self._lib.ssn_encoder_destroy(self._h)
            self.closed = True

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self, n=0):
        """How a call with ``n`` points is cut (row_chunk, n_chunks), the scratch sizes, and the launches / device milliseconds
        (phase and product apart) of the last call, as a dict."""
        if self.closed:
            raise fe.SimulationError("the encoder is closed")
        out = _lib.EncoderInfo()
        self._check(self._lib.ssn_encoder_get_info(self._h, int(n), C.byref(out)))
        return {name: getattr(out, name) for name, _ in _lib.EncoderInfo._fields_}

    def _points_arg(self, x):
        """(points, n, (pointer, on_device, dtype code, leading dimension)): host points as a C-contiguous float32 / float64 array,
        device tensors as they are."""
        return self._rows_arg(x, self.dim, "points")

    def _boxes_arg(self, boxes):
        """``_points_arg`` for boxes ``(N, dim, 2)`` (or one ``(dim, 2)``): rows of ``lo_0, hi_0, lo_1, hi_1, ...``; a device tensor
        whose last two axes are dense is read in place, whatever its row stride."""
        tensor = hasattr(boxes, "is_cuda") and hasattr(boxes, "data_ptr")
        if not tensor:
            boxes = np.asarray(boxes)
            if boxes.dtype != np.float32:
                boxes = boxes.astype(np.float64)
        if boxes.ndim == 2:
            boxes = boxes[None]
        if boxes.ndim != 3 or tuple(boxes.shape[1:]) != (self.dim, 2):
            raise ValueError(f"boxes must be (N, {self.dim}, 2), got {tuple(boxes.shape)}")
        n = int(boxes.shape[0])
        if tensor and boxes.is_cuda and n > 1 and boxes.stride(2) == 1 and boxes.stride(1) == 2 and boxes.stride(0) >= 2 * self.dim:
            flat = boxes.as_strided((n, 2 * self.dim), (boxes.stride(0), 1))
        else:
            flat = boxes.reshape(n, 2 * self.dim)
        return self._rows_arg(flat, 2 * self.dim, "boxes")

    def _rows_arg(self, x, width, what):
        tensor = hasattr(x, "is_cuda") and hasattr(x, "data_ptr")
        if tensor and not x.is_cuda:
            x, tensor = x.detach().numpy(), False
        if tensor:
            import torch
            if x.device.index != self.device:
                raise ValueError(f"{what} live on {x.device}, the encoder on device {self.device}")
            x = x.detach()
            if x.dim() == 1:
                x = x[None, :]
            if x.dtype not in (torch.float32, torch.float64):
                x = x.to(torch.float64)
            if x.dim() != 2 or x.shape[1] != width:
                raise ValueError(f"{what} must be (N, {width}), got {tuple(x.shape)}")
            n = int(x.shape[0])
            if x.stride(1) != 1 or (n > 1 and x.stride(0) < width):
                x = x.contiguous()
            ld = max(int(x.stride(0)), width) if n > 1 else width
            torch.cuda.current_stream(x.device).synchronize()          # the rows are complete before the encoder's stream reads them
            return x, n, (x.data_ptr() if n else None, 1, _lib.SSN_F32 if x.dtype == torch.float32 else _lib.SSN_F64, ld)
        x = np.atleast_2d(np.asarray(x))
        x = np.ascontiguousarray(x, dtype=np.float32 if x.dtype == np.float32 else np.float64)
        if x.ndim != 2 or x.shape[1] != width:
            raise ValueError(f"{what} must be (N, {width}), got {x.shape}")
        n = int(x.shape[0])
        return x, n, (x.ctypes.data if n else None, 0, _lib.SSN_F32 if x.dtype == np.float32 else _lib.SSN_F64, width)

    def encode(self, x, out="host"):
        """SSPs of the points ``x``: array-like ``(N, dim)`` (or one point), or a torch tensor on the encoder's device (float32 /
        float64, any row stride), which is read in place.  ``out="host"``: an ``(N, d)`` float64 array.  ``out="device"``: a torch
        tensor of the encoder's dtype on its device."""
        if self.closed:
            raise fe.SimulationError("the encoder is closed")
        if out not in ("host", "device"):
            raise ValueError(f"out must be 'host' or 'device', got {out!r}")
        x, n, (ptr, on_device, code, ld) = self._points_arg(x)
        if out == "host" and not on_device and code == _lib.SSN_F64:
            res = np.empty((n, self.width), dtype=np.float64)
            self._check(self._lib.ssn_encoder_encode(self._h, ptr, n, res.ctypes.data))
            return res
        import torch
        res = torch.empty((n, self.width), dtype=torch.float32 if self.dtype == "f32" else torch.float64, device=f"cuda:{self.device}")
        torch.cuda.current_stream(res.device).synchronize()
        self._check(self._lib.ssn_encoder_encode_device(self._h, ptr, on_device, code, ld, n, res.data_ptr() if n else None, self.width))
        return res if out == "device" else res.cpu().to(torch.float64).numpy()

    @property
    def region_min_scratch(self):
        """The smallest ``scratch_bytes`` ``encode_region`` accepts: one 64-box tile (a box row stages ``2 dim`` doubles)."""
        return int(self.info()["min_scratch_bytes"]) + 64 * 8 * self.dim

    def encode_region(self, boxes, samples=None, mean=False, normalize=False, out="host"):
        """SSPs of axis-aligned boxes in closed form (``k_encode_phase_box``).  ``boxes``: ``(N, dim, 2)`` rows of
        ``[lo, hi]`` per axis (the layout of ``domain_bounds``) or one ``(dim, 2)``, array-like or a torch tensor on the encoder's
        device.  ``samples=None``: the integral of ``encode`` over each box, or with ``mean=True`` its mean (a zero-width box is then
        ``encode(centre)``).  ``samples``: an int or one per axis (>= 2) - the sum of ``encode`` over that linspace mesh, both ends
        included (``get_sims_for_area`` of slam_map_new.py with 20).  ``normalize``: every row divided by ``max(norm, 1e-8)`` like
        ``SSPSpace.normalize`` (on the device for ``out="device"``).  Returns as ``encode`` does."""
        if self.closed:
            raise fe.SimulationError("the encoder is closed")
        if out not in ("host", "device"):
            raise ValueError(f"out must be 'host' or 'device', got {out!r}")
        counts = region_samples(self.dim, samples, mean)
        sp = counts.ctypes.data if counts is not None else None
        x, n, (ptr, on_device, code, ld) = self._boxes_arg(boxes)
        if out == "host" and not on_device and code == _lib.SSN_F64:
            res = np.empty((n, self.width), dtype=np.float64)
            self._check(self._lib.ssn_encoder_encode_boxes(self._h, ptr, n, sp, int(bool(mean)), res.ctypes.data))
            return unit_rows(res) if normalize else res
        import torch
        res = torch.empty((n, self.width), dtype=torch.float32 if self.dtype == "f32" else torch.float64, device=f"cuda:{self.device}")
        torch.cuda.current_stream(res.device).synchronize()
        self._check(self._lib.ssn_encoder_encode_boxes_device(self._h, ptr, on_device, code, ld, n, sp, int(bool(mean)),
                                                              int(bool(normalize) and out == "device"), res.data_ptr() if n else None, self.width))
        if out == "device":
            return res
        res = res.cpu().to(torch.float64).numpy()
        return unit_rows(res) if normalize else res


def region_samples(dim, samples, mean):
    """The per-axis mesh counts of ``encode_region`` as an int32 array (None without a mesh); ValueError for a count below 2, a
    wrong number of counts, or ``mean`` beside ``samples``."""
    if samples is None:
        return None
    if mean:
        raise ValueError("mean given together with samples: the mean of a mesh is its sum over the number of points")
    counts = np.asarray(samples)
    if counts.ndim == 0:
        counts = np.full(dim, counts)
    if counts.shape != (dim,) or not np.issubdtype(counts.dtype, np.integer):
        raise ValueError(f"samples must be an int or {dim} ints, got {samples!r}")
    if np.any(counts < 2):
        raise ValueError(f"samples {counts.tolist()} below 2: a linspace mesh has both ends")
    return np.ascontiguousarray(counts, dtype=np.int32)


def unit_rows(v):
    """Every row over ``max(norm, 1e-8)``: ``SSPSpace.normalize`` applied per row."""
    return v / np.maximum(np.sqrt(np.sum(v * v, axis=1, keepdims=True)), 1e-8)
