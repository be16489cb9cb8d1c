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
import functools

import numpy as np

from . import _lib, service
from .service import BACKENDS

__all__ = ["SSPEncoder", "BACKENDS", "backend_dtype"]

backend_dtype = functools.partial(service.backend_dtype, what="encode")      # (backend) -> the SSPEncoder's dtype, None: NumPy


def tables(space):
    """``(K, M, w)`` of ``space.refine_tables()`` as C-contiguous float64 arrays."""
    K, M, w = space.refine_tables()
    return int(K), np.ascontiguousarray(M, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64)


class SSPEncoder(service.DeviceService):
    """SSPs of points, on the GPU.

    ``SSPEncoder(space, dtype="f64", device=0, scratch_bytes=None)`` takes the phase matrix and length scale the space has at that
    moment.  ``dtype``: "f64" (every entry an ordered float64 sum) or "f32" (f32 matrix cores; the phases stay float64).
    ``scratch_bytes``: size of the device work area (default 64 MB); a smaller one only means more chunks, never another bit.
    """

    noun, destroy = "encoder", "ssn_encoder_destroy"

    def __init__(self, space, dtype="f64", device=0, scratch_bytes=None):
        super().__init__(dtype, device)
        if space is None or not hasattr(space, "refine_tables"):
            raise ValueError("SSPEncoder needs an SSPSpace")
        K, M, w = tables(space)
        self.dim, self.width = int(space.domain_dim), int(space.ssp_dim)
        self._create("ssn_encoder_create", self.width, K, self.dim, M.ctypes.data, w.ctypes.data, int(scratch_bytes or 0))

    def info(self, n=0):
        """How a call with ``n`` points is cut (row_chunk, n_chunks), the scratch sizes, and the launches / device milliseconds
        (phase and product apart) of the last call, as a dict."""
        return self._info(_lib.EncoderInfo, "ssn_encoder_get_info", n)

    def _boxes(self, boxes):
        """``service.rows_operand`` for boxes ``(N, dim, 2)`` (or one ``(dim, 2)``) as rows of ``lo_0, hi_0, lo_1, hi_1, ...``; a
        device tensor whose last two axes are dense is read in place, whatever its row stride."""
        tensor = hasattr(boxes, "is_cuda") and hasattr(boxes, "data_ptr")
        if not tensor:
            boxes = np.asarray(boxes)
        if boxes.ndim == 2:
            boxes = boxes[None]
        if boxes.ndim != 3 or tuple(boxes.shape[1:]) != (self.dim, 2):
            raise ValueError(f"boxes must be (N, {self.dim}, 2), got {tuple(boxes.shape)}")
        n = int(boxes.shape[0])
        if tensor and boxes.is_cuda and n > 1 and boxes.stride(2) == 1 and boxes.stride(1) == 2 and boxes.stride(0) >= 2 * self.dim:
            flat = boxes.as_strided((n, 2 * self.dim), (boxes.stride(0), 1))
        else:
            flat = boxes.reshape(n, 2 * self.dim)
        return service.rows_operand(flat, 2 * self.dim, "boxes", self.device, who="encoder")

    def _encode(self, op, out, host_fn, device_fn, mode=(), device_mode=(), normalize=False):
        """The tail of both encodes.  Host float64 rows to a host result are one ABI call, ``host_fn(handle, rows, n, *mode,
        result)``; anything else goes through a device result, ``device_fn(handle, *op, *mode, *device_mode, result, leading
        dimension)``.  ``normalize``: the rows of a host result over ``max(norm, 1e-8)`` (the call normalises a device result)."""
        if out == "host" and not op.on_device and op.code == _lib.SSN_F64:
            res = np.empty((op.n, self.width), dtype=np.float64)
            self._check(host_fn(self._h, op.ptr, op.n, *mode, res.ctypes.data))
        else:
            res, ld = service.result(self, op.n, self.width)
            self._check(device_fn(self._h, *op, *mode, *device_mode, res.data_ptr() if op.n else None, ld))
            res = service.finish(res, out)
        return unit_rows(res) if normalize and out == "host" else res

    def encode(self, x, out="host"):
        """SSPs of the points ``x``: array-like ``(N, dim)`` (or one point), or a torch tensor on the encoder's device (float32 /
        float64, any row stride), which is read in place.  ``out="host"``: an ``(N, d)`` float64 array.  ``out="device"``: a torch
        tensor of the encoder's dtype on its device."""
        self._open()
        service.check_out(out)
        x, _, op = service.rows_operand(x, self.dim, "points", self.device, who="encoder")
        return self._encode(op, out, self._lib.ssn_encoder_encode, self._lib.ssn_encoder_encode_device)

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
        self._open()
        service.check_out(out)
        counts = region_samples(self.dim, samples, mean)
        mode = (counts.ctypes.data if counts is not None else None, int(bool(mean)))
        x, _, op = self._boxes(boxes)
        return self._encode(op, out, self._lib.ssn_encoder_encode_boxes, self._lib.ssn_encoder_encode_boxes_device, mode,
                            (int(bool(normalize) and out == "device"),), normalize)

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
