"""Binding on the device: ``SSPSpace.bind(a, b)`` / ``SPSpace.bind(a, b)`` - ``ifft(fft(a) * fft(b)).real`` per row - as one HIP call.

``SSPBinder`` (``csrc/ssn_bind.hip`` behind ``ssn_binder_*`` of ``include/ssn.h``) depends on the width ``d`` and the
dtype only, so one serves an ``SSPSpace`` and an ``SPSpace`` alike.  "f32": one workgroup per output row runs the whole circular
convolution in LDS (``k_bind_rows``: both rows in one complex transform, balanced by a power of two); "f64", the parity mode: every
entry an ordered fma chain (``k_bind_direct``).  The operands' inversion, the pairing of one pose row with the L landmark rows of its
sample and the normalisation of the landmark vector queries (``slam_map_new.py:453-485``) ride in the same launch.  There is no CPU
fallback: without a GPU the constructor raises.

    with SSPBinder(space) as binder:
        rel = binder.bind(poses, frames, invert_a=True, normalize=True, norm_floor=1e-6)      # (S, d) x (S, L, d) -> (S, L, d)

``space.bind(a, b, backend="hip")`` does the plain product through a binder cached on the space.
"""
import functools

import numpy as np

from . import _lib, service
from .service import BACKENDS

__all__ = ["SSPBinder", "BACKENDS", "backend_dtype"]

backend_dtype = functools.partial(service.backend_dtype, what="bind")      # (backend) -> the SSPBinder's dtype, None: NumPy


class SSPBinder(service.DeviceService):
    """Circular convolution of rows, on the GPU.

    ``SSPBinder(d_or_space, dtype="f32", device=0, scratch_bytes=None)``: the width, or a space to take it from (``ssp_dim`` of an
    ``SSPSpace``, ``dim`` of an ``SPSpace``).  ``scratch_bytes``: size of the device work area (default 64 MB); a smaller one only
    means more chunks, never another bit.
    """

    noun, destroy = "binder", "ssn_binder_destroy"

    def __init__(self, d_or_space, dtype="f32", device=0, scratch_bytes=None):
        super().__init__(dtype, device)
        d = getattr(d_or_space, "ssp_dim", None)
        if d is None:
            d = getattr(d_or_space, "dim", d_or_space)
        if isinstance(d, bool) or not isinstance(d, (int, np.integer)):
            raise ValueError(f"SSPBinder needs a width or a space, got {d_or_space!r}")
        self.width = int(d)
        self._create("ssn_binder_create", self.width, int(scratch_bytes or 0))

    def info(self, n=0):
        """How a call with ``n`` output rows is cut (row_chunk, n_chunks), the scratch sizes, the planned route (transform_length,
        bluestein_m, radices, threads, lds_bytes) and the launches / device milliseconds of the last call, as a dict."""
        res = self._info(_lib.BinderInfo, "ssn_binder_get_info", n)
        res["radices"] = tuple(int(r) for r in res["radices"][:res["n_radices"]])
        return res

    def bind(self, a, b, invert_a=False, invert_b=False, normalize=False, norm_floor=1e-8, out="host", into=None):
        """``a (*) b`` row by row.  ``a``, ``b``: array-likes or torch tensors on the binder's device (float32 / float64, any row
        stride, read in place), shaped ``(d,)``, ``(N, d)`` or ``(S, L, d)``; the operand with fewer rows is paired with the other's
        rows as 1 : n or as one row per group of ``n / count`` consecutive rows - ``(S, d)`` with ``(S, L, d)`` gives ``(S, L, d)``.
        ``invert_a`` / ``invert_b``: that operand is read at ``(d - i) mod d`` (``space.invert``).  ``normalize``: every output row
        over ``max(norm, norm_floor)``.  ``out="host"``: a float64 array; ``out="device"``: a torch tensor of the binder's dtype.
        ``into``: a caller's 2-D device tensor of the binder's dtype (any row stride) whose ``[:n, :d]`` receives the rows -
        nothing else of it is touched; it is returned."""
        self._open()
        service.check_out(out)
        d = self.width
        a, lead_a, op_a = service.rows_operand(a, d, "a", self.device, who="binder", ndim=(1, 2, 3))
        b, lead_b, op_b = service.rows_operand(b, d, "b", self.device, who="binder", ndim=(1, 2, 3))
        n = max(op_a.n, op_b.n)
        for what, cnt in (("a", op_a.n), ("b", op_b.n)):
            if n and (cnt == 0 or n % cnt):
                raise ValueError(f"{cnt} rows of {what} do not pair with {n} output rows (1, n, or a divisor of n)")
        if op_a.n != op_b.n:
            lead = lead_a if op_a.n > op_b.n else lead_b
        else:
            lead = lead_a if len(lead_a) >= len(lead_b) else lead_b
        lead = tuple(lead) or (1,)          # two single rows give (1, d), as np.atleast_2d does in space.bind
        flags = (_lib.SSN_BIND_INVERT_A if invert_a else 0) | (_lib.SSN_BIND_INVERT_B if invert_b else 0) | (_lib.SSN_BIND_NORMALIZE if normalize else 0)
        if into is None and out == "host" and not (op_a.on_device or op_b.on_device) and op_a.code == op_b.code == _lib.SSN_F64:
            res = np.empty((n, d), dtype=np.float64)
            self._check(self._lib.ssn_binder_bind(self._h, op_a.ptr, op_a.n, op_b.ptr, op_b.n, n, flags, float(norm_floor), res.ctypes.data))
            return res.reshape(lead + (d,))
        res, ld = service.result(self, n, d, into)
        self._check(self._lib.ssn_binder_bind_device(self._h, *op_a, *op_b, n, flags, float(norm_floor), res.data_ptr() if n else None, ld))
        if into is not None:
            return into
        return service.finish(res.reshape(lead + (d,)), out)
