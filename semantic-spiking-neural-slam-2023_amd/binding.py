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
import ctypes as C

import numpy as np

from . import _lib
from . import frontend as fe

__all__ = ["SSPBinder", "BACKENDS", "backend_dtype"]

# bind backends of SSPSpace.bind / SPSpace.bind and the harness: None is the NumPy path
BACKENDS = {None: None, "numpy": None, "hip": "f32", "hip-f32": "f32", "hip-f64": "f64"}


def backend_dtype(backend):
    """dtype of the SSPBinder behind a backend name, None for the NumPy path; ValueError for an unknown name."""
    try:
        return BACKENDS[backend]
    except (KeyError, TypeError):
        raise ValueError(f"unknown bind backend {backend!r}: one of None, 'numpy', 'hip', 'hip-f64'") from None


def _is_tensor(x):
    return hasattr(x, "is_cuda") and hasattr(x, "data_ptr")


class SSPBinder:
    """Circular convolution of rows, on the GPU.

    ``SSPBinder(d_or_space, dtype="f32", device=0, scratch_bytes=None)``: the width, or a space to take it from (``ssp_dim`` of an
    ``SSPSpace``, ``dim`` of an ``SPSpace``).  ``scratch_bytes``: size of the device work area (default 64 MB); a smaller one only
    means more chunks, never another bit.
    """

    def __init__(self, d_or_space, dtype="f32", device=0, scratch_bytes=None):
        if dtype not in ("f32", "f64"):
            raise ValueError(f"dtype must be 'f32' or 'f64', got {dtype!r}")
        d = getattr(d_or_space, "ssp_dim", None)
        if d is None:
            d = getattr(d_or_space, "dim", d_or_space)
        if isinstance(d, bool) or not isinstance(d, (int, np.integer)):
            raise ValueError(f"SSPBinder needs a width or a space, got {d_or_space!r}")
        self.width, self.dtype, self.device = int(d), dtype, int(device)
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.closed = True
        rc = self._lib.ssn_binder_create(_lib.SSN_F32 if dtype == "f32" else _lib.SSN_F64, self.device, self.width, int(scratch_bytes or 0),
                                         C.byref(self._h))
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
            self._lib.ssn_binder_destroy(self._h)
            self.closed = True

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self, n=0):
        """How a call with ``n`` output rows is cut (row_chunk, n_chunks), the scratch sizes, the planned route (transform_length,
        bluestein_m, radices, threads, lds_bytes) and the launches / device milliseconds of the last call, as a dict."""
        if self.closed:
            raise fe.SimulationError("the binder is closed")
        out = _lib.BinderInfo()
        self._check(self._lib.ssn_binder_get_info(self._h, int(n), C.byref(out)))
        res = {name: getattr(out, name) for name, _ in _lib.BinderInfo._fields_}
        res["radices"] = tuple(int(r) for r in out.radices[:out.n_radices])
        return res

    def _operand(self, x, what):
        """(kept array, lead shape, (pointer, on_device, dtype code, leading dimension, rows)): a host operand as a C-contiguous
        float32 / float64 array, a device tensor as it is when its rows are evenly spaced."""
        d = self.width
        tensor = _is_tensor(x)
        if tensor and not x.is_cuda:
            x, tensor = x.detach().numpy(), False
        if tensor:
            import torch
            if x.device.index != self.device:
                raise ValueError(f"{what} lives on {x.device}, the binder on device {self.device}")
            x = x.detach()
            if x.dtype not in (torch.float32, torch.float64):
                x = x.to(torch.float64)
            if x.dim() not in (1, 2, 3) or x.shape[-1] != d:
                raise ValueError(f"{what} must be ({d},), (N, {d}) or (S, L, {d}), got {tuple(x.shape)}")
            lead = tuple(int(s) for s in x.shape[:-1])
            if x.dim() == 3:
                x = x.reshape(-1, d) if x.is_contiguous() else x.contiguous().reshape(-1, d)
            elif x.dim() == 1:
                x = x[None, :]
            n = int(x.shape[0])
            if x.stride(1) != 1 or (n > 1 and x.stride(0) < d):
                x = x.contiguous()
            ld = max(int(x.stride(0)), d) if n > 1 else d
            torch.cuda.current_stream(x.device).synchronize()          # the rows are complete before the binder's stream reads them
            return x, lead, (x.data_ptr() if n else None, 1, _lib.SSN_F32 if x.dtype == torch.float32 else _lib.SSN_F64, ld, n)
        x = np.asarray(x)
        if x.ndim not in (1, 2, 3) or x.shape[-1] != d:
            raise ValueError(f"{what} must be ({d},), (N, {d}) or (S, L, {d}), got {x.shape}")
        lead = x.shape[:-1]
        x = np.ascontiguousarray(x.reshape(-1, d), dtype=np.float32 if x.dtype == np.float32 else np.float64)
        n = int(x.shape[0])
        return x, lead, (x.ctypes.data if n else None, 0, _lib.SSN_F32 if x.dtype == np.float32 else _lib.SSN_F64, d, n)

    def bind(self, a, b, invert_a=False, invert_b=False, normalize=False, norm_floor=1e-8, out="host", into=None):
        """``a (*) b`` row by row.  ``a``, ``b``: array-likes or torch tensors on the binder's device (float32 / float64, any row
        stride, read in place), shaped ``(d,)``, ``(N, d)`` or ``(S, L, d)``; the operand with fewer rows is paired with the other's
        rows as 1 : n or as one row per group of ``n / count`` consecutive rows - ``(S, d)`` with ``(S, L, d)`` gives ``(S, L, d)``.
        ``invert_a`` / ``invert_b``: that operand is read at ``(d - i) mod d`` (``space.invert``).  ``normalize``: every output row
        over ``max(norm, norm_floor)``.  ``out="host"``: a float64 array; ``out="device"``: a torch tensor of the binder's dtype.
        ``into``: a caller's 2-D device tensor of the binder's dtype (any row stride) whose ``[:n, :d]`` receives the rows -
        nothing else of it is touched; it is returned."""
        if self.closed:
            raise fe.SimulationError("the binder is closed")
        if out not in ("host", "device"):
            raise ValueError(f"out must be 'host' or 'device', got {out!r}")
        d = self.width
        a, lead_a, (pa, a_dev, a_code, a_ld, a_n) = self._operand(a, "a")
        b, lead_b, (pb, b_dev, b_code, b_ld, b_n) = self._operand(b, "b")
        n = max(a_n, b_n)
        for what, cnt in (("a", a_n), ("b", b_n)):
            if n and (cnt == 0 or n % cnt):
                raise ValueError(f"{cnt} rows of {what} do not pair with {n} output rows (1, n, or a divisor of n)")
        if a_n != b_n:
            lead = lead_a if a_n > b_n else lead_b
        else:
            lead = lead_a if len(lead_a) >= len(lead_b) else lead_b
        lead = tuple(lead) or (1,)          # two single rows give (1, d), as np.atleast_2d does in space.bind
        flags = (_lib.SSN_BIND_INVERT_A if invert_a else 0) | (_lib.SSN_BIND_INVERT_B if invert_b else 0) | (_lib.SSN_BIND_NORMALIZE if normalize else 0)
        if into is None and out == "host" and not a_dev and not b_dev and a_code == _lib.SSN_F64 and b_code == _lib.SSN_F64:
            res = np.empty((n, d), dtype=np.float64)
            self._check(self._lib.ssn_binder_bind(self._h, pa, a_n, pb, b_n, n, flags, float(norm_floor), res.ctypes.data))
            return res.reshape(lead + (d,))
        import torch
        tdtype = torch.float32 if self.dtype == "f32" else torch.float64
        if into is not None:
            if not _is_tensor(into) or not into.is_cuda or into.device.index != self.device or into.dtype != tdtype:
                raise ValueError(f"into must be a {tdtype} tensor on cuda:{self.device}")
            if into.dim() != 2 or into.shape[0] < n or into.shape[1] < d or into.stride(1) != 1 or (into.shape[0] > 1 and into.stride(0) < d):
                raise ValueError(f"into must be 2-D with at least ({n}, {d}) entries and unit column stride, got {tuple(into.shape)}")
            res, ld = into, (int(into.stride(0)) if into.shape[0] > 1 else d)
        else:
            res, ld = torch.empty((n, d), dtype=tdtype, device=f"cuda:{self.device}"), d
        torch.cuda.current_stream(res.device).synchronize()
        self._check(self._lib.ssn_binder_bind_device(self._h, pa, a_dev, a_code, a_ld, a_n, pb, b_dev, b_code, b_ld, b_n, n, flags, float(norm_floor),
                                                     res.data_ptr() if n else None, ld))
        if into is not None:
            return into
        res = res.reshape(lead + (d,))
        return res if out == "device" else res.cpu().to(torch.float64).numpy()
