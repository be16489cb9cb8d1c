"""What the device services - ``GridDecoder``, ``SSPEncoder``, ``SSPBinder`` - share on the Python side: the backend
names, the life cycle of an ABI handle, the marshalling of row operands, the device result and the caches a space keeps of them.
``csrc/ssn_service.hpp`` is the C++ half.  Not part of the package's public names.
"""
import collections
import ctypes as C
import math

import numpy as np

from . import _lib
from . import frontend as fe

# backends of SSPSpace.decode / encode / bind, clean_up and the harness: None is the NumPy path
BACKENDS = {None: None, "numpy": None, "hip": "f32", "hip-f32": "f32", "hip-f64": "f64"}
CODE = {"f32": _lib.SSN_F32, "f64": _lib.SSN_F64}


def backend_dtype(backend, what):
    """dtype of the service behind a backend name, None for the NumPy path; ValueError ("unknown <what> backend") for an unknown name."""
    try:
        return BACKENDS[backend]
    except (KeyError, TypeError):
        raise ValueError(f"unknown {what} backend {backend!r}: one of None, 'numpy', 'hip', 'hip-f64'") from None


def check_out(out):
    if out not in ("host", "device"):
        raise ValueError(f"out must be 'host' or 'device', got {out!r}")


class DeviceService:
    """A handle of the C ABI with a dtype and a device: made by ``_create``, destroyed once by ``close`` (or the ``with`` block, or
    the collector).  Subclasses name their ``noun`` ("the <noun> is closed") and the ABI's ``destroy`` function."""
    noun = "service"
    destroy = None

    def __init__(self, dtype, device):
        if dtype not in ("f32", "f64"):
            raise ValueError(f"dtype must be 'f32' or 'f64', got {dtype!r}")
        self.dtype, self.device = dtype, int(device)
        self._lib, self._h = None, C.c_void_p()
        self.closed = True          # until _create succeeds: a constructor that raised leaves nothing to destroy

    def _create(self, fn_name, *args):
        """The ABI call ``fn_name(dtype code, device, *args, handle)``; a non-zero status is a BuildError."""
        self._lib = _lib.load()
        rc = getattr(self._lib, fn_name)(CODE[self.dtype], self.device, *args, C.byref(self._h))
        if rc != 0:
            raise fe.BuildError(f"{_lib.STATUS.get(rc, rc)}: {_lib.last_error()}")
        self.closed = False

    def _check(self, rc):
        if rc != 0:
            raise fe.SimulationError(f"{_lib.STATUS.get(rc, rc)}: {_lib.last_error()}")

    def _open(self):
        if self.closed:
            raise fe.SimulationError(f"the {self.noun} is closed")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if not self.closed:
            getattr(self._lib, self.destroy)(self._h)
            self.closed = True

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _info(self, struct, fn_name, n):
        """The service's ``*_get_info`` struct for a call with ``n`` rows, as a dict."""
        self._open()
        out = struct()
        self._check(getattr(self._lib, fn_name)(self._h, int(n), C.byref(out)))
        return {name: getattr(out, name) for name, _ in struct._fields_}


# what the ABI's *_device entries take for a block of rows: pointer (None without rows), host / device, dtype code, leading
# dimension in elements, rows
Operand = collections.namedtuple("Operand", "ptr on_device code ld n")


def rows_operand(x, width, what, device, *, who, ndim=(1, 2), keep_f32=True, count="N"):
    """Rows of ``width`` values for the service ``who`` ("decoder", ...) on ``device`` -> ``(kept, lead_shape, Operand)``.

    ``x``: a host array-like, a CPU tensor (host data), or a torch tensor on ``device``, with one of the ranks ``ndim`` - one row,
    ``(N, width)``, or ``(S, L, width)`` flattened to ``S L`` rows; ``lead_shape`` is its shape without the last axis.  Anything
    but float32 / float64 is widened to float64, and so is host float32 without ``keep_f32`` (for an entry point that takes
    doubles).  Host rows arrive as a C-contiguous array.  A device tensor is read in place when it has unit column stride and a row
    stride >= ``width`` - the leading dimension - and through a contiguous copy otherwise; the caller's current stream is
    synchronised, so the rows are complete before the service's stream reads them.  ``kept`` holds the memory behind the pointer
    and must outlive the call.  ``what`` / ``count`` name the operand and its row count in the errors."""
    tensor = hasattr(x, "is_cuda") and hasattr(x, "data_ptr")
    if tensor and not x.is_cuda:
        x, tensor = x.detach().numpy(), False
    if tensor:
        import torch
        if x.device.index != device:
            raise ValueError(f"{what} {'live' if what.endswith('s') else 'lives'} on {x.device}, the {who} on device {device}")
        x = x.detach()
        if x.dtype not in (torch.float32, torch.float64):
            x = x.to(torch.float64)
    else:
        x = np.asarray(x)
    shape = tuple(x.shape)
    if len(shape) not in ndim or shape[-1] != width:
        forms = f"({width},), (N, {width}) or (S, L, {width})" if 3 in ndim else f"({count}, {width})"
        raise ValueError(f"{what} must be {forms}, got {shape}")
    lead = shape[:-1]
    n = math.prod(lead)
    if not tensor:
        x = np.ascontiguousarray(x.reshape(n, width), dtype=np.float32 if keep_f32 and x.dtype == np.float32 else np.float64)
        return x, lead, Operand(x.ctypes.data if n else None, 0, _lib.SSN_F32 if x.dtype == np.float32 else _lib.SSN_F64, width, n)
    if len(shape) != 2:
        x = x.reshape(n, width)          # (a view when the rows are evenly spaced, a copy otherwise)
    row_stride, col_stride = x.stride()
    if col_stride != 1 or (n > 1 and row_stride < width):
        x, row_stride = x.contiguous(), width
    torch.cuda.current_stream(x.device).synchronize()
    return x, lead, Operand(x.data_ptr() if n else None, 1, _lib.SSN_F32 if x.dtype == torch.float32 else _lib.SSN_F64,
                            row_stride if n > 1 else width, n)


def result(service, n, width, into=None, exact=False):
    """The device tensor a call writes ``(n, width)`` values of the service's dtype into, and its leading dimension: a new one, or
    the caller's ``into`` - 2-D on the service's device, unit column stride, ``exact``: shaped ``(n, width)`` with any row stride
    >= width; otherwise at least that large, only ``[:n, :width]`` being written.  The caller's current stream is synchronised:
    whatever filled or freed that memory is complete before the service's stream writes."""
    import torch
    tdt = torch.float32 if service.dtype == "f32" else torch.float64
    if into is None:
        res, ld = torch.empty((n, width), dtype=tdt, device=f"cuda:{service.device}"), width
    else:
        on_device = hasattr(into, "is_cuda") and hasattr(into, "data_ptr") and into.is_cuda and into.device.index == service.device
        strided = on_device and into.dim() == 2 and (into.stride(1) != 1 or (into.shape[0] > 1 and into.stride(0) < width))
        if exact:
            if not on_device:
                raise ValueError(f"into= must be a tensor on the {service.noun}'s device {service.device}")
            if into.dtype != tdt:
                raise ValueError(f"into= must be {tdt}, the {service.noun}'s dtype, got {into.dtype}")
            if tuple(into.shape) != (n, width):
                raise ValueError(f"into= must be ({n}, {width}), got {tuple(into.shape)}")
            if strided:
                raise ValueError(f"into= needs unit column stride and a row stride >= {width}, got strides {tuple(into.stride())}")
        else:
            if not on_device or into.dtype != tdt:
                raise ValueError(f"into must be a {tdt} tensor on cuda:{service.device}")
            if into.dim() != 2 or into.shape[0] < n or into.shape[1] < width or strided:
                raise ValueError(f"into must be 2-D with at least ({n}, {width}) entries and unit column stride, got {tuple(into.shape)}")
        res, ld = into, (int(into.stride(0)) if into.shape[0] > 1 else width)
    torch.cuda.current_stream(res.device).synchronize()
    return res, ld


def finish(res, out):
    """A device result as the caller asked for it: the tensor itself, or a float64 NumPy array."""
    if out == "device":
        return res
    import torch
    return res.cpu().to(torch.float64).numpy()


class ServiceCache:
    """The device services a space keeps for its ``backend="hip"`` calls: a plain dict per kind in the space's ``__dict__``
    (``_decoder_cache``, ``_encoder_cache``, ``_binder_cache``), absent until first use.  They hold device handles, so they stay
    with the object they were made for (``strip`` in ``__getstate__``) and are closed when the space changes (``drop_all``)."""
    KINDS = ("decoder", "encoder", "binder")

    def __init__(self, owner, kind, single=False):
        self.owner, self.name, self.single = owner.__dict__, f"_{kind}_cache", single

    def get(self, key, make):
        """The service under ``key``, made by ``make()`` on first use; ``single``: the others are closed first (one at a time)."""
        cache = self.owner.get(self.name, {})
        if key not in cache:
            if self.single:
                self.drop()
            service = make()
            cache = self.owner.setdefault(self.name, {})
            cache[key] = service
        return cache[key]

    def drop(self):
        for service in self.owner.pop(self.name, {}).values():
            service.close()

    @classmethod
    def drop_all(cls, owner):
        for kind in cls.KINDS:
            cls(owner, kind).drop()

    @classmethod
    def strip(cls, state):
        """``state`` (a copy of a ``__dict__``) without the caches."""
        for kind in cls.KINDS:
            state.pop(f"_{kind}_cache", None)
        return state
