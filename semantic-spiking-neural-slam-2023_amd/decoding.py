"""Grid decoding of SSP trajectories on the device: ``SSPSpace.decode(rows, 'from-set', 'grid', n)`` as one HIP call.

Every experiment of the reference ends with ``ssp_space.decode(sim.data[probe], 'from-set', 'grid', n)``
(``run_pathint.py:171-179``, ``run_slam.py:242-268``, ``run_slamview.py:167-192``): a ``(n^dim x d) . (d x T)`` product and an
argmax per row.  ``GridDecoder`` holds the sample table on the GPU and runs that as a product on the f32 matrix cores whose epilogue
keeps only each row's best column (``csrc/ssn_decode.hip`` behind ``ssn_decoder_*`` of ``include/ssn.h``); the ``T x n^dim``
similarity matrix never exists.  There is no CPU fallback: without a GPU the constructor raises.

    with GridDecoder(space, 100) as dec:
        est = dec.decode(sim.data[probe])              # == space.decode(sim.data[probe], 'from-set', 'grid', 100)

``SSPSpace.decode(..., backend="hip")`` does the same through a decoder cached on the space.  Where the similarities themselves are
wanted - the maps the reference's figure scripts draw - ``GridDecoder.similarity`` keeps them (``k_decode_map``):

        sims = dec.similarity(sim.data[probe], power=2)    # == (sim.data[probe] @ sample_ssps.T) ** 2, (T, n_samples)
"""
import functools

import numpy as np

from . import _lib, service
from .service import BACKENDS

__all__ = ["GridDecoder", "BACKENDS", "backend_dtype"]

backend_dtype = functools.partial(service.backend_dtype, what="decode")      # (backend) -> the GridDecoder's dtype, None: NumPy


class GridDecoder(service.DeviceService):
    """Best sample per row, on the GPU.

    ``GridDecoder(ssp_space, num_samples, sampling_method)`` takes its table from ``ssp_space.get_sample_pts_and_ssps``;
    ``GridDecoder(samples=(sample_ssps, sample_points))`` takes it as ``SSPSpace.decode(samples=...)`` does (with ``ssp_space`` only
    needed for ``clean_up``).  ``dtype``: "f32" (matrix cores; the index agrees with the float64 host answer wherever the two best
    similarities differ by more than the f32 error of the product) or "f64" (parity mode).  ``scratch_bytes``: size of the device
    work area (default 64 MB); a smaller one only means more row chunks and fewer column strips, never another answer.
    ``table``: "host" (the default) encodes the sample table on the host and uploads it; "device" takes only
    ``ssp_space.get_sample_points`` and has a float64 ``ssn_encoder`` make the table on the GPU, chunk by chunk, straight into the
    decoder's dtype (``ssn_decoder_create_from_points``) - the table never exists on the host.  Beside ``samples=``
    it is a ValueError: the caller already holds the SSPs.

    Rows are scaled as the host scales them (divided by their norm when it is >= 1e-6).  Non-finite rows are out of contract: their
    index is some value inside ``[0, n_samples)``.
    """

    noun, destroy = "decoder", "ssn_decoder_destroy"

    def __init__(self, ssp_space=None, num_samples=100, sampling_method="grid", samples=None, dtype="f32", device=0,
                 scratch_bytes=None, trust=None, table="host"):
        super().__init__(dtype, device)
        if table not in ("host", "device"):
            raise ValueError(f"table must be 'host' or 'device', got {table!r}")
        if table == "device" and samples is not None:
            raise ValueError("table='device' makes the table from the space's sample points; with samples= the caller already holds the SSPs")
        if samples is None and ssp_space is None:
            raise ValueError("GridDecoder needs an ssp_space or samples=(sample_ssps, sample_points)")
        self.ssp_space = ssp_space
        self.table_source = table
        self._encoder = None          # the SSPEncoder of clean_up(encode="device"), made on first use
        # the box of refine(): the pitch of the space's own grid, or trust= beside samples=
        self._grid = (num_samples, sampling_method) if samples is None else None
        self._trust, self._refine_key = trust, None
        if table == "device":
            from .encoding import tables
            pts = np.ascontiguousarray(ssp_space.get_sample_points(num_samples, sampling_method), dtype=np.float64)
            K, M, w = tables(ssp_space)
            self.sample_points, self.n_samples, self.width = pts, int(pts.shape[0]), int(ssp_space.ssp_dim)
            self._create("ssn_decoder_create_from_points", pts.ctypes.data, self.n_samples, self.width, K, int(ssp_space.domain_dim),
                         M.ctypes.data, w.ctypes.data, int(scratch_bytes or 0), 0)
            return
        if samples is None:
            sample_ssps, sample_points = ssp_space.get_sample_pts_and_ssps(num_samples, sampling_method)
        else:
            sample_ssps, sample_points = samples
        table = np.ascontiguousarray(np.asarray(sample_ssps, dtype=np.float64))
        if table.ndim != 2:
            raise ValueError(f"sample_ssps must be (n_samples, width), got shape {table.shape}")
        self.sample_points, self.n_samples, self.width = np.asarray(sample_points), int(table.shape[0]), int(table.shape[1])
        self._create("ssn_decoder_create", table.ctypes.data, self.n_samples, self.width, int(scratch_bytes or 0))

    def close(self):
        enc = self.__dict__.pop("_encoder", None)
        if enc is not None:
            enc.close()
        super().close()

    def info(self, n_rows=0):
        """How a call with ``n_rows`` rows is cut (row_chunk, n_chunks, n_strips, tiles_per_strip), the scratch sizes, and the
        launches / device milliseconds of the last call, as a dict."""
        return self._info(_lib.DecoderInfo, "ssn_decoder_get_info", n_rows)

    # -- decoding ------------------------------------------------------------------------------
    def _rows(self, rows):
        """``service.rows_operand`` for rows of the decoder's width; host rows as float64, what ``ssn_decoder_rows`` takes."""
        return service.rows_operand(rows, self.width, "rows", self.device, who="decoder", keep_f32=False, count="T")

    def indices(self, rows, return_sims=False):
        """Index of the best sample of every row (int64, lowest index on ties); with ``return_sims`` also the similarity of the
        scaled row to it.  ``rows``: array-like ``(T, width)`` (or one row), or a torch tensor on the decoder's device (float32 /
        float64, any row stride), which is read in place."""
        self._open()
        rows, _, op = self._rows(rows)
        best = np.empty(op.n, dtype=np.int32)
        sims = np.empty(op.n, dtype=np.float64) if return_sims else None
        sims_p = sims.ctypes.data if return_sims else None
        if op.on_device:
            self._check(self._lib.ssn_decoder_rows_device(self._h, op.ptr, op.code, op.ld, op.n, best.ctypes.data, sims_p))
        else:
            self._check(self._lib.ssn_decoder_rows(self._h, rows.ctypes.data, op.n, best.ctypes.data, sims_p))
        best = best.astype(np.int64)
        return (best, sims) if return_sims else best

    def set_map_stage(self, nbytes=0):
        """Size of the device + pinned staging of host maps (0: the default, 64 MB or one tile of doubles); at least one 128-row
        tile, ``128 * n_samples`` values.  Never changes a result."""
        self._open()
        self._check(self._lib.ssn_decoder_set_map_stage(self._h, int(nbytes)))

    def similarity(self, rows, power=1, normalize=False, out="host", out_dtype=None, into=None):
        """The ``(T, n_samples)`` similarity map ``(rows @ table.T) ** power`` (``k_decode_map``): the values
        ``indices`` compares, kept.  ``rows`` as ``indices`` takes them; ``normalize=True`` scales them as ``decode`` does (a row of
        norm below 1e-6 stays as it is), the default uses them raw like the reference's figure scripts.  ``power``: 1 or 2 (the
        square is one multiply in the decoder's dtype).  ``out="host"`` returns float64 NumPy (``out_dtype="f32"``: float32, from an
        f32 decoder - half the copy); ``out="device"`` a torch tensor in the decoder's dtype; ``into=`` a caller's 2-D device tensor
        of that dtype, ``(T, n_samples)`` with unit column stride and any row stride >= n_samples, written in place (nothing outside
        ``[:T, :n_samples]`` is touched) and returned.  With ``normalize=True, power=1`` the argmax of a row is ``indices(rows)``."""
        self._open()
        if power not in (1, 2) or isinstance(power, bool):
            raise ValueError(f"power must be 1 or 2, got {power!r}")
        service.check_out(out)
        if out_dtype not in (None, "f32", "f64"):
            raise ValueError(f"out_dtype must be None, 'f32' or 'f64', got {out_dtype!r}")
        if out_dtype == "f32" and self.dtype == "f64":
            raise ValueError("out_dtype='f32' from an f64 decoder is not offered: the map is never narrowed")
        if (out == "device" or into is not None) and out_dtype not in (None, self.dtype):
            raise ValueError(f"a device map has the decoder's dtype {self.dtype!r}, not out_dtype={out_dtype!r}")
        rows, _, op = self._rows(rows)
        n = op.n
        flags = (_lib.SSN_MAP_NORMALIZE if normalize else 0) | (_lib.SSN_MAP_SQUARE if power == 2 else 0)
        rows_args = (op.ptr, 1, op.code, op.ld) if op.on_device else (rows.ctypes.data, 0, 0, self.width)
        if out == "host" and into is None:
            dt = out_dtype or "f64"
            res = np.empty((n, self.n_samples), dtype=np.float32 if dt == "f32" else np.float64)
            self._check(self._lib.ssn_decoder_map(self._h, *rows_args, n, flags, res.ctypes.data, 0, service.CODE[dt], self.n_samples))
            return res
        into, ld = service.result(self, n, self.n_samples, into, exact=True)
        self._check(self._lib.ssn_decoder_map(self._h, *rows_args, n, flags, into.data_ptr() if n else None, 1, service.CODE[self.dtype], ld))
        return into

    def _set_refine(self, trust=None):
        """Build and upload the refinement tables on first use (again when ``trust`` changes)."""
        space = self.ssp_space
        if space is None:
            raise ValueError("refine needs the decoder's ssp_space (its phase matrix and length scale)")
        if space.ssp_dim != self.width or self.sample_points.ndim != 2 or self.sample_points.shape != (self.n_samples, space.domain_dim):
            raise ValueError(f"refine needs samples of the decoder's ssp_space: ({self.n_samples}, {space.ssp_dim}) SSPs with "
                             f"({self.n_samples}, {space.domain_dim}) points, got width {self.width} and points {self.sample_points.shape}")
        if space.domain_dim > 3:
            raise ValueError(f"refine supports domain_dim 1, 2 and 3, not domain_dim {space.domain_dim}")
        trust = self._trust if trust is None else trust
        if trust is None and self._grid is None:
            raise ValueError("refine on a decoder made with samples= needs trust=: the half width of the box around the best sample")
        key = ("grid",) if trust is None else tuple(np.atleast_1d(np.asarray(trust, dtype=float)).tolist())
        if key == self._refine_key:
            return
        lo, hi, pitch = space.refine_box(*(self._grid or (None, None)), trust=trust)
        K, M, w = space.refine_tables()
        d = self.width
        W = np.exp(-2j * np.pi * np.outer(np.arange(K), np.arange(d)) / d)
        dft = np.empty((2 * K, d))
        dft[0::2], dft[1::2] = W.real, W.imag
        pts = np.ascontiguousarray(self.sample_points, dtype=np.float64)
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (dft, M, w, pts, lo, hi, pitch)]
        self._check(self._lib.ssn_decoder_set_refine(self._h, arrs[0].ctypes.data, K, arrs[1].ctypes.data, arrs[2].ctypes.data, space.domain_dim,
                                                     arrs[3].ctypes.data, arrs[4].ctypes.data, arrs[5].ctypes.data, arrs[6].ctypes.data))
        self._refine_key = key

    def refine(self, rows, iterations=8, return_info=False, trust=None):
        """The grid decode followed by ``iterations`` safeguarded Newton steps per row on ``<encode(x), row>`` inside the box
        ``x0 +- pitch`` (``k_decode_refine``): ``(T, dim)`` float64 points; with ``return_info`` also ``f`` (the
        similarity at x), ``status`` (bit 1: on a box face, 2: Hessian not negative definite at x, 4: last step above
        1e-6 pitch) and ``best`` (the grid index).  Rows as ``indices`` takes them.  ``iterations=0`` is the grid decode."""
        self._open()
        iterations = int(iterations)
        if iterations < 0:
            raise ValueError(f"iterations must be >= 0, got {iterations}")
        self._set_refine(trust)
        rows, _, op = self._rows(rows)
        n, dim = op.n, self.sample_points.shape[1]
        x = np.empty((n, dim), dtype=np.float64)
        best, f, status = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float64), np.empty(n, dtype=np.int32)
        out = (x.ctypes.data, best.ctypes.data, f.ctypes.data, status.ctypes.data)
        if op.on_device:
            self._check(self._lib.ssn_decoder_refine_rows_device(self._h, op.ptr, op.code, op.ld, n, iterations, *out))
        else:
            self._check(self._lib.ssn_decoder_refine_rows(self._h, rows.ctypes.data, n, iterations, *out))
        return (x, f, status, best.astype(np.int64)) if return_info else x

    def indices_composed(self, rows):
        """Measurement aid (tools/bench_decode.py): the same indices from the composition this decoder replaces - the similarity
        matrix written out by ``k_gemm_nt_mfma_f32``, then ``k_argmax_partial`` over it.  f32, host rows, one chunk, at most 2 GB
        of similarities; ``info()["last_kernel_ms"]`` is its device time afterwards."""
        self._open()
        rows, _, op = self._rows(np.asarray(rows, dtype=np.float64))
        best = np.empty(op.n, dtype=np.int32)
        self._check(self._lib.ssn_decoder_rows_composed(self._h, rows.ctypes.data, op.n, best.ctypes.data))
        return best.astype(np.int64)

    def decode(self, rows, return_sims=False, refine=False, iterations=8):
        """``sample_points[best]``: what ``SSPSpace.decode(rows, 'from-set', ..., samples=...)`` returns.  ``refine=True`` is
        shorthand for ``refine(rows, iterations)``."""
        if refine:
            return self.refine(rows, iterations)
        if return_sims:
            best, sims = self.indices(rows, True)
            return self.sample_points[best], sims
        return self.sample_points[self.indices(rows)]

    def clean_up(self, rows, refine=False, encode="host", out="host", iterations=8):
        """The SSPs of the decoded (``refine=True``: refined) points: ``ssp_space.encode(decode(rows))``.  ``encode``: "host" is the
        space's float64 NumPy transform; "device" / "hip" encode the points with an ``SSPEncoder`` of the decoder's dtype on the
        decoder's device, and ``out="device"`` then leaves the rows there as a torch tensor."""
        if self.ssp_space is None:
            raise ValueError("clean_up needs the decoder's ssp_space")
        if encode not in ("host", "device", "hip"):
            raise ValueError(f"encode must be 'host', 'device' or 'hip', got {encode!r}")
        service.check_out(out)
        if encode == "host" and out == "device":
            raise ValueError("out='device' needs encode='device': the host encode returns a NumPy array")
        points = self.decode(rows, refine=refine, iterations=iterations)
        if encode == "host":
            return self.ssp_space.encode(points)
        self._open()
        if self._encoder is None:
            from .encoding import SSPEncoder
            self._encoder = SSPEncoder(self.ssp_space, dtype=self.dtype, device=self.device)
        return self._encoder.encode(points, out=out)
