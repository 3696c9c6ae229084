"""The Step-2 LD matrix of a region (`regenie --step 2 --compute-corr`, hard calls or integer dosages): ctypes wrapper over include/rg_ld.h
(regenie_amd/csrc/ld_corr.hip).  `append` is what Data::get_G_svs does per block (Data.cpp:4227-4304), `finish` is
Data::print_ld (Data.cpp:4368-4449).  No CPU path: without the HIP library or a GPU the constructor raises."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .engine import RgError, load_library

R2_U16, CORR_F64, COV_F64, GTG_F64 = 0, 1, 2, 3


def pack_bed_rows(G: np.ndarray) -> np.ndarray:
    """[bs][n] calls in {0, 1, 2}, missing = NaN or < 0 -> .bed-coded rows [bs][ceil(n / 4)] (00 -> 2, 01 -> missing, 10 -> 1, 11 -> 0)."""
    G = np.asarray(G, dtype=np.float64)
    bs, n = G.shape
    miss = np.isnan(G) | (G < 0)
    code = np.where(miss, 1, np.where(G == 2, 0, np.where(G == 1, 2, 3))).astype(np.uint8)
    code = np.concatenate([code, np.zeros((bs, (-n) % 4), np.uint8)], axis=1).reshape(bs, -1, 4)
    return (code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6)).astype(np.uint8)


class LDMatrix:
    TOL = 1e-8        # params.tol, Regenie.hpp:226
    NUMTOL = 1e-6     # params.numtol, Regenie.hpp:220

    def __init__(self, n: int, n_cov: int, n_col: int, device: int = 0):
        self.lib = load_library()
        self.h = C.c_void_p()
        self.n, self.C, self.M = int(n), int(n_cov), int(n_col)
        rc = self.lib.rg_ld_create(C.byref(self.h), int(device), self.n, self.C, self.M)
        if rc != 0:
            msg = self.lib.rg_ld_last_error(self.h).decode() if self.h else "rg_ld_create failed"
            self.close()
            raise RgError(rc, msg)

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.rg_ld_destroy(self.h)
        self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise RgError(rc, self.lib.rg_ld_last_error(self.h).decode())

    def set_basis(self, X: np.ndarray) -> None:
        """X [C][n]: the orthonormal covariate basis (new_cov^T, intercept included)."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.shape != (self.C, self.n):
            raise ValueError("set_basis: expected X %s" % ((self.C, self.n),))
        self._check(self.lib.rg_ld_set_basis(self.h, X.ctypes.data))

    def force_columns(self, cols) -> None:
        """Columns no variant fills (forced-in IDs that the genotype file does not have): zero vectors."""
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        self._check(self.lib.rg_ld_force_columns(self.h, cols.size, cols.ctypes.data))

    def append(self, rows, cols, flip: bool = False) -> None:
        """rows [bs][>= ceil(n / 4)] uint8 .bed-coded hard calls (numpy, or a CUDA torch tensor read in place); cols [bs]: the column
        of the matrix each row takes."""
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        on_device = 0
        if isinstance(rows, np.ndarray):
            rows = np.ascontiguousarray(rows, dtype=np.uint8)
            if rows.ndim != 2:
                raise ValueError("append: rows must be 2-d")
            bs, ld, ptr = rows.shape[0], rows.shape[1], rows.ctypes.data
        else:
            if not (rows.is_cuda and rows.element_size() == 1 and rows.dim() == 2 and rows.stride(1) == 1):
                raise ValueError("append: device rows must be a 2-d uint8 CUDA tensor with unit byte stride")
            bs, ld, ptr, on_device = rows.shape[0], rows.stride(0), rows.data_ptr(), 1
            import torch
            torch.cuda.current_stream(rows.device).synchronize()   # the library runs on its own stream
        if rows.shape[1] < (self.n + 3) // 4:
            raise ValueError("append: rows must hold ceil(n / 4) bytes")
        if cols.shape != (bs,):
            raise ValueError("append: one column index per row")
        self._check(self.lib.rg_ld_append(self.h, ptr, ld, bs, on_device, 1 if flip else 0, cols.ctypes.data))

    def append_int(self, rows_u16, cols, scale: int) -> None:
        """rows_u16 [bs][>= n] uint16 dosages in units of 1 / scale, 0xFFFF = missing (numpy, or a CUDA torch tensor of 2-byte
        elements read in place); cols [bs]: the column of the matrix each row takes."""
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        rows, on_device = rows_u16, 0
        if isinstance(rows, np.ndarray):
            rows = np.ascontiguousarray(rows, dtype=np.uint16)
            if rows.ndim != 2:
                raise ValueError("append_int: rows must be 2-d")
            bs, ld, ptr = rows.shape[0], rows.shape[1], rows.ctypes.data
        else:
            if not (rows.is_cuda and rows.element_size() == 2 and rows.dim() == 2 and rows.stride(1) == 1):
                raise ValueError("append_int: device rows must be a 2-d CUDA tensor of 2-byte elements with unit stride")
            bs, ld, ptr, on_device = rows.shape[0], rows.stride(0), rows.data_ptr(), 1
            import torch
            torch.cuda.current_stream(rows.device).synchronize()   # the library runs on its own stream
        if rows.shape[1] < self.n:
            raise ValueError("append_int: rows must hold n dosages")
        if cols.shape != (bs,):
            raise ValueError("append_int: one column index per row")
        self._check(self.lib.rg_ld_append_int(self.h, ptr, ld, bs, on_device, int(scale), cols.ctypes.data))

    def finish(self, form: int = CORR_F64, tol: float = TOL, numtol: float = NUMTOL) -> np.ndarray:
        """R2_U16 -> uint16 [M (M - 1) / 2] (the binary .corr body, quantised on the device); CORR_F64 / COV_F64 / GTG_F64 -> float64 [M][M]
        (GTG_F64: the unscaled matrix after print_ld's two diagonal rules, `--skip-scaleG`)."""
        M = self.M
        out = np.empty(M * (M - 1) // 2, np.uint16) if form == R2_U16 else np.empty((M, M), np.float64)
        self._check(self.lib.rg_ld_finish(self.h, int(form), out.ctypes.data if out.size else C.c_void_p(8), 0, float(tol), float(numtol)))
        return out

    def finish_sparse(self, thr: float, tol: float = TOL, numtol: float = NUMTOL):
        """`--skip-scaleG --sparse-thr thr` (Data.cpp:4407-4421), thresholded on the device: -> sd float64 [M] (sqrt of the diagonal of
        GTG_F64) and the triplets row, col (int32, 0-based, row < col) and val = LD[row][col] / sd[row] / sd[col] with |val| >= thr, in
        row-major order.  Only the triplets leave the device."""
        sd = np.empty(self.M, np.float64)
        count = C.c_int64(0)
        self._check(self.lib.rg_ld_finish_sparse(self.h, float(thr), float(tol), float(numtol), sd.ctypes.data, C.byref(count)))
        k = int(count.value)
        row, col, val = np.empty(k, np.int32), np.empty(k, np.int32), np.empty(k, np.float64)
        self._check(self.lib.rg_ld_sparse_fetch(self.h, row.ctypes.data, col.ctypes.data, val.ctypes.data))
        return sd, row, col, val

    def pair_sums(self, a0: int, na: int, b0: int, nb: int) -> dict:
        """Raw integer sums of rows [a0, a0 + na) against rows [b0, b0 + nb) in append order: A = g0 . g0, B = g0 . miss, Bt = miss . g0, D = miss . miss."""
        res = {k: np.empty((max(na, 0), max(nb, 0)), np.int32) for k in ("A", "B", "Bt", "D")}
        self._check(self.lib.rg_ld_pair_sums(self.h, int(a0), int(na), int(b0), int(nb), *[res[k].ctypes.data for k in ("A", "B", "Bt", "D")]))
        return res

    def pair_sums_int(self, a0: int, na: int, b0: int, nb: int) -> dict:
        """pair_sums for integer-dosage panels: int64 sums with g0 in integer units."""
        res = {k: np.empty((max(na, 0), max(nb, 0)), np.int64) for k in ("A", "B", "Bt", "D")}
        self._check(self.lib.rg_ld_pair_sums_int(self.h, int(a0), int(na), int(b0), int(nb), *[res[k].ctypes.data for k in ("A", "B", "Bt", "D")]))
        return res

    @property
    def kernel_ms(self) -> float:
        return self.lib.rg_ld_last_kernel_ms(self.h)

    @property
    def tiles(self) -> int:
        return self.lib.rg_ld_last_tiles(self.h)
