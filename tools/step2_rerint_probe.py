#!/usr/bin/env python
"""Step 2, `--apply-rerint` / `--apply-rerint-cov`: time of rg_s2_qt_rerint alone (regenie_amd/csrc/step2_rerint.hip) at n samples, P traits, C covariates
-- device time of its kernels (hipEvents on the library's stream) and the wall time of the call with scale_Y / scf_sv alone coming back, as the driver
calls it -- next to the same transformation on the host: the NumPy restatement (tests/rerint_restate.py) on one thread and with one trait per thread on 16, checked against the device's
result (SciPy's quantile there: the restatement's own, the standard library's, is a Python call per value).  Usage (GPU box): python tools/step2_rerint_probe.py [n [P [C]]]      (default 500000 10 5)"""
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from scipy.special import ndtri
import torch  # noqa: F401  (its HIP runtime comes up first: tests/conftest.py)

from regenie_amd import step2
from tests import rerint_restate as rr


def main(n=500_000, P=10, C=5):
    torch.cuda.init()
    rng = np.random.default_rng(1)
    X = np.linalg.qr(np.column_stack([np.ones(n), rng.normal(size=(n, C - 1))]))[0]
    mask = (rng.random((n, P)) > 0.05).astype(np.uint8)
    res0 = rng.standard_gamma(2.0, size=(n, P)) * mask
    Xt, rt, mt = (np.ascontiguousarray(a.T) for a in (X, res0, mask))
    with step2.Step2QT(n, C, P) as s2:
        for mode, name in ((step2.RERINT, "--apply-rerint"), (step2.RERINT_COV, "--apply-rerint-cov")):
            kern, wall = [], []
            sy, sv = np.zeros(P), np.zeros(P)
            out = step2._RerintOut(sy.ctypes.data, sv.ctypes.data, None, None)
            for _ in range(6):
                s2.set_null(Xt, rt, mt, np.zeros(P))
                t0 = time.perf_counter()
                s2._check(s2.lib.rg_s2_qt_rerint(s2.h, mode, None, 1e-6, ctypes.byref(out)))
                wall.append(1e3 * (time.perf_counter() - t0))
                kern.append(s2.lib.rg_s2_last_kernel_ms(s2.h))
            s2.set_null(Xt, rt, mt, np.zeros(P))
            got = s2.rerint(mode)
            t0 = time.perf_counter()
            want = rr.transform(res0, X, mask, mode, quantile=ndtri)
            host = 1e3 * (time.perf_counter() - t0)
            t0 = time.perf_counter()      # the same, one trait per host thread, 16 threads (NumPy's sort and elementwise loops run outside the interpreter lock)
            with ThreadPoolExecutor(16) as ex:
                cols = list(ex.map(lambda p: rr.transform(res0[:, p:p + 1], X, mask[:, p:p + 1], mode, quantile=ndtri), range(P)))
            host16 = 1e3 * (time.perf_counter() - t0)
            assert all(np.abs(c["res"][:, 0] - want["res"][:, p]).max() <= 1e-12 * np.abs(want["res"][:, p]).max() for p, c in enumerate(cols))
            dev = float(np.max(np.abs(got["res"] - want["res"].T) / np.abs(want["res"]).max(axis=0)[:, None]))
            print("%s n=%d P=%d C=%d: kernels %.3f ms (runs %s), call %.3f ms (runs %s) | NumPy restatement on the host %.0f ms on one thread, %.0f ms with a trait per thread on 16 | ranks equal: %s, "
                  "max deviation of the residuals %.3g of the largest" % (name, n, P, C, float(np.median(kern[1:])), " ".join("%.3f" % v for v in kern[1:]),
                                                                         float(np.median(wall[1:])), " ".join("%.3f" % v for v in wall[1:]), host, host16,
                                                                         bool(np.array_equal(got["ranks"], want["ranks"].T)), dev), flush=True)


if __name__ == "__main__":
    main(*(int(v) for v in sys.argv[1:4]))
