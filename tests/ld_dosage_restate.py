"""Data::compute_ld_dosages + the dense Data::print_ld (reference src/Data.cpp:3887-3980, :4092-4203) restated on integer dosages.

Gi [n][M] uint16 in units of 1 / scale over the analysed samples, MISSING = 0xFFFF (a forced-in column is all zero), X [n][C] the
orthonormal covariate basis.  float64: the dense products of tests/ld_restate.py on Gi / scale.  longdouble: the integer sums
A = g0^T g0, B = g0^T miss, D = miss^T miss as float64 BLAS products while they stay below 2^53 (asserted), the division by scale
and everything that is not an integer in longdouble."""
import numpy as np

from tests import ld_restate as lr

MISSING = 0xFFFF


def ints(Gi):
    """g0 (0 at a missing entry) and the indicator, as integers held in float64."""
    Gi = np.asarray(Gi)
    m = Gi == MISSING
    return np.where(m, 0, Gi).astype(np.float64), m.astype(np.float64)


def exact_product(a, b):
    """a^T b for integer-valued float64 arrays [n][.]: exact when the bound on every sum is below 2^53."""
    assert float(np.abs(a).max(initial=0)) * float(np.abs(b).max(initial=0)) * a.shape[0] < 2.0 ** 53
    return a.T @ b


def to_float(Gi, scale):
    """Genotype units in float64, NaN at a missing entry: what the reference holds in Gblock.Gmat."""
    Gi = np.asarray(Gi)
    return np.where(Gi == MISSING, np.nan, Gi.astype(np.float64) / scale)


def ld_cov(Gi, scale, X, dtype=np.float64):
    if dtype is np.float64 or dtype == np.float64:
        return lr.ld_cov(to_float(Gi, scale), X)
    g0, m = ints(Gi)
    s = dtype(scale)
    nobs = (m == 0).sum(axis=0)
    tot = g0.sum(axis=0)                      # integers below 2^53
    mean = np.where(nobs > 0, tot.astype(dtype) / (s * np.maximum(nobs, 1).astype(dtype)), dtype(0))
    Xl = np.asarray(X, dtype=dtype)
    gx = np.empty((g0.shape[1], Xl.shape[1]), dtype=dtype)
    for c in range(Xl.shape[1]):
        xc = Xl[:, c]
        gx[:, c] = (g0.astype(dtype) * xc[:, None]).sum(axis=0) / s + mean * (m.astype(dtype) * xc[:, None]).sum(axis=0)
    A = exact_product(g0, g0).astype(dtype) / (s * s)
    B = exact_product(g0, m).astype(dtype) / s
    D = exact_product(m, m).astype(dtype)
    gtg = A + mean[None, :] * B + mean[:, None] * B.T + (mean[:, None] * mean[None, :]) * D
    return gtg - gx @ gx.T


def corr_of(LD, dtype=np.float64, tol=lr.TOL, numtol=lr.NUMTOL):
    """print_ld's diagonal rules and scaling (the steps of ld_restate.ld_corr) on a covariance."""
    LD = np.array(LD, dtype=dtype)
    d = np.diag(LD).copy()
    z = (d < 0) & (np.abs(d) < tol)
    LD[z, :] = 0
    LD[:, z] = 0
    d = np.diag(LD)
    sds = np.where(d <= 0, np.sqrt(dtype(numtol)), np.sqrt(np.where(d <= 0, 1, d)))
    LD[np.diag_indices_from(LD)] = sds * sds
    return (1 / sds)[:, None] * LD * (1 / sds)[None, :]


def ld_corr(Gi, scale, X, dtype=np.float64):
    return corr_of(ld_cov(Gi, scale, X, dtype), dtype)
