"""Data::print_ld (reference src/Data.cpp:4368-4449) restated on dense numpy arrays, in float64 or numpy.longdouble.

G [n][M] hard calls over the analysed samples (NaN = missing; a forced-in column is all zero), X [n][C] the orthonormal
covariate basis (intercept included).  tests/test_ld_restate_cpu.py holds it to the reference's own output files."""
import numpy as np

TOL, NUMTOL, MULT = 1e-8, 1e-6, 65535.0


def covar_basis(cov, n):
    """new_cov as getBasis leaves it (Pheno.cpp:1660-1681): an orthonormal basis of [1, covariates]."""
    Xr = np.ones((n, 1)) if cov is None else np.column_stack([np.ones(n), cov])
    d, V = np.linalg.eigh(Xr.T @ Xr)
    keep = d > d.max() * 1e-15
    return Xr @ (V[:, keep] / np.sqrt(d[keep]))


def mean_impute(G, dtype=np.float64):
    G = np.array(G, dtype=dtype)
    miss = np.isnan(G)
    nobs = (~miss).sum(axis=0)
    tot = np.where(miss, 0, G).sum(axis=0)
    mean = np.where(nobs > 0, tot / np.maximum(nobs, 1), 0)
    return np.where(miss, mean[None, :], G)


def _gtx(Gi, X, dtype):
    return Gi.T @ np.asarray(X, dtype=dtype)


def ld_cov(G, X, dtype=np.float64, Gb=None):
    """G^T G - (G^T X)(G^T X)^T of the mean-imputed calls (Gb given: the block G against Gb).  float64: the dense products as written
    in print_ld.  longdouble: the same sums with the integer part taken exactly -- sum g_i g_j = A + m_j B_ij + m_i B_ji + m_i m_j D with
    A = g0^T g0, B = g0^T miss, D = miss^T miss, which are integers below 2^53 and therefore exact as float64 BLAS products -- and
    everything that is not an integer (the means, the combination, G^T X and its product) in longdouble: numpy has no fast longdouble
    matrix product, and this one is closer to the true value than a dense longdouble product would be."""
    if dtype is np.float64 or dtype == np.float64:
        Ga_i = mean_impute(G)
        Gb_i = Ga_i if Gb is None else mean_impute(Gb)
        return Ga_i.T @ Gb_i - _gtx(Ga_i, X, np.float64) @ _gtx(Gb_i, X, np.float64).T

    def parts(H):
        H = np.asarray(H, dtype=np.float64)
        m = np.isnan(H)
        g0 = np.where(m, 0.0, H)
        nobs = (~m).sum(axis=0)
        mean = np.where(nobs > 0, g0.sum(axis=0).astype(dtype) / np.maximum(nobs, 1).astype(dtype), dtype(0))
        Xl = np.asarray(X, dtype=dtype)
        # G^T X in longdouble: per covariate column, sum over samples of (g0 + mean * miss) * x
        gx = np.empty((H.shape[1], Xl.shape[1]), dtype=dtype)
        for c in range(Xl.shape[1]):
            xc = Xl[:, c]
            gx[:, c] = (g0.astype(dtype) * xc[:, None]).sum(axis=0) + mean * (m.astype(dtype) * xc[:, None]).sum(axis=0)
        return g0, m.astype(np.float64), mean, gx

    a = parts(G)
    b = a if Gb is None else parts(Gb)
    A, B, Bt, D = (a[0].T @ b[0]).astype(dtype), (a[0].T @ b[1]).astype(dtype), (a[1].T @ b[0]).astype(dtype), (a[1].T @ b[1]).astype(dtype)
    gtg = A + b[2][None, :] * B + a[2][:, None] * Bt + (a[2][:, None] * b[2][None, :]) * D
    return gtg - a[3] @ b[3].T


def ld_corr(G, X, dtype=np.float64, tol=TOL, numtol=NUMTOL):
    LD = ld_cov(G, X, dtype)
    d = np.diag(LD).copy()
    z = (d < 0) & (np.abs(d) < tol)
    LD[z, :] = 0
    LD[:, z] = 0
    d = np.diag(LD)
    sds = np.where(d <= 0, np.sqrt(dtype(numtol)), np.sqrt(np.where(d <= 0, 1, d)))
    LD[np.diag_indices_from(LD)] = sds * sds
    return (1 / sds)[:, None] * LD * (1 / sds)[None, :]


def quantise(R):
    """The body of the binary .corr: r * r * 65535 + 0.5 truncated, row-major over i < j; also the un-truncated values."""
    iu = np.triu_indices(R.shape[0], 1)
    r = np.asarray(R[iu], dtype=np.float64)
    v = r * r * MULT + 0.5
    return np.minimum(v, MULT).astype(np.uint16), v


def read_corr_bin(path_or_bytes):
    raw = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, "rb").read()
    hdr = np.frombuffer(raw[:8], dtype=np.int32)
    return int(hdr[0]), int(hdr[1]), np.frombuffer(raw[8:], dtype=np.uint16)


def check_binary(got_u16, ref_u16, v_restate, band=1e-6, max_band=3):
    """The issue's rule: equal, except where the fp64 restatement puts r^2 * 65535 + 0.5 within `band` of an integer; those may differ by
    exactly 1, and at most `max_band` of them.  Returns the number let through."""
    got = np.asarray(got_u16, dtype=np.int64)
    ref = np.asarray(ref_u16, dtype=np.int64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    diff = np.nonzero(got != ref)[0]
    near = np.abs(v_restate - np.rint(v_restate)) < band
    bad = [k for k in diff if not (near[k] and abs(got[k] - ref[k]) == 1)]
    print("binary R^2: %d values, %d differ, %d of them inside the %.0e band" % (got.size, diff.size, diff.size - len(bad), band))
    assert not bad, "values differ outside the rounding band: first at %d (got %d, reference %d)" % (bad[0], got[bad[0]], ref[bad[0]])
    assert diff.size <= max_band, "%d values let through the band" % diff.size
    return int(diff.size)


def check_text(got_text, ref_text):
    """Six printed digits: |a - b| <= 1e-5 |b| + 1e-12 per number and the same shape; reports the byte-identical lines."""
    gl, rl = got_text.rstrip("\n").split("\n"), ref_text.rstrip("\n").split("\n")
    assert len(gl) == len(rl), (len(gl), len(rl))
    same = sum(a == b for a, b in zip(gl, rl))
    a = np.array([[float(t) for t in ln.split()] for ln in gl])
    b = np.array([[float(t) for t in ln.split()] for ln in rl])
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.abs(a - b) - (1e-5 * np.abs(b) + 1e-12)
    print("text corr: %d of %d lines byte-identical, worst excess over the bound %.3g" % (same, len(rl), err.max()))
    assert err.max() <= 0, "entry %s: got %r, reference %r" % (np.unravel_index(err.argmax(), err.shape), a.flat[err.argmax()], b.flat[err.argmax()])
    return same
