"""The level-0 leave-one-out predictors of one block (reference src/Data.cpp:755-767 + src/Step1_Models.cpp:615-726), restated in plain
NumPy with the number format as a parameter, and the cases the leave-one-out kernel tests sweep (tests/test_loocv_restate_cpu.py,
tests/test_loocv_tri_gpu.py draw the same inputs from here).

The reference diagonalises A = G G^T once and serves every ridge value from the eigenvectors; the device reduces A to tridiagonal form
(regenie_amd/csrc/loocv_tri.hip).  This file does neither: per ridge value it factors A + lambda I = L L^T with a hand-written Cholesky
(np.linalg has no extended precision), and
    h_i = |L^-1 g_i|^2,   num_ip = (L^-1 g_i) . (L^-1 G Y_p),   W_ip = (num_ip - h_i y_ip) / (1 - h_i),
then the mask / centre / re-mask / scale standardisation (Step1_Models.cpp:693-704).  Run in np.longdouble (x87 extended: 64-bit mantissa,
eps 1.1e-19) from the raw imputed calls on -- mean imputation, residualisation on the covariate basis and scaling included -- it is the
yardstick; run in float64 it is a second fp64 route beside the oracle's eigendecomposition.

The covariate basis X and the phenotypes Y are inputs (what the device is handed): they are taken as given, converted exactly."""
from __future__ import annotations

import types

import numpy as np

LD = np.longdouble


def have_extended_precision() -> bool:
    return np.finfo(LD).eps < 1e-18


def cholesky(M):
    """Lower Cholesky factor of a symmetric positive definite matrix in M's own dtype: a column loop, rows vectorised."""
    n = M.shape[0]
    L = np.zeros_like(M)
    for j in range(n):
        v = M[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            raise np.linalg.LinAlgError("not positive definite at column %d" % j)
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return L


def forward(L, B):
    """L^-1 B for lower-triangular L (row loop, columns of B vectorised)."""
    Z = np.empty_like(B)
    for k in range(L.shape[0]):
        Z[k] = (B[k] - L[k, :k] @ Z[:k]) / L[k, k]
    return Z


def backward_t(L, B):
    """L^-T B."""
    Z = np.empty_like(B)
    for k in range(L.shape[0] - 1, -1, -1):
        Z[k] = (B[k] - L[k + 1:, k] @ Z[k + 1:]) / L[k, k]
    return Z


def standardise_genotypes(raw, ain, X, n_analyzed, dtype):
    """raw: (bs, N) calls or dosages as float64 with -3 for missing (samples the run ignores already dropped, --ref-first already applied).
    Geno.cpp:1702-1769 (mean over the analysed non-missing samples, missing -> mean, samples not analysed -> 0) and Data.cpp:190-224
    (residualise on the basis X, scale by norm / sqrt(n_analyzed - C)), all in `dtype`.  Returns (G~ (bs, N), scale (bs,))."""
    miss = raw == -3
    g = raw.astype(dtype)
    ok = (~miss) & ain[None, :]
    mu = np.where(ok, g, dtype(0)).sum(axis=1) / ok.sum(axis=1).astype(dtype)
    g = np.where(miss, mu[:, None], g)
    g = np.where(ain[None, :], g, dtype(0))
    Xd = X.astype(dtype)
    g = g - (g @ Xd) @ Xd.T
    scale = np.sqrt((g * g).sum(axis=1)) / np.sqrt(dtype(n_analyzed - X.shape[1]))
    return g / scale[:, None], scale


def level0_raw(G, Y, lam, dtype, omit=None):
    """The predictors before standardisation, (P, N, R0), and the leverages h (N, R0).  omit="tail": the terms k >= (bs & ~3) of both sums
    over the factor's rows are dropped -- what a recurrence kernel that walks k four at a time computes when its tail loop is lost."""
    G = G.astype(dtype)
    Y = Y.astype(dtype)
    bs, N = G.shape
    P = Y.shape[1]
    A = G @ G.T
    B = G @ Y
    W = np.zeros((P, N, len(lam)), dtype)
    H = np.zeros((N, len(lam)), dtype)
    keep = bs & ~3 if omit == "tail" else bs
    for r, l in enumerate(lam):
        L = cholesky(A + dtype(l) * np.eye(bs, dtype=dtype))
        Z = forward(L, G)[:keep]
        U = forward(L, B)[:keep]
        h = (Z * Z).sum(axis=0)
        num = Z.T @ U
        with np.errstate(invalid="ignore", divide="ignore"):
            W[:, :, r] = ((num - h[:, None] * Y) / (dtype(1) - h)[:, None]).T
        H[:, r] = h
    return W, H


def standardise_predictors(W, mask, neff, dtype):
    """Step1_Models.cpp:693-704 on (P, N, R0): mask, centre by the column sum over Neff, mask again, scale by norm / sqrt(Neff - 1)."""
    out = np.empty_like(W)
    for p in range(W.shape[0]):
        m = mask[:, p].astype(dtype)[:, None]
        Wp = W[p] * m
        mean = Wp.sum(axis=0) / dtype(neff[p])
        Wp = (Wp - mean[None, :]) * m
        sd = np.sqrt((Wp * Wp).sum(axis=0)) / np.sqrt(dtype(neff[p] - 1))
        with np.errstate(invalid="ignore", divide="ignore"):
            out[p] = Wp / sd[None, :]
    return out


def level0(raw, ain, X, Y, mask, neff, lam, n_analyzed, dtype=LD, omit=None):
    """ridge_level_0_loocv of one block from its raw calls.  Returns dict(W (P, N, R0) in `dtype`, h (N, R0), scale (bs,))."""
    G, scale = standardise_genotypes(raw, ain, X, n_analyzed, dtype)
    W, H = level0_raw(G, Y, lam, dtype, omit)
    return dict(W=standardise_predictors(W, mask, neff, dtype), h=H, scale=scale, G=G)


def brute_force_raw(G, Y, lam, dtype=LD):
    """Leave-one-out by its definition: for every sample i the ridge regression of Y on the block's SNPs is refitted WITHOUT sample i,
    beta = (A - g_i g_i^T + lambda I)^-1 (G Y - g_i y_i), and predicts sample i.  (P, N, R0), before standardisation."""
    G = G.astype(dtype)
    Y = Y.astype(dtype)
    bs, N = G.shape
    A = G @ G.T
    B = G @ Y
    W = np.zeros((Y.shape[1], N, len(lam)), dtype)
    for r, l in enumerate(lam):
        for i in range(N):
            gi = G[:, i]
            L = cholesky(A - np.outer(gi, gi) + dtype(l) * np.eye(bs, dtype=dtype))
            beta = backward_t(L, forward(L, B - np.outer(gi, Y[i])))
            W[:, i, r] = gi @ beta
    return W


def column_dev(W, ref):
    """max_i |W - ref| / max_i |ref| of every column, for (P, N, R0) arrays -> (P, R0) float64 (nan where W has a nan)."""
    W = np.asarray(W).astype(LD)
    d = np.abs(W - ref).max(axis=1) / np.abs(ref).max(axis=1)
    return d.astype(np.float64)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
# blocks: the block orders, all in ONE level-0 call; C counts the intercept; R0 = 1 means the single explicit ridge value h = 0.5.
CASES = [
    dict(id="order1", blocks=[1], N=129, P=1, R0=5, C=1),
    dict(id="orders2_3_1_5", blocks=[2, 3, 1, 5], N=129, P=2, R0=5, C=3),
    dict(id="slab_edges", blocks=[63, 64, 65], N=300, P=3, R0=8, C=3),
    dict(id="singular130_1_66", blocks=[130, 1, 66], N=257, P=5, R0=2, C=3, singular=True),
    dict(id="P6", blocks=[67, 4], N=300, P=6, R0=8, C=3),
    dict(id="P10", blocks=[67, 4], N=300, P=10, R0=8, C=3),
    dict(id="P11", blocks=[67, 4], N=300, P=11, R0=8, C=3),
    dict(id="C17", blocks=[65, 7], N=300, P=2, R0=1, C=17),
    dict(id="C33", blocks=[65, 7], N=300, P=2, R0=1, C=33),
    dict(id="more_snps_than_samples", blocks=[64], N=50, P=2, R0=5, C=3),
    dict(id="second_chunk", blocks=[5, 3], N=65536 + 193, P=6, R0=5, C=3),
    dict(id="bt_missing_removed_ref_first", blocks=[65, 33], N=1031, P=3, R0=5, C=5, binary=True, miss_pheno=0.04, miss_call=0.02,
         removed=37, ref_first=True),
    dict(id="dosages", blocks=[65, 7], N=300, P=3, R0=5, C=3, dosage=True, miss_call=0.005),
]
CASE_IDS = [c["id"] for c in CASES]
_BY_ID = {c["id"]: c for c in CASES}


def _ridge_values(R0, M):
    from oracle import regenie_step1 as orc
    h0 = np.array([0.5]) if R0 == 1 else orc.set_ridge_params(R0)
    return M * (1 - h0) / h0                      # Data.cpp:607


_problems = {}


def problem(case_id):
    """The inputs of a case, built once: prep (the oracle's Prepared: basis, residualised phenotypes, masks), rows (per block: packed .bed
    rows, or (bs, N) float64 dosages with -3 for missing), raw (per block: what standardise_genotypes takes), lam, blocks, ref_first, dosage."""
    if case_id in _problems:
        return _problems[case_id]
    from oracle import regenie_step1 as orc
    from tests.util import pack_bed
    c = _BY_ID[case_id]
    blocks, N, P, C = c["blocks"], c["N"], c["P"], c["C"]
    M = sum(blocks)
    rng = np.random.default_rng(1000 + CASE_IDS.index(case_id))
    # MAF from [0.2, 0.5] at N <= 300: no SNP comes near the low-variance check by chance
    maf = rng.uniform(0.2 if N <= 300 else 0.05, 0.5, (M, 1))
    g = rng.binomial(2, maf, (M, N)).astype(np.int8)
    if c.get("singular"):
        g[129] = g[0]                               # a copy
        g[65] = 2 - g[1]                            # the complement: -1 times SNP 1 once residualised on the intercept
    gs = g.astype(np.float64)
    gs = (gs - gs.mean(axis=1, keepdims=True)) / gs.std(axis=1, keepdims=True)
    if c.get("miss_call"):
        g[rng.random((M, N)) < c["miss_call"]] = -3
    cov = rng.standard_normal((N, C - 1))
    ncausal = min(M, 50)
    Y = np.empty((N, P))
    for p in range(P):
        idx = rng.choice(M, ncausal, replace=False)
        Y[:, p] = gs[idx].T @ (rng.standard_normal(ncausal) * np.sqrt(0.2 / ncausal)) + rng.standard_normal(N) * np.sqrt(0.8)
        if C > 1:
            Y[:, p] += 0.3 * cov[:, 0]
    if c.get("binary"):
        Y = (Y > np.quantile(Y, 0.7, axis=0, keepdims=True)).astype(np.float64)
    mask = np.ones((N, P), bool)
    if c.get("miss_pheno"):
        mask &= rng.random((N, P)) >= c["miss_pheno"]          # differs per trait
    ain = np.ones(N, bool)
    if c.get("removed"):
        ain[rng.choice(N, c["removed"], replace=False)] = False
    ain &= mask.any(axis=1)
    mask &= ain[:, None]
    X = np.column_stack([np.ones(N), cov]) * ain[:, None]
    prep = orc.Prepared(ids=["%d_%d" % (i + 1, i + 1) for i in range(N)], n_file=N, ind_ignore=np.zeros(N, bool), ind_in_analysis=ain,
                        pheno_names=["Y%d" % (p + 1) for p in range(P)], Y=Y * mask, Y_raw=None, mask=mask, X=X,
                        Neff=mask.sum(axis=0).astype(np.float64), scale_Y=np.ones(P), ncov=C, n_analyzed=int(ain.sum()),
                        pheno_pass=np.ones(P, bool))
    orc.prep_run(prep, orc.Step1Options())          # getBasis, residualise and scale the phenotypes
    assert prep.ncov == C
    starts = np.concatenate([[0], np.cumsum(blocks)])
    rows, raw = [], []
    for b, bs in enumerate(blocks):
        gb = g[starts[b]:starts[b] + bs]
        if c.get("dosage"):
            d = gb.astype(np.float64)
            soft = np.round(np.clip(d + rng.normal(0, 0.15, d.shape), 0, 2) * 255) / 255      # what an 8-bit BGEN stores
            d = np.where(gb == -3, -3.0, np.where(rng.random(d.shape) < 0.6, soft, d))
            rows.append(np.ascontiguousarray(d))
            raw.append(d)
        else:
            r = np.ascontiguousarray(pack_bed(gb))
            rows.append(r)
            d = orc.decode_bed_rows(r, N).astype(np.float64)
            raw.append(np.where(d == -3, d, 2 - d) if c.get("ref_first") else d)
    for a in rows + raw + [prep.X, prep.Y, prep.mask, prep.Neff, prep.ind_in_analysis]:
        a.setflags(write=False)
    pr = types.SimpleNamespace(case=c, prep=prep, rows=rows, raw=raw, lam=_ridge_values(c["R0"], M), blocks=list(blocks),
                               ref_first=bool(c.get("ref_first")), dosage=bool(c.get("dosage")))
    _problems[case_id] = pr
    return pr


def restated(pr, b, dtype=LD, omit=None):
    p = pr.prep
    return level0(pr.raw[b], p.ind_in_analysis, p.X, p.Y, p.mask, p.Neff, pr.lam, p.n_analyzed, dtype, omit)


def oracle_w(pr, b):
    """The block through the oracle's own route (eigendecomposition, fp64): (P, N, R0)."""
    from oracle import regenie_step1 as orc
    p = pr.prep
    if pr.dosage:
        G = orc.read_chunk_from_dosages(pr.rows[b], p.ind_ignore, p.ind_in_analysis)
    else:
        G = orc.read_chunk_from_bed(pr.rows[b], p.n_file, p.ind_ignore, p.ind_in_analysis, pr.ref_first)
    G, _ = orc.residualize_genotypes(G, p)
    return orc.ridge_level_0_loocv(G, p, pr.lam)


FLOOR = 1.04e-14      # tests/test_rerint_gpu.py's TOL: what two host fp64 routines for one function differ by, times ten
CAP = 1e-11           # no column's bound may exceed this
_refs = {}


def references(case_id):
    """Per block of a case, computed once and shared: W_ld (P, N, R0) long double; d_orc, d_f64 (P, R0): the per-column deviation of the
    oracle's eigen route and of this file's fp64 run from it; bound (P, R0) = 10 max(d_orc, d_f64, FLOOR) -- taken from the references
    alone; one_minus_h_min; scale_min."""
    if case_id in _refs:
        return _refs[case_id]
    if not have_extended_precision():
        raise RuntimeError("np.longdouble is no wider than float64 on this platform: no yardstick for the leave-one-out tests")
    pr = problem(case_id)
    out = []
    for b in range(len(pr.blocks)):
        ld = restated(pr, b, LD)
        d_orc = column_dev(oracle_w(pr, b), ld["W"])
        d_f64 = column_dev(restated(pr, b, np.float64)["W"], ld["W"])
        d64 = np.maximum(d_orc, d_f64)
        ld["W"].setflags(write=False)
        out.append(types.SimpleNamespace(W_ld=ld["W"], d_orc=d_orc, d_f64=d_f64, d64=d64, bound=10 * np.maximum(d64, FLOOR),
                                         one_minus_h_min=float((1 - ld["h"]).min()), scale_min=float(ld["scale"].min())))
    _refs[case_id] = out
    return out
