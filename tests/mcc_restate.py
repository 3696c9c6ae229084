"""TEST INFRASTRUCTURE.  A NumPy restatement of the moment-matched Step-2 test (`--qt --mcc --mcc-thr 1`) from plain arrays -- independent of
the driver and of the HIP library: the vector the test sees (raw mean-imputed genotype of a sparse variant, residualised and rescaled genotype
otherwise), the non-strict score statistic on it, the power sums of the two normalised vectors, the first three permutation moments of
D = cor^2, the gamma fit and the substitution of LOG10P and SE (compute_score_qt_mcc, Step2_Models.cpp:237-341; MCC::setup_y, MCCResults::dkat).
The moments are written here in the vectors' own terms (every sum formed from the normalised vectors, as the reference forms them), the driver
derives them from raw power sums by binomial expansion: two routes to the same numbers."""
import gzip
import math
import os

import numpy as np
from scipy import special as sp_special

from tests import mcc_cases as mc


def _gamma_q(a, x):
    return float(sp_special.gammaincc(a, x))


def _chi2_isf(p):
    return float(sp_special.chdtri(1.0, p))


def _third_moment(n, x, y):
    """E[D^3] under permutations; x, y: dicts of T = sum v^2, S2 = sum v^4, S3 = sum v^6, U = (sum v^3)^2 of the two normalised vectors."""
    T, S2, S3, U = y["T"], y["S2"], y["S3"], y["U"]
    Ts, S2s, S3s, Us = x["T"], x["S2"], x["S3"], x["U"]
    T2, T3, T2s, T3s = T * T, T ** 3, Ts * Ts, Ts ** 3
    R, Rs, B, Bs = T * S2, Ts * S2s, U, Us
    n2, n3, n4 = n * n, n ** 3, n ** 4
    t = [n2 * (n + 1) * (n2 + 15 * n - 4) * S3 * S3s,
         4 * (n4 - 8 * n3 + 19 * n2 - 4 * n - 16) * U * Us,
         24 * (n2 - n - 4) * (U * Bs + B * Us),
         6 * (n4 - 8 * n3 + 21 * n2 - 6 * n - 24) * B * Bs,
         12 * (n4 - n3 - 8 * n2 + 36 * n - 48) * R * Rs,
         12 * (n3 - 2 * n2 + 9 * n - 12) * (T * S2 * Rs + R * Ts * S2s),
         3 * (n4 - 4 * n3 - 2 * n2 + 9 * n - 12) * T * Ts * S2 * S2s,
         24 * ((n3 - 3 * n2 - 2 * n + 8) * (R * Us + U * Rs) + (n3 - 2 * n2 - 3 * n + 12) * (R * Bs + B * Rs)),
         12 * (n2 - n + 4) * (T * S2 * Us + U * Ts * S2s),
         6 * (2 * n3 - 7 * n2 - 3 * n + 12) * (T * S2 * Bs + B * Ts * S2s),
         -2 * n * (n - 1) * (n2 - n + 4) * ((2 * U + 3 * B) * S3s + (2 * Us + 3 * Bs) * S3),
         -3 * n * (n - 1) ** 2 * (n + 4) * ((T * S2 + 4 * R) * S3s + (Ts * S2s + 4 * Rs) * S3),
         2 * n * (n - 1) * (n - 2) * ((T3 + 6 * T * T2 + 8 * T3) * S3s + (T3s + 6 * Ts * T2s + 8 * T3s) * S3),
         T3 * ((n3 - 9 * n2 + 23 * n - 14) * T3s + 6 * (n - 4) * Ts * T2s + 8 * T3s),
         6 * T * T2 * ((n - 4) * T3s + (n3 - 9 * n2 + 24 * n - 14) * Ts * T2s + 4 * (n - 3) * T3s),
         8 * T3 * (T3s + 3 * (n - 3) * Ts * T2s + (n3 - 9 * n2 + 26 * n - 22) * T3s),
         -16 * (T3 * Us + U * T3s) - 6 * (T * T2 * Us + U * Ts * T2s) * (2 * n2 - 10 * n + 16),
         -8 * (T3 * Us + U * T3s) * (3 * n2 - 15 * n + 16) - (T3 * Bs + B * T3s) * (6 * n2 - 30 * n + 24),
         -6 * (T * T2 * Bs + B * Ts * T2s) * (4 * n2 - 20 * n + 24) - 8 * (T3 * Bs + B * T3s) * (3 * n2 - 15 * n + 24),
         -(n - 2) * (24 * (T3 * Rs + R * T3s) + 6 * (T * T2 * Rs + R * Ts * T2s) * (2 * n2 - 10 * n + 24)
                     + 8 * (T3 * Rs + R * T3s) * (3 * n2 - 15 * n + 24) + (3 * n2 - 15 * n + 6) * (T3 * Ts * S2s + T * S2 * T3s)
                     + 6 * (T * T2 * Ts * S2s + Ts * T2s * T * S2) * (n2 - 5 * n + 6) + 48 * (T3 * Ts * S2s + T3s * T * S2))]
    return sum(t) / (n * (n - 1) * (n - 2) * (n - 3) * (n - 4) * (n - 5))


def _side(v):
    return {"T": float((v ** 2).sum()), "S2": float((v ** 4).sum()), "S3": float((v ** 6).sum()), "U": float((v ** 3).sum()) ** 2}


def mcc_one(r, yres, mask, n_cov):
    """One (variant, trait): r the vector the test sees, yres the trait's scaled residual (0 where masked).  -> p, skewness of D."""
    m = mask.astype(bool)
    ni = float(m.sum()) - n_cov
    y = np.where(m, yres - yres[m].sum() / m.sum(), 0.0)
    y = y / np.linalg.norm(y)
    x = np.where(m, r - r[m].sum() / ni, 0.0)
    x = x / np.linalg.norm(x)
    D = float(x @ y) ** 2
    xs, ys = _side(x), _side(y)
    m1 = xs["T"] * ys["T"] / ni
    T2, T2s = ys["T"] ** 2, xs["T"] ** 2
    m2 = 2 * ((ni - 1) * T2 - T2) * ((ni - 1) * T2s - T2s) / ((ni - 1) ** 2 * (ni + 1) * (ni - 2)) \
        + (ni * (ni + 1) * ys["S2"] - (ni - 1) * 3 * T2) * (ni * (ni + 1) * xs["S2"] - (ni - 1) * 3 * T2s) / ((ni + 1) * ni * (ni - 1) * (ni - 2) * (ni - 3))
    skew = (_third_moment(ni, xs, ys) - 3 * m1 * m2 - m1 ** 3) / m2 ** 1.5
    if not skew > 0:
        return float("nan"), skew
    shape, scale, loc = 4 / skew ** 2, math.sqrt(m2) * skew / 2, m1 - 2 * math.sqrt(m2) / skew
    return (0.99999 if D - loc < 0 else _gamma_q(shape, (D - loc) / scale)), skew


def mcc_block(G, X, res, mask, scf_sv, n_samples=None):
    """G [M][n] (NaN or negative = missing), X [n][C] orthonormal, res / mask [n][P], scf_sv [P].  -> dict of [M][P] arrays: beta, se, chisq, logp, p, skew
    (NaN rows: ignored variants)."""
    from oracle import regenie_step2_qt as s2o
    M, n = G.shape
    P, C = res.shape[1], X.shape[1]
    out = {k: np.full((M, P), np.nan) for k in ("beta", "se", "chisq", "logp", "p", "skew")}
    for j in range(M):
        g, mean, nobs = s2o.mean_impute(G[j])
        if nobs == 0:
            continue
        if s2o.check_sparse(g, n_samples or n):
            r, sf = g, 1.0
        else:
            r, sf, ign = s2o.residualize_geno(X, g)
            if ign:
                continue
        for t in range(P):
            den = float((mask[:, t] * r * r).sum())
            st = float(res[:, t] @ r) / math.sqrt(den)
            bh = st * scf_sv[t] / (math.sqrt(den) * sf)
            p, skew = mcc_one(r, res[:, t], mask[:, t], C)
            out["beta"][j, t], out["chisq"][j, t], out["p"][j, t], out["skew"][j, t] = bh, st * st, p, skew
            out["logp"][j, t] = -math.log10(p)
            out["se"][j, t] = bh / st * math.sqrt(st * st / _chi2_isf(p))
    return out


def case_arrays(name, tmp):
    """The plain arrays of case (a) or (d): genotypes of chromosome 2, covariate basis, scaled LOCO residuals, masks."""
    from oracle import regenie_step1 as s1, regenie_step2_qt as s2o
    mc.write_inputs(tmp)
    opt = s1.Step1Options(bed=os.path.join(mc.EX, "example_3chr"), pheno_file=os.path.join(tmp, "pheno_skew.txt"),
                          covar_file=os.path.join(mc.EX, "covariates.txt"), test_mode=True)
    fam = s1.read_fam(opt.bed + ".fam")
    prep = s1.read_pheno_and_cov(opt, fam)
    s1.prep_run(prep, opt)
    blup = np.zeros_like(prep.Y)
    for k in (1, 2):
        lines = open(os.path.join(tmp, "ex_%d.loco" % k)).read().splitlines()
        col = {s: i for i, s in enumerate(lines[0].split()[1:])}
        row = [ln.split() for ln in lines[1:] if ln.split()[0] == "2"][0][1:]
        blup[:, k - 1] = [float(row[col[s]]) for s in prep.ids]
    mask = prep.mask.astype(np.float64)
    res, _, scf = s2o.compute_res(prep.Y, blup * mask, mask, prep.Neff, prep.ncov, prep.scale_Y)
    if name == "a_bed_all":
        from tests.ld_cases import read_bed
        G, ids, chrom, _, _ = read_bed(opt.bed)
        G = G[np.array([str(c) == "2" for c in chrom])]
    else:
        from oracle.bgen import BgenOracle
        b = BgenOracle(os.path.join(mc.EX, "example_3chr.bgen"))
        G = np.array([b.dosages(j) for j, v in enumerate(b.variants) if v["chrom"].lstrip("0") == "2"])
        G = np.where(G == -3.0, np.nan, G)
    return G, prep.X, res, mask, scf


def restate_case(name):
    """-> per trait a dict of arrays over the golden's rows (logp, se, p, skew)."""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        G, X, res, mask, scf = case_arrays(name, tmp)
    out = mcc_block(G, X, res, mask, scf)
    return [{k: v[:, t] for k, v in out.items()} for t in range(res.shape[1])]


def golden_columns(name, k):
    rows = [ln.split(" ") for ln in gzip.open(os.path.join(mc.REF, name, "out_Y%d.regenie.gz" % k), "rt").read().splitlines()]
    c = {h: i for i, h in enumerate(rows[0])}
    return {h: np.array([float(r[c[h]]) for r in rows[1:]]) for h in ("BETA", "SE", "CHISQ", "LOG10P")}
