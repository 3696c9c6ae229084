"""TEST INFRASTRUCTURE.  A NumPy restatement of regenie's two-stage rank-inverse-normal transformation of the Step-2 residuals (`--apply-rerint` =
RN-Resid-Unadj, `--apply-rerint-cov` = RN-Resid-Adj of Sofer et al. 2020), written from reading Data::compute_res / residualize_res (Data.cpp:2386-2436)
and rint_pheno (Pheno.cpp:1975-2011) -- independent of the driver and of the HIP library:
  res = (Y - LOCO prediction) * mask
  per trait, over its observed samples: sort the values; a run of m equal values that starts at sorted position i (0-based) gets the rank
  (i + 1) + (m - 1) / 2; value <- Phi^-1((rank - kc) / (nvals - 2 kc + 1)) with kc = 3 / 8 (Blom's constant; the denominator is nvals + 1 / 4)
  --apply-rerint-cov: beta = res^T X, res -= (X beta^T) * mask
  res *= mask; scale_Y = |res_p| / sqrt(Neff_p - ncov), 1 for a dropped trait, an error below numtol; res /= scale_Y
  then compute_res goes on as ever: p_sd_yres = |res_p| / sqrt(Neff_p - ncov), res /= p_sd_yres, scf_sv = scale_Y * p_sd_yres.
The quantile is the standard library's statistics.NormalDist().inv_cdf."""
import gzip
import os

from statistics import NormalDist

import numpy as np

from tests import rerint_cases as rc

KC = 3.0 / 8.0
NUMTOL = 1e-6
_inv_cdf = np.frompyfunc(NormalDist().inv_cdf, 1, 1)


def ndtri(u):
    """The standard-normal quantile of the standard library (AS241), elementwise."""
    return _inv_cdf(np.asarray(u, dtype=np.float64)).astype(np.float64)


def ranks_with_ties(v):
    """rint_pheno's ranks of a vector: 1-based, a block of ties shares the mean of its positions."""
    v = np.asarray(v, dtype=np.float64)
    order = np.argsort(v, kind="stable")
    s = v[order]
    start = np.concatenate([[True], s[1:] != s[:-1]])
    first = np.flatnonzero(start)                       # first sorted position of each block
    length = np.diff(np.concatenate([first, [len(s)]]))
    block = np.cumsum(start) - 1
    r = np.empty(len(s))
    r[order] = (first[block] + 1) + (length[block] - 1) / 2.0
    return r


def rint(v, quantile=ndtri):
    r = ranks_with_ties(v)
    return quantile((r - KC) / (len(v) - 2 * KC + 1)), r


def residualize_res(res, X, mask, ncov, mode, pheno_pass=None, quantile=ndtri):
    """res [n][P] masked residuals, X [n][C] orthonormal, mask [n][P] 0 / 1.  mode 1: --apply-rerint, 2: --apply-rerint-cov.
    -> res (scaled by scale_Y), scale_Y [P], ranks [n][P] (0 = unobserved)."""
    res = np.array(res, dtype=np.float64)
    mask = np.asarray(mask, dtype=np.float64)
    ranks = np.zeros_like(res)
    for p in range(res.shape[1]):
        m = mask[:, p] != 0
        res[m, p], ranks[m, p] = rint(res[m, p], quantile)
    if mode == 2:
        beta = res.T @ X
        res = res - (X @ beta.T) * mask
    res = res * mask
    scale_Y = np.sqrt((res ** 2).sum(axis=0)) / np.sqrt(mask.sum(axis=0) - ncov)
    if pheno_pass is not None:
        scale_Y = np.where(np.asarray(pheno_pass) != 0, scale_Y, 1.0)
    if scale_Y.min() < NUMTOL:
        raise ValueError("some phenotype residuals has sd=0.")
    return res / scale_Y, scale_Y, ranks


def transform(res0, X, mask, mode, pheno_pass=None, quantile=ndtri):
    """The whole of compute_res after the masking, from res0 = (Y - LOCO prediction) * mask.  -> dict res, scf_sv, scale_Y, ranks."""
    mask = np.asarray(mask, dtype=np.float64)
    ncov = X.shape[1]
    res, scale_Y, ranks = residualize_res(res0, X, mask, ncov, mode, pheno_pass, quantile)
    p_sd = np.sqrt((res ** 2).sum(axis=0)) / np.sqrt(mask.sum(axis=0) - ncov)
    return {"res": res / p_sd, "scf_sv": scale_Y * p_sd, "scale_Y": scale_Y, "ranks": ranks}


def case_arrays(name, tmp):
    """The plain arrays of a case of tests/rerint_cases.py RESTATED: genotypes of chromosome 2 [M][n] (NaN = missing), covariate basis X [n][C], the
    masked residuals Y - LOCO prediction [n][P], masks [n][P], and the reading of check_sparse_G's rule the input format takes."""
    from oracle import regenie_step1 as s1
    rc.write_inputs(tmp)
    a = rc.args_of(name, tmp)
    val = lambda k, d="": a[a.index(k) + 1] if k in a else d      # noqa: E731
    opt = s1.Step1Options(bed=os.path.join(rc.EX, "example_3chr"), pheno_file=val("--phenoFile"), covar_file=val("--covarFile"),
                          cat_covar=tuple(val("--catCovarList").split(",")) if "--catCovarList" in a else (), test_mode=True)
    prep = s1.read_pheno_and_cov(opt, s1.read_fam(opt.bed + ".fam"))
    cond = []
    if "--condition-list" in a:      # extract_condition_snps (Pheno.cpp:952-983): the listed variants, in ascending id order, mean-imputed, join the raw
        from tests.ld_cases import read_bed      # covariates before the basis is formed; they leave the tested set like excluded ones
        cond = sorted(set(ln.split()[0] for ln in open(val("--condition-list")) if ln.split()))
        Gc, vid, _, _, _ = read_bed(opt.bed)
        cols = np.array([Gc[list(vid).index(v)] for v in cond])
        cols = np.where(np.isnan(cols), np.nanmean(cols, axis=1, keepdims=True), cols)
        prep.X = np.column_stack([prep.X, cols.T])
    s1.prep_run(prep, opt)
    blup = np.zeros_like(prep.Y)
    for k, ln in enumerate(open(val("--pred")).read().splitlines()):
        lines = open(ln.split()[1]).read().splitlines()
        col = {s: i for i, s in enumerate(lines[0].split()[1:])}
        row = [t.split() for t in lines[1:] if t.split()[0] == "2"][0][1:]
        blup[:, k] = [float(row[col[s]]) for s in prep.ids]
    mask = prep.mask.astype(np.float64)
    res0 = (prep.Y - blup * mask) * mask
    zero_count_rule = False
    if "--bgen" in a:
        from oracle.bgen import BgenOracle
        b = BgenOracle(val("--bgen"))
        G = np.array([b.dosages(j) for j, v in enumerate(b.variants) if v["chrom"].lstrip("0") == "2"])
        G = np.where(G == -3.0, np.nan, G)
    else:      # the .pgen of the cases holds the hard calls of the .bed
        from tests.ld_cases import read_bed
        G, vid, chrom, _, _ = read_bed(opt.bed)
        G = G[np.array([str(c) == "2" and v not in cond for c, v in zip(chrom, vid)])]
        zero_count_rule = "--pgen" in a
    return G, prep.X, res0, mask, zero_count_rule


def restate_case(name):
    """-> per trait a dict of arrays over the case's 400 variants: beta, se, chisq, logp (what regenie prints as BETA SE CHISQ LOG10P)."""
    import tempfile
    from oracle import regenie_step2_qt as s2o
    with tempfile.TemporaryDirectory() as tmp:
        G, X, res0, mask, zero_count_rule = case_arrays(name, tmp)
    t = transform(res0, X, mask, rc.mode_of(name))
    if "--mcc" in rc.CASES[name]:
        from tests import mcc_restate as mr
        out = mr.mcc_block(G, X, t["res"], mask, t["scf_sv"])
    else:
        out = s2o.score_qt_block_ref(G, X, t["res"], mask, t["scf_sv"], zero_count_rule=zero_count_rule)
        out["beta"] = out["bhat"]
        out["logp"] = np.array([[s2o.get_logp(c) for c in row] for row in out["chisq"]])
    return [{k: out[k][:, p] for k in ("beta", "se", "chisq", "logp")} for p in range(res0.shape[1])]


def differing_rows(name):
    """Rows of the case's files in which one of BETA SE CHISQ LOG10P, printed with six significant digits as regenie prints them, is not the
    restatement's."""
    res = restate_case(name)
    differ = 0
    for k in (1, 2):
        rows = [ln.split(" ") for ln in gzip.open(os.path.join(rc.REF, name, "out_Y%d.regenie.gz" % k), "rt").read().splitlines()]
        c = [rows[0].index(h) for h in ("BETA", "SE", "CHISQ", "LOG10P")]
        for j, r in enumerate(rows[1:]):
            differ += any("%g" % res[k - 1][key][j] != r[ci] for key, ci in zip(("beta", "se", "chisq", "logp"), c))
    return differ


def golden_columns(name, k):
    rows = [ln.split(" ") for ln in gzip.open(os.path.join(rc.REF, name, "out_Y%d.regenie.gz" % k), "rt").read().splitlines()]
    c = {h: i for i, h in enumerate(rows[0])}
    return {h: np.array([float(r[c[h]]) for r in rows[1:]]) for h in ("BETA", "SE", "CHISQ", "LOG10P")}
