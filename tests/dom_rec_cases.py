"""The reference cases of the non-additive Step-2 tests (`--step 2 --test dominant|recessive [--minHOMs N]`): the command lines, the generator of
their inputs and a NumPy restatement of the quantitative-trait test on recoded hard calls -- one definition for
tests/golden/make_dom_rec_ref_outputs.py (which runs regenie itself) and for the tests (which run the driver and the library).
Data: the example's example_3chr (500 samples, chromosome 2 = 400 variants) as .bed, .bgen and -- written here -- a hard-call .pgen, with the LOCO
files regenie's Step 1 wrote for it (ref_outputs/qt_kfold_3chr: any prediction is a valid offset of Step 2); and a synthetic .bed of 500 samples x
400 variants with missing calls, phenotypes that differ in their missing values, rare variants, and five variants built to carry exactly
0, 1, MIN_HOMS - 1, MIN_HOMS and MIN_HOMS + 1 homozygotes of the counted allele."""
import gzip
import os

import numpy as np

from tests import condtl_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "tests", "golden", "example")
REF = os.path.join(ROOT, "tests", "golden", "ref_outputs", "dom_rec")
COND = ["inf_120", "inf_260", "inf_75"]
MIN_HOMS = 5
SYN = dict(M=400, N=500, P=2, seed=53, miss_rate=0.02, missing_pheno=0.1)
HOM_ROWS = {10: 0, 11: 1, 12: MIN_HOMS - 1, 13: MIN_HOMS, 14: MIN_HOMS + 1}      # variant row of the synthetic set -> homozygotes it carries


def synthetic_calls():
    """int8 (M, N), -3 missing: tests/util.py's HWE draws, the first 40 variants made rare, five rows with a fixed number of homozygotes."""
    from tests.util import synth_dosages, u01
    g = synth_dosages(SYN["M"], SYN["N"], miss_rate=SYN["miss_rate"], seed=SYN["seed"])
    j, i = np.arange(40)[:, None], np.arange(SYN["N"])[None, :]
    rare = (u01(700, j, i) < 0.02).astype(np.int8) + (u01(701, j, i) < 0.02).astype(np.int8)
    g[:40] = np.where(g[:40] == -3, np.int8(-3), rare)
    for row, nhom in HOM_ROWS.items():
        v = np.zeros(SYN["N"], np.int8)
        v[:nhom] = 2                     # the homozygotes
        v[20:60] = 1                     # 40 heterozygotes: the variant passes --minMAC whatever nhom is
        v[100:104] = -3                  # and has missing calls
        g[row] = v[np.random.default_rng(900 + row).permutation(SYN["N"])]
    return g


def write_inputs(d):
    """Writes every input the cases need into directory d; returns the synthetic calls."""
    from oracle import pgen as opg
    from tests.ld_cases import read_bed
    from tests.util import write_plink
    R = os.path.join(ROOT, "tests", "golden", "ref_outputs", "qt_kfold_3chr")
    with open(os.path.join(d, "pred_ex.list"), "w") as pl:
        for k in (1, 2):
            fn = os.path.join(d, "ex_%d.loco" % k)
            open(fn, "wb").write(gzip.open(os.path.join(R, "out_%d.loco.gz" % k), "rb").read())
            pl.write("Y%d %s\n" % (k, fn))
    with open(os.path.join(d, "cond.txt"), "w") as f:
        f.write("\n".join(COND) + "\n")
    rng = np.random.default_rng(19)
    fam = [ln.split()[:2] for ln in open(os.path.join(EX, "example_3chr.fam"))]
    with open(os.path.join(d, "ex_counts.txt"), "w") as f:
        f.write("FID IID Y1 Y2\n")
        for a, b in fam:
            f.write("%s %s %d %d\n" % (a, b, rng.poisson(2.0), rng.poisson(0.7)))
    # the hard calls of example_3chr as a .pgen (ALT = the first .bim allele, which .bed counts)
    G, vid, _, _, fam3 = read_bed(os.path.join(EX, "example_3chr"))
    bim = [ln.split() for ln in open(os.path.join(EX, "example_3chr.bim"))]
    T = os.path.join(d, "ex3")
    opg.write_pgen_fixed(T + ".pgen", np.where(np.isnan(G), 3, G).astype(np.uint8))
    with open(T + ".pvar", "w") as f:
        f.write("#CHROM\tPOS\tID\tREF\tALT\n")
        for t in bim:
            f.write("%s\t%s\t%s\t%s\t%s\n" % (t[0], t[3], t[1], t[5], t[4]))
    with open(T + ".psam", "w") as f:
        f.write("#FID\tIID\tSEX\n")
        for s in fam3:
            f.write("%s\t%s\tNA\n" % (s[0], s[1]))
    # the synthetic set: one chromosome, phenotypes with different missingness, LOCO files written here
    g = synthetic_calls()
    S = os.path.join(d, "syn")
    write_plink(S, g, [1] * SYN["M"], P=SYN["P"], seed=SYN["seed"], missing_pheno=SYN["missing_pheno"])
    ids = ["%d_%d" % (i + 1, i + 1) for i in range(SYN["N"])]
    with open(os.path.join(d, "pred_syn.list"), "w") as pl:
        for k in range(1, SYN["P"] + 1):
            fn = os.path.join(d, "syn_%d.loco" % k)
            cc.write_loco(fn, ids, 300 + k)
            pl.write("Y%d %s\n" % (k, fn))
    return g


_EXQ = ["--phenoFile", "{E}/phenotype.txt", "--covarFile", "{E}/covariates.txt", "--pred", "{D}/pred_ex.list", "--bsize", "200", "--chr", "2"]
_EXB = ["--phenoFile", "{E}/phenotype_bin.txt", "--covarFile", "{E}/covariates.txt", "--pred", "{D}/pred_ex.list", "--bsize", "200", "--chr", "2"]
_SYN = ["--bed", "{D}/syn", "--phenoFile", "{D}/syn.pheno", "--covarFile", "{D}/syn.covar", "--pred", "{D}/pred_syn.list", "--bsize", "150", "--qt"]
_BED = ["--bed", "{E}/example_3chr"]
# name -> the whole argument list ({E} the example directory, {D} the directory write_inputs filled)
CASES = {
    "a_qt_dom_bed": ["--step", "2"] + _BED + ["--qt", "--test", "dominant"] + _EXQ,
    "b_qt_rec_minhoms": ["--step", "2", "--test", "recessive", "--minHOMs", str(MIN_HOMS)] + _SYN,
    "c_qt_dom_missing": ["--step", "2", "--test", "dominant"] + _SYN,
    "d_qt_rec_bgen": ["--step", "2", "--bgen", "{E}/example_3chr.bgen", "--sample", "{E}/example_3chr.sample", "--qt", "--test", "recessive"] + _EXQ,
    "e_qt_dom_pgen": ["--step", "2", "--pgen", "{D}/ex3", "--qt", "--test", "dominant"] + _EXQ,
    # (--minHOMs 10: a variant with a handful of homozygotes is near separation under the recessive coding, where the approximate Firth fit of either
    # program stops a stopping tolerance away from its limit -- and its corrected CHISQ can fall below the quantile compare_regenie_files keys on)
    "f_bt_firth_rec": ["--step", "2"] + _BED + ["--bt", "--firth", "--approx", "--test", "recessive", "--minHOMs", "10"] + _EXB,
    "p_bt_rec_score": ["--step", "2"] + _BED + ["--bt", "--test", "recessive"] + _EXB,      # no correction: also tells which rows of (f) / (o) a correction re-tests
    "g_bt_spa_dom": ["--step", "2"] + _BED + ["--bt", "--spa", "--test", "dominant"] + _EXB,
    "h_ct_dom": ["--step", "2"] + _BED + ["--ct", "--test", "dominant", "--phenoFile", "{D}/ex_counts.txt", "--covarFile", "{E}/covariates.txt",
                                          "--pred", "{D}/pred_ex.list", "--bsize", "200", "--chr", "2"],
    "i_qt_rec_ref_first": ["--step", "2"] + _BED + ["--qt", "--test", "recessive", "--ref-first"] + _EXQ,
    "j_qt_dom_condtl": ["--step", "2"] + _BED + ["--qt", "--test", "dominant", "--condition-list", "{D}/cond.txt"] + _EXQ,
    "k_qt_rec_mcc": ["--step", "2"] + _BED + ["--qt", "--test", "recessive", "--mcc", "--mcc-thr", "1"] + _EXQ,
    "l_qt_additive": ["--step", "2"] + _BED + ["--qt", "--test", "additive"] + _EXQ,
    "o_bt_firth_exact_rec": ["--step", "2"] + _BED + ["--bt", "--firth", "--test", "recessive", "--minHOMs", "10"] + _EXB,      # the exact test rebuilds the vector on the host
    "m_bad_value": ["--step", "2"] + _BED + ["--qt", "--test", "overdominant"] + _EXQ,
    "n_step1": ["--step", "1"] + _BED + ["--qt", "--test", "dominant", "--phenoFile", "{E}/phenotype.txt", "--covarFile", "{E}/covariates.txt", "--bsize", "100"],
}
FILE_CASES = [c for c in CASES if c[0] in "abcdefghijklop"]
ERROR_CASES = ["m_bad_value", "n_step1"]
LOG_MARKS = ("homALT carriers",)         # log lines of regenie the driver must print too


def args_of(name, D):
    return [a.replace("{E}", EX).replace("{D}", D) for a in CASES[name]]


def traits_of(name):
    return 2


SCORE_OF = {"f_bt_firth_rec": "p_bt_rec_score", "o_bt_firth_exact_rec": "p_bt_rec_score"}      # corrected case -> the same command without the correction


def golden(name, k):
    return gzip.open(os.path.join(REF, name, "out_Y%d.regenie.gz" % k), "rt").read().splitlines()


# ---- the restatement: recode, then the formulas in the header of include/rg_step2.h ------------------------------------------------------------
def recode(G, coding):
    """G: float array of hard calls 0 / 1 / 2 with NaN missing; coding 0 additive, 1 dominant (2 -> 1), 2 recessive (1 -> 0, 2 -> 1)."""
    if coding == 1:
        return np.where(G == 2, 1.0, G)
    if coding == 2:
        return np.where(G >= 1, G - 1.0, G)
    return G


def qt_block(G, coding, X, res, mask, scf_sv, n_samples=None, numtol=1e-6, min_homs=0.0, min_mac=5.0, filters=True):
    """The Step-2 quantitative-trait test of hard calls G [M][n] (NaN missing) under a coding, in fp64: additive counts (A1FREQ, N and the MAC filter
    per trait), then the recoding, mean imputation with the RECODED mean, check_sparse_G on that vector, the dense or sparse statistic.
    filters=False: the library's view -- no MAC / --minHOMs / recoded-mean filter (those are the caller's), every observed row is scored.
    X [n][C] orthonormal, res / mask [n][P], scf_sv [P].  -> dict of [M][P] arrays (NaN: not printed) and the per-variant integer counts."""
    M, n = G.shape
    P, C = res.shape[1], X.shape[1]
    out = {k: np.full((M, P), np.nan) for k in ("beta", "se", "chisq", "a1freq", "n", "stats", "stats_all", "bhat_all")}      # *_all: before the per-trait MAC filter
    out["sparse"] = np.zeros(M, bool)
    out["scale_fac"] = np.full(M, np.nan)
    out["counts"] = np.zeros((M, 4), np.int64)
    out["total_p"] = np.zeros((M, P))
    out["n_obs_p"] = np.zeros((M, P), np.int64)
    out["mean"] = np.zeros(M)
    out["ignored"] = np.zeros(M, bool)
    for j in range(M):
        obs = ~np.isnan(G[j])
        g_add = np.where(obs, G[j], 0.0)
        out["counts"][j] = [(G[j] == 1).sum(), (G[j] == 2).sum(), (~obs).sum(), 0]
        for t in range(P):
            m = mask[:, t] > 0
            out["total_p"][j, t] = g_add[m].sum()
            out["n_obs_p"][j, t] = (obs & m).sum()
        nobs = int(obs.sum())
        total = g_add.sum()
        r = recode(G[j], coding)
        sum_pos = np.where(obs, r, 0.0).sum()
        out["mean"][j] = sum_pos / nobs if nobs else 0.0
        if nobs == 0 or (filters and (min(total, 2 * nobs - total) < min_mac or (coding == 2 and sum_pos < min_homs) or (coding and sum_pos / nobs < numtol))):
            out["ignored"][j] = True
            continue
        g = np.where(obs, r, sum_pos / nobs)
        b = X.T @ g
        sparse = np.count_nonzero(g) <= (n_samples or n) * 0.5          # check_sparse_G on the vector as tested
        out["sparse"][j] = sparse
        if sparse:       # no residualisation, scale_fac = 1; per-trait denominators with "X'X = I for every trait"
            num = res.T @ g - (res.T @ X) @ b
            den = np.array([float((g * mask[:, t]) @ (g * mask[:, t])) - 2.0 * float((X.T @ (g * mask[:, t])) @ b) + float(b @ b) for t in range(P)])
            out["scale_fac"][j] = 1.0
        else:            # G <- G - X (X^T G), scale_fac = |G| / sqrt(n - C), "ignored" below numtol; denum = mask^T G^2
            v = g - X @ b
            sf = np.linalg.norm(v) / np.sqrt(n - C)
            out["scale_fac"][j] = sf
            if not sf >= numtol:
                out["ignored"][j] = True
                continue
            num, den = res.T @ v, (mask * (v * v)[:, None]).sum(axis=0)
        for t in range(P):
          with np.errstate(invalid="ignore", divide="ignore"):       # an all-zero vector on the sparse branch: 0 / 0
            st = float(num[t]) / np.sqrt(den[t])
            bh = st * scf_sv[t] / np.sqrt(den[t])
            out["stats_all"][j, t], out["bhat_all"][j, t] = st, bh
            tq, nq = out["total_p"][j, t], out["n_obs_p"][j, t]
            if filters and min(tq, 2 * nq - tq) < min_mac:
                continue
            out["stats"][j, t], out["beta"][j, t], out["se"][j, t], out["chisq"][j, t] = st, bh, bh / st, st * st
            out["a1freq"][j, t], out["n"][j, t] = tq / (2.0 * nq), nq
    return out


def null_of(bed, pheno_file, covar_file, loco_fmt, chrom):
    """The null of the quantitative traits of a data set on one chromosome, as tests/test_reference_pin.py builds it: the analysed samples (a sample
    without any phenotype leaves the analysis), then X, res, mask, scf_sv over them.  -> ia (analysed among the file's samples), n_samples, X, res, mask, scf_sv."""
    from oracle import regenie_step1 as s1, regenie_step2_qt as s2o
    opt = s1.Step1Options(bed=bed, pheno_file=pheno_file, covar_file=covar_file, test_mode=True)
    _, _, _, _, prep = s1.load_inputs(opt)
    ia = prep.ind_in_analysis
    assert not prep.ind_ignore.any()
    ids = [i for i, k in zip(prep.ids, ia) if k]
    X, Y, mask = prep.X[ia], prep.Y[ia], prep.mask[ia].astype(np.float64)
    blup = np.zeros_like(Y)
    for k in range(1, Y.shape[1] + 1):
        lines = open(loco_fmt % k).read().splitlines()
        col = {s: i for i, s in enumerate(lines[0].split()[1:])}
        row = [ln.split() for ln in lines[1:] if ln.split()[0] == str(chrom)][0][1:]
        blup[:, k - 1] = [float(row[col[s]]) for s in ids]
    res, _, scf = s2o.compute_res(Y, blup * mask, mask, prep.Neff, X.shape[1], prep.scale_Y)
    return ia, len(ia), X, res, mask, scf


def example_null(tmp, pheno_file=None):
    """The null of the example's two quantitative traits on chromosome 2: X, res, mask, scf_sv."""
    return null_of(os.path.join(EX, "example_3chr"), pheno_file or os.path.join(EX, "phenotype.txt"), os.path.join(EX, "covariates.txt"),
                   os.path.join(tmp, "ex_%d.loco"), 2)[2:]


def restate_example_bed(name, tmp):
    """Cases on example_3chr.bed, chromosome 2: -> qt_block's dict."""
    from tests.ld_cases import read_bed
    a = CASES[name]
    coding = {"additive": 0, "dominant": 1, "recessive": 2}[a[a.index("--test") + 1]]
    G, ids, chrom, _, _ = read_bed(os.path.join(EX, "example_3chr"))
    G = G[np.array([str(c) == "2" for c in chrom])]
    if "--ref-first" in a:
        G = 2.0 - G
    X, res, mask, scf = example_null(tmp)
    return qt_block(G, coding, X, res, mask, scf)


def restate_synthetic_bed(name, tmp):
    """Cases (b) and (c) on the synthetic .bed -- missing calls, traits that differ in their missing values, `--minHOMs`: -> ids, qt_block's dict."""
    from tests.ld_cases import read_bed
    a = CASES[name]
    coding = {"additive": 0, "dominant": 1, "recessive": 2}[a[a.index("--test") + 1]]
    min_homs = float(a[a.index("--minHOMs") + 1]) if "--minHOMs" in a else 0.0
    S = os.path.join(tmp, "syn")
    G, ids, _, _, fam = read_bed(S)
    ia, n_samples, X, res, mask, scf = null_of(S, S + ".pheno", S + ".covar", os.path.join(tmp, "syn_%d.loco"), 1)
    return ids, qt_block(G[:, ia], coding, X, res, mask, scf, n_samples=n_samples, min_homs=min_homs)
