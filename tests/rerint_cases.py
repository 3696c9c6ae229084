"""The reference cases of the two-stage rank-inverse-normal transformation of the Step-2 residuals (`--step 2 --qt --apply-rerint | --apply-rerint-cov`):
the command lines and the generator of their inputs -- one definition for tests/golden/make_rerint_ref_outputs.py (which runs regenie itself on them)
and for the tests (which run the driver).  Data: what tests/mcc_cases.py writes (example_3chr as .bed / .bgen / .pgen, two skewed phenotypes of which the
second has scattered NAs, the LOCO files of ref_outputs/qt_kfold_3chr, a condition list), plus
  cov_cat.txt     the example's covariates and a categorical one with three levels (case b)
  pheno_ties.txt  two phenotypes on coarse grids (11 and 5 distinct values), the second with NAs; with pred_zero.list -- LOCO files of zeros -- and no
                  covariate file the Step-2 residuals are the centred phenotypes and tie exactly as the phenotypes do (case h)."""
import os

import numpy as np

from tests import mcc_cases as mc

ROOT = mc.ROOT
EX = mc.EX
REF = os.path.join(ROOT, "tests", "golden", "ref_outputs", "rerint")
TIE_LEVELS = (11, 5)


def tied_phenotypes():
    """-> ids, Y (500, 2) on grids of TIE_LEVELS values, NaN where the second trait is missing (the rows tests/mcc_cases.py sets missing)."""
    ids, Ys = mc.phenotypes()
    rng = np.random.default_rng(31)
    Y = np.column_stack([rng.integers(0, k, len(ids)).astype(np.float64) for k in TIE_LEVELS])
    Y[np.isnan(Ys[:, 1]), 1] = np.nan
    return ids, Y


def write_inputs(d):
    mc.write_inputs(d)
    rows = [ln.split() for ln in open(os.path.join(EX, "covariates.txt"))]
    cat = np.random.default_rng(29).integers(0, 3, len(rows) - 1)
    with open(os.path.join(d, "cov_cat.txt"), "w") as f:
        f.write(" ".join(rows[0]) + " CAT\n")
        for r, c in zip(rows[1:], cat):
            f.write(" ".join(r) + " %s\n" % "abc"[c])
    ids, Y = tied_phenotypes()
    with open(os.path.join(d, "pheno_ties.txt"), "w") as f:
        f.write("FID IID Y1 Y2\n")
        for (a, b), y in zip(ids, Y):
            f.write("%s %s %d %s\n" % (a, b, y[0], "NA" if np.isnan(y[1]) else "%d" % y[1]))
    with open(os.path.join(d, "pred_zero.list"), "w") as pl:
        for k in (1, 2):
            fn = os.path.join(d, "zero_%d.loco" % k)
            with open(fn, "w") as f:
                f.write("FID_IID " + " ".join("%s_%s" % ab for ab in ids) + "\n")
                for c in range(1, 24):
                    f.write("%d " % c + " ".join("0" for _ in ids) + "\n")
            pl.write("Y%d %s\n" % (k, fn))


_TAIL = ["--pred", "{D}/pred.list", "--bsize", "200", "--chr", "2"]
_PHENO = ["--phenoFile", "{D}/pheno_skew.txt", "--covarFile", "{E}/covariates.txt"] + _TAIL + ["--qt"]
_BED = ["--bed", "{E}/example_3chr"]
_BT = _BED + ["--phenoFile", "{E}/phenotype_bin.txt", "--covarFile", "{E}/covariates.txt"] + _TAIL + ["--bt"]
# name -> arguments after `--step 2` ({E} the example directory, {D} the directory write_inputs filled)
CASES = {
    "a_bed_rerint": _BED + ["--apply-rerint"] + _PHENO,
    "b_bed_cov_cat": _BED + ["--apply-rerint-cov", "--phenoFile", "{D}/pheno_skew.txt", "--covarFile", "{D}/cov_cat.txt", "--catCovarList", "CAT"] + _TAIL + ["--qt"],
    "c_bgen_cov": ["--bgen", "{E}/example_3chr.bgen", "--sample", "{E}/example_3chr.sample", "--apply-rerint-cov"] + _PHENO,
    "d_pgen_rerint": ["--pgen", "{D}/ex3", "--apply-rerint"] + _PHENO,
    "e_bed_rerint_mcc": _BED + ["--apply-rerint", "--mcc", "--mcc-thr", "1"] + _PHENO,
    "f_bed_cov_condtl": _BED + ["--apply-rerint-cov", "--condition-list", "{D}/cond.txt"] + _PHENO,
    "g_bt_ignored": _BT + ["--apply-rerint"],
    "g0_bt_plain": _BT,
    "h_bed_ties": _BED + ["--apply-rerint", "--phenoFile", "{D}/pheno_ties.txt", "--pred", "{D}/pred_zero.list", "--bsize", "200", "--chr", "2", "--qt"],
}
QT_CASES = [c for c in CASES if c[0] in "abcdefh"]
RESTATED = ["a_bed_rerint", "b_bed_cov_cat", "c_bgen_cov", "d_pgen_rerint", "e_bed_rerint_mcc", "f_bed_cov_condtl", "h_bed_ties"]      # tests/rerint_restate.py restate_case


def args_of(name, D):
    return ["--step", "2"] + [a.replace("{E}", EX).replace("{D}", D) for a in CASES[name]]


def mode_of(name):
    """1: --apply-rerint, 2: --apply-rerint-cov (RG_S2_RERINT / RG_S2_RERINT_COV)."""
    return 2 if "--apply-rerint-cov" in CASES[name] else 1
