"""The reference cases of the moment-matched Step-2 test (`--step 2 --qt --mcc [--mcc-thr p] [--mcc-skew s]`): the command lines and the generator
of their inputs -- one definition for tests/golden/make_mcc_ref_outputs.py (which runs regenie itself on them) and for the tests (which run the
driver).  Data: the example's example_3chr (500 samples, chromosome 2 = 400 variants) as .bed, .bgen and -- written here -- a hard-call .pgen;
the example's two phenotypes pushed through exp() (skewed), the second with scattered NAs so that the masks differ; covariates as shipped; the
LOCO files regenie's Step 1 wrote for the example (ref_outputs/qt_kfold_3chr: any prediction is a valid offset of Step 2)."""
import gzip
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "tests", "golden", "example")
REF = os.path.join(ROOT, "tests", "golden", "ref_outputs", "mcc")
COND = ["inf_120", "inf_260", "inf_75"]          # case (f), ascending id order
N_NA = 41                                        # missing values of the second trait


def phenotypes():
    """-> ids [(fid, iid)], Y (500, 2): exp() of the example's phenotypes, NaN where the second trait is set missing."""
    rows = [ln.split() for ln in list(open(os.path.join(EX, "phenotype.txt")))[1:]]
    ids = [(r[0], r[1]) for r in rows]
    Y = np.exp(np.array([[float(r[2]), float(r[3])] for r in rows]))
    Y[np.random.default_rng(23).choice(len(rows), N_NA, replace=False), 1] = np.nan
    return ids, Y


def skewness(y):
    y = y[~np.isnan(y)]
    d = y - y.mean()
    return float((d ** 3).mean() / (d ** 2).mean() ** 1.5)


def skew_threshold():
    """A value of --mcc-skew between the two traits' skewness, so that exactly one qualifies."""
    _, Y = phenotypes()
    s = sorted(abs(skewness(Y[:, k])) for k in range(2))
    assert s[1] - s[0] > 0.01
    return "%.3f" % (0.5 * (s[0] + s[1]))


def write_inputs(d):
    """Writes every input the cases need into directory d."""
    from oracle import pgen as opg
    from tests.ld_cases import read_bed
    R = os.path.join(ROOT, "tests", "golden", "ref_outputs", "qt_kfold_3chr")
    with open(os.path.join(d, "pred.list"), "w") as pl:
        for k in (1, 2):
            fn = os.path.join(d, "ex_%d.loco" % k)
            open(fn, "wb").write(gzip.open(os.path.join(R, "out_%d.loco.gz" % k), "rb").read())
            pl.write("Y%d %s\n" % (k, fn))
    ids, Y = phenotypes()
    with open(os.path.join(d, "pheno_skew.txt"), "w") as f:
        f.write("FID IID Y1 Y2\n")
        for (a, b), y in zip(ids, Y):
            f.write("%s %s %.10g %s\n" % (a, b, y[0], "NA" if np.isnan(y[1]) else "%.10g" % y[1]))
    with open(os.path.join(d, "cond.txt"), "w") as f:
        f.write("\n".join(COND) + "\n")
    # the hard calls of example_3chr as a .pgen (ALT = the first .bim allele, which .bed counts)
    G, vid, _, _, fam = read_bed(os.path.join(EX, "example_3chr"))
    bim = [ln.split() for ln in open(os.path.join(EX, "example_3chr.bim"))]
    T = os.path.join(d, "ex3")
    opg.write_pgen_fixed(T + ".pgen", np.where(np.isnan(G), 3, G).astype(np.uint8))
    with open(T + ".pvar", "w") as f:
        f.write("#CHROM\tPOS\tID\tREF\tALT\n")
        for t in bim:
            f.write("%s\t%s\t%s\t%s\t%s\n" % (t[0], t[3], t[1], t[5], t[4]))
    with open(T + ".psam", "w") as f:
        f.write("#FID\tIID\tSEX\n")
        for s in fam:
            f.write("%s\t%s\tNA\n" % (s[0], s[1]))


_COMMON = ["--phenoFile", "{D}/pheno_skew.txt", "--covarFile", "{E}/covariates.txt", "--pred", "{D}/pred.list", "--bsize", "200", "--chr", "2", "--qt"]
_BED = ["--bed", "{E}/example_3chr"]
# name -> arguments after `--step 2` ({E} the example directory, {D} the directory write_inputs filled)
CASES = {
    "a_bed_all": _BED + ["--mcc", "--mcc-thr", "1"] + _COMMON,
    "b_bed_thr": _BED + ["--mcc"] + _COMMON,
    "c_bed_skew": _BED + ["--mcc", "--mcc-skew", skew_threshold()] + _COMMON,
    "d_bgen_all": ["--bgen", "{E}/example_3chr.bgen", "--sample", "{E}/example_3chr.sample", "--mcc", "--mcc-thr", "1"] + _COMMON,
    "e_pgen_all": ["--pgen", "{D}/ex3", "--mcc", "--mcc-thr", "1"] + _COMMON,
    "f_bed_condtl": _BED + ["--mcc", "--mcc-thr", "1", "--condition-list", "{D}/cond.txt"] + _COMMON,
    "g_skew_without_mcc": _BED + ["--mcc-skew", "1"] + _COMMON,
    "h_negative_skew": _BED + ["--mcc", "--mcc-skew", "-1"] + _COMMON,
}
FILE_CASES = [c for c in CASES if c[0] in "abcdef"]
ERROR_CASES = ["g_skew_without_mcc", "h_negative_skew"]


def args_of(name, D):
    return ["--step", "2"] + [a.replace("{E}", EX).replace("{D}", D) for a in CASES[name]]
