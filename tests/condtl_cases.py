"""The reference cases of conditional analysis (`--step 2 --condition-list FILE [--condition-file FORMAT,FILE]`): the command lines and the
generator of their inputs -- one definition for tests/golden/make_condtl_ref_outputs.py (which runs regenie itself on them) and for the tests
(which run the driver).  Two data sets: the example's example_3chr (500 samples, chromosome 2 = 400 variants) with the LOCO files regenie's
Step 1 wrote for it (ref_outputs/qt_kfold_3chr), and 600 synthetic samples x 300 variants from tests/util.py's writers with LOCO files written
here (any prediction is a valid offset of Step 2)."""
import gzip
import os
import shutil

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "tests", "golden", "example")
REF = os.path.join(ROOT, "tests", "golden", "ref_outputs", "condtl")

# example_3chr: three variants of chromosome 2 (inf_0 .. inf_399); the list of case (a) in ascending id order
EX_COND = ["inf_120", "inf_260", "inf_75"]
assert EX_COND == sorted(EX_COND)
EX_MISSING = ("inf_260", 17)          # case (a): this variant gets 17 missing calls
# the synthetic set: ids s0 .. s299, chromosome 1 = s0 .. s99, chromosome 2 = s100 .. s299
SYN = dict(M=300, N=600, chroms=[1] * 100 + [2] * 200, P=3, seed=41, miss_rate=0.02, missing_pheno=0.1)
SYN_COND = ["s130", "s177", "s215"]
N_EXTRA = 50                          # samples of the --condition-file that are not in the main file


def write_loco(path, ids, seed):
    """A LOCO file as Step 1 writes it: FID_IID header, one row per chromosome 1 .. 23."""
    rng = np.random.default_rng(seed)
    with open(path, "w") as f:
        f.write("FID_IID " + " ".join(ids) + "\n")
        for c in range(1, 24):
            f.write("%d " % c + " ".join("%.6g" % v for v in 0.15 * rng.standard_normal(len(ids))) + "\n")


def _set_missing(src, dst, vid, k):
    """Copies the .bed / .bim / .fam trio src -> dst with k calls of variant vid set to missing (code 01)."""
    for ext in (".bim", ".fam"):
        shutil.copy(src + ext, dst + ext)
    ids = [ln.split()[1] for ln in open(src + ".bim")]
    n = sum(1 for _ in open(src + ".fam"))
    raw = bytearray(open(src + ".bed", "rb").read())
    bpr = (n + 3) // 4
    row = 3 + ids.index(vid) * bpr
    for i in np.random.default_rng(5).choice(n, k, replace=False):
        raw[row + i // 4] = (raw[row + i // 4] & ~(3 << (2 * (i % 4)))) | (1 << (2 * (i % 4)))
    open(dst + ".bed", "wb").write(bytes(raw))


def second_file_samples():
    """The samples of the --condition-file: the 600 of the main file and N_EXTRA more, permuted.  -> list of (fid, iid), main-file index or -1."""
    n = SYN["N"]
    perm = np.random.default_rng(77).permutation(n + N_EXTRA)
    return [("%d" % (k + 1), "%d" % (k + 1)) for k in perm], [int(k) if k < n else -1 for k in perm]


def write_inputs(d):
    """Writes every input the cases need into directory d and returns the synthetic hard calls g (M, N; -3 missing)."""
    from oracle import bgen as obg, pgen as opg
    from tests.util import pack_bed, synth_dosages, u01, write_plink, write_synth_bgen, write_synth_pgen
    R = os.path.join(ROOT, "tests", "golden", "ref_outputs", "qt_kfold_3chr")
    with open(os.path.join(d, "pred_ex.list"), "w") as pl:
        for k in (1, 2):
            fn = os.path.join(d, "ex_%d.loco" % k)
            open(fn, "wb").write(gzip.open(os.path.join(R, "out_%d.loco.gz" % k), "rb").read())
            pl.write("Y%d %s\n" % (k, fn))
    _set_missing(os.path.join(EX, "example_3chr"), os.path.join(d, "ex3m"), *EX_MISSING)
    with open(os.path.join(d, "cond_ex.txt"), "w") as f:
        f.write("\n".join(EX_COND) + "\n")
    with open(os.path.join(d, "cond_ex_shuffled.txt"), "w") as f:      # out of order, one id twice, a second token on a line
        f.write("%s\n%s\tignored\n%s\n%s\n" % (EX_COND[2], EX_COND[0], EX_COND[2], EX_COND[1]))
    with open(os.path.join(d, "cond_ex_unknown.txt"), "w") as f:
        f.write("%s\nnot_a_variant\n%s\n" % (EX_COND[0], EX_COND[1]))
    # count phenotypes for the example's samples
    rng = np.random.default_rng(19)
    fam = [ln.split()[:2] for ln in open(os.path.join(EX, "example_3chr.fam"))]
    with open(os.path.join(d, "ex_counts.txt"), "w") as f:
        f.write("FID IID Y1 Y2\n")
        for a, b in fam:
            f.write("%s %s %d %d\n" % (a, b, rng.poisson(2.0), rng.poisson(0.7)))
    # 62 covariates for the example's samples (the cap)
    with open(os.path.join(d, "ex_cov62.txt"), "w") as f:
        f.write("FID IID " + " ".join("W%d" % (c + 1) for c in range(62)) + "\n")
        for a, b in fam:
            f.write("%s %s " % (a, b) + " ".join("%.6f" % v for v in rng.standard_normal(62)) + "\n")
    # the synthetic set in the three formats
    S = os.path.join(d, "syn")
    g = synth_dosages(SYN["M"], SYN["N"], miss_rate=SYN["miss_rate"], seed=SYN["seed"])
    write_plink(S, g, SYN["chroms"], P=SYN["P"], seed=SYN["seed"], missing_pheno=SYN["missing_pheno"])
    write_synth_bgen(S, g, SYN["chroms"], seed=SYN["seed"])
    write_synth_pgen(S + "_p", g, SYN["chroms"], seed=SYN["seed"], soft=0.4)
    ids = ["%d_%d" % (i + 1, i + 1) for i in range(SYN["N"])]
    with open(os.path.join(d, "pred_syn.list"), "w") as pl:
        for k in range(1, SYN["P"] + 1):
            fn = os.path.join(d, "syn_%d.loco" % k)
            write_loco(fn, ids, 100 + k)
            pl.write("Y%d %s\n" % (k, fn))
    with open(os.path.join(d, "cond_syn.txt"), "w") as f:
        f.write("\n".join(SYN_COND) + "\n")
    # the second genotype file of case (h): 8 variants -- the three of the list among them, not in id order -- for a permuted superset of the samples.
    # The shared samples carry the main file's calls; hard calls in .bed and .pgen, 8-bit probabilities in the BGEN file
    vids = ["s10", SYN_COND[2], "s250", SYN_COND[0], "s101", SYN_COND[1], "s299", "s5"]
    vidx = [int(v[1:]) for v in vids]
    sam, where = second_file_samples()
    w = np.array(where)
    extra = synth_dosages(len(vids), len(sam), miss_rate=0.03, seed=SYN["seed"] + 1)
    g2 = np.where(w[None, :] >= 0, g[np.array(vidx)][:, np.maximum(w, 0)], extra).astype(np.int8)
    T = os.path.join(d, "second")
    with open(T + ".bed", "wb") as f:
        f.write(b"\x6c\x1b\x01")
        f.write(pack_bed(g2).tobytes())
    with open(T + ".bim", "w") as f:
        for v, j in zip(vids, vidx):
            f.write("%d\t%s\t0\t%d\tA\tG\n" % (SYN["chroms"][j], v, j + 1))
    with open(T + ".fam", "w") as f:
        for a, b in sam:
            f.write("%s %s 0 0 0 -9\n" % (a, b))
    opg.write_pgen_fixed(T + ".pgen", np.where(g2 < 0, 3, g2).astype(np.uint8))
    with open(T + ".pvar", "w") as f:
        f.write("#CHROM\tPOS\tID\tREF\tALT\n")
        for v, j in zip(vids, vidx):
            f.write("%d\t%d\t%s\tG\tA\n" % (SYN["chroms"][j], j + 1, v))
    with open(T + ".psam", "w") as f:
        f.write("#FID\tIID\tSEX\n")
        for a, b in sam:
            f.write("%s\t%s\tNA\n" % (a, b))
    jj, ii = np.arange(len(vids))[:, None], np.arange(len(sam))[None, :]
    hom, het = np.where(g2 == 2, 255, 0).astype(np.int64), np.where(g2 == 1, 255, 0).astype(np.int64)
    soft = (u01(900, jj, ii) < 0.4) & (g2 == 1)          # some heterozygous calls smeared towards the first homozygote
    amt = (u01(901, jj, ii) * 80).astype(np.int64)
    het[soft] -= amt[soft]
    hom[soft] += amt[soft]
    obg.write_bgen(T + ".bgen", np.stack([hom, het], axis=-1).astype(np.uint8), g2 < 0, [(int(SYN["chroms"][j]), j + 1, v, "A", "G") for v, j in zip(vids, vidx)],
                   sample_ids=["anon_%d" % k for k in range(len(sam))], compression=1)
    with open(T + ".sample", "w") as f:
        f.write("ID_1 ID_2 missing\n0 0 0\n")
        for a, b in sam:
            f.write("%s %s 0\n" % (a, b))
    return g


_EXQ = ["--phenoFile", "{E}/phenotype.txt", "--covarFile", "{E}/covariates.txt", "--pred", "{D}/pred_ex.list", "--bsize", "200", "--chr", "2"]
_EXB = ["--phenoFile", "{E}/phenotype_bin.txt", "--covarFile", "{E}/covariates.txt", "--pred", "{D}/pred_ex.list", "--bsize", "200", "--chr", "2"]
_SYN = ["--phenoFile", "{D}/syn.pheno", "--covarFile", "{D}/syn.covar", "--pred", "{D}/pred_syn.list", "--bsize", "100", "--chr", "2", "--qt"]
# name -> arguments after `--step 2` ({E} the example directory, {D} the directory write_inputs filled)
CASES = {
    "a_qt_bed": ["--bed", "{D}/ex3m", "--qt", "--condition-list", "{D}/cond_ex.txt"] + _EXQ,
    "b_qt_bed_shuffled": ["--bed", "{D}/ex3m", "--qt", "--condition-list", "{D}/cond_ex_shuffled.txt"] + _EXQ,
    "c_bt_firth": ["--bed", "{D}/ex3m", "--bt", "--firth", "--approx", "--condition-list", "{D}/cond_ex.txt"] + _EXB,
    "c_bt_spa": ["--bed", "{D}/ex3m", "--bt", "--spa", "--condition-list", "{D}/cond_ex.txt"] + _EXB,
    "d_ct": ["--bed", "{D}/ex3m", "--ct", "--condition-list", "{D}/cond_ex.txt", "--phenoFile", "{D}/ex_counts.txt", "--covarFile", "{E}/covariates.txt",
             "--pred", "{D}/pred_ex.list", "--bsize", "200", "--chr", "2"],
    "e_qt_missing": ["--bed", "{D}/syn", "--condition-list", "{D}/cond_syn.txt"] + _SYN,
    "f_bgen": ["--bgen", "{D}/syn.bgen", "--sample", "{D}/syn.sample", "--condition-list", "{D}/cond_syn.txt"] + _SYN,
    "f_bgen_ref_first": ["--bgen", "{D}/syn.bgen", "--sample", "{D}/syn.sample", "--ref-first", "--condition-list", "{D}/cond_syn.txt"] + _SYN,
    "g_pgen_dosage": ["--pgen", "{D}/syn_p", "--condition-list", "{D}/cond_syn.txt"] + _SYN,
    "h_file_bed": ["--bed", "{D}/syn", "--condition-list", "{D}/cond_syn.txt", "--condition-file", "bed,{D}/second"] + _SYN,
    "h_file_pgen": ["--bed", "{D}/syn", "--condition-list", "{D}/cond_syn.txt", "--condition-file", "pgen,{D}/second"] + _SYN,
    "h_file_bgen": ["--bed", "{D}/syn", "--condition-list", "{D}/cond_syn.txt", "--condition-file", "bgen,{D}/second.bgen",
                    "--condition-file-sample", "{D}/second.sample"] + _SYN,
    "i_unknown_id": ["--bed", "{D}/ex3m", "--qt", "--condition-list", "{D}/cond_ex_unknown.txt"] + _EXQ,
    "j_max_vars": ["--bed", "{D}/ex3m", "--qt", "--condition-list", "{D}/cond_ex.txt", "--max-condition-vars", "2"] + _EXQ,
    "k_corr": ["--bed", "{D}/ex3m", "--covarFile", "{E}/covariates.txt", "--bsize", "100", "--chr", "2", "--compute-corr", "--condition-list", "{D}/cond_ex.txt"],
}
FILE_CASES = [c for c in CASES if c[0] in "abcdefgh"]      # compared file against file
ERROR_CASES = ["i_unknown_id", "j_max_vars"]


def args_of(name, D):
    return ["--step", "2"] + [a.replace("{E}", EX).replace("{D}", D) for a in CASES[name]]


def traits_of(name):
    return 3 if "{D}/syn.pheno" in CASES[name] else 2


def compare_regenie_files(got, ref, name):
    """Lines of a .regenie file against regenie's own.  Expected: byte-identical.  A line that is not must meet the rule tests/test_cli_gpu.py applies to
    its route -- the identifying columns, N, TEST and EXTRA as text, A1FREQ as text (files with an INFO column: A1FREQ and INFO as text or within 2e-6,
    they are sums of dosages), BETA / SE / CHISQ / LOG10P to the printed digits (2e-5; --spa 3e-5; rows the approximate Firth test corrected, CHISQ above
    the 0.95 quantile, 2e-4: regenie's own stopping tolerance).  -> the number of lines that are not byte-identical."""
    from pytest import approx
    assert got[0] == ref[0] and len(got) == len(ref) and len(ref) > 150, name
    ncol = len(ref[0].split(" "))
    assert ncol in (13, 14)
    t0 = ncol - 5                                    # first of BETA SE CHISQ LOG10P
    rel = 3e-5 if "spa" in name else 2e-5
    differ = 0
    for a, b in zip(got[1:], ref[1:]):
        if a == b:
            continue
        differ += 1
        ta, tb = a.split(" "), b.split(" ")
        assert ta[:5] == tb[:5] and ta[t0 - 2:t0] == tb[t0 - 2:t0] and ta[-1] == tb[-1], (name, a, b)       # ids, N TEST, EXTRA
        if ncol == 13:
            assert ta[5] == tb[5], (name, a, b)                                                             # A1FREQ
        else:
            for x, y in zip(ta[5:t0 - 2], tb[5:t0 - 2]):                                                    # A1FREQ INFO
                assert x == y or float(x) == approx(float(y), rel=2e-6), (name, a, b)
        corrected = "firth" in name and tb[t0 + 2] != "NA" and float(tb[t0 + 2]) > 3.8414588
        for x, y in zip(ta[t0:t0 + 4], tb[t0:t0 + 4]):
            assert (x == y == "NA") or float(x) == approx(float(y), rel=2e-4 if corrected else rel, abs=2e-9), (name, a, b)
    return differ
