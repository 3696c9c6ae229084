"""The reference cases of Step 2 on chromosome X with males (`--step 2 --par-region BUILD`): the command lines, the generator of their inputs and a
NumPy restatement of the reference's minor-allele-count rule -- one definition for tests/golden/make_chrx_ref_outputs.py (which runs regenie itself)
and for the tests (which run the driver).

Data: 400 synthetic samples (about half male, a few with sex code 0) x 400 variants from tests/util.py's writers: chromosome 22 = s0 .. s99,
chromosome 23 = s100 .. s399 with positions on both sides of both PAR bounds of hg19 / b37 (the bounds themselves included) and of the custom
`5000000,100000000`.  Outside the PAR regions males are coded 0 / 2.  Three groups of variants are built by hand:
  DROP  3 - 4 male homozygotes and 0 - 1 female heterozygote: autosomal MAC >= 5 (kept by the autosomal rule), sex-aware MAC < 5 (dropped)
  FLIP  4 male homozygotes, one of them without phenotype Y2, and 1 female heterozygote: the variant is kept (sex-aware MAC 5), the test of Y2 has
        autosomal MAC 7 and sex-aware MAC 4
  F50   20 male homozygotes and 15 female heterozygotes: sparse, autosomal MAC 55 >= 50, sex-aware MAC 35 < 50 (the carriers-only Firth fit)
LOCO files are written here (any prediction is a valid offset of Step 2)."""
import gzip
import os

import numpy as np

from tests import condtl_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "ref_outputs", "chrx")
N, M, P = 400, 400, 2
CHROMS = [22] * 100 + [23] * 300
BOUNDS = {"hg18": (2709520, 154584238), "b36": (2709520, 154584238), "hg19": (2699520, 154931044), "b37": (2699520, 154931044),
          "hg38": (2781479, 155701383), "b38": (2781479, 155701383)}
MIN_MAC = 5.0
DROP = list(range(130, 144))
FLIP = list(range(150, 158))
F50 = list(range(170, 176))
HET_MALE = [200, 221, 305]          # the het-male case: these non-PAR variants get male calls of 1
SEED = 61


def par_bounds(code):
    """check_build_code (Regenie.cpp:1643-1660) -> (par1_max_bound, par2_min_bound); ValueError for what the reference refuses."""
    if code in BOUNDS:
        return BOUNDS[code]
    t = code.split(",")
    try:
        a, b = int(t[0]), int(t[1])
    except (ValueError, IndexError):
        raise ValueError("invalid build code given")
    if a < 1 or b < 1 or b < a:
        raise ValueError("invalid build code given")
    return a - 1, b + 1


def positions():
    p1, p2 = BOUNDS["hg19"]
    pos = list(range(1, 101))                                                        # chromosome 22
    pos += [int(v) for v in np.linspace(60001, p1, 20)]                              # PAR1, the bound itself last
    pos += [int(v) for v in np.linspace(p1 + 1, p2 - 1, 260)]                        # non-PAR, both neighbours of the bounds included
    pos += [int(v) for v in np.linspace(p2, p2 + 300000, 20)]                        # PAR2, the bound itself first
    return np.array(pos, np.int64)


def non_par(code):
    """in_non_par (Geno.cpp:2802-2814) per variant."""
    lo, hi = par_bounds(code)
    pos = positions()
    return (np.array(CHROMS) == 23) & (pos > lo) & (pos < hi)


def sexes():
    from tests.util import u01
    sex = np.where(u01(811, 0, np.arange(N)) < 0.5, 1, 2)
    sex[[7, 91, 203, 333, 390]] = 0                                                  # unknown: not male
    return sex


def na_y2(pheno_missing):
    """Males with both phenotypes whose Y2 is then set to NA (Y1 stays): one of them carries each FLIP variant."""
    return np.flatnonzero((sexes() == 1) & ~pheno_missing)[5:5 + len(FLIP)]


def calls(pheno_missing):
    """int8 (M, N), -3 missing.  pheno_missing [N] bool: samples with a missing phenotype (the hand-built variants avoid them as carriers, apart
    from the FLIP male)."""
    from tests.util import synth_dosages
    g = synth_dosages(M, N, miss_rate=0.02, seed=SEED)
    sex = sexes()
    male = sex == 1
    npar = non_par("hg19")
    hemi = np.where(g >= 1, np.int8(2), g)                                           # males outside the PAR regions: 0 / 2
    g = np.where(npar[:, None] & male[None, :], hemi, g).astype(np.int8)
    rng = np.random.default_rng(SEED)
    free_m = np.setdiff1d(np.flatnonzero(male & ~pheno_missing), na_y2(pheno_missing))
    free_f = np.flatnonzero((sex == 2) & ~pheno_missing)
    for t, row in enumerate(DROP):      # autosomal / sex-aware MAC: 7 / 4, 8 / 4, 6 / 3 (the last with two missing calls)
        v = np.zeros(N, np.int8)
        v[rng.choice(free_m, 4 if t % 3 == 1 else 3, replace=False)] = 2
        if t % 3 == 0:
            v[rng.choice(free_f, 1, replace=False)] = 1
        if t % 3 == 2:
            v[rng.choice(free_f, 2, replace=False)] = -3
        g[row] = v
    for t, row in enumerate(FLIP):
        v = np.zeros(N, np.int8)
        v[rng.choice(free_m, 3, replace=False)] = 2
        v[na_y2(pheno_missing)[t]] = 2
        v[rng.choice(free_f, 1, replace=False)] = 1
        g[row] = v
    for row in F50:
        v = np.zeros(N, np.int8)
        v[rng.choice(free_m, 20, replace=False)] = 2
        v[rng.choice(free_f, 15, replace=False)] = 1
        g[row] = v
    return g


def _rewrite(prefix, sex, g=None):
    """write_plink's .bim / .fam with the positions and the sex codes of these cases."""
    pos = positions()
    with open(prefix + ".bim", "w") as f:
        for j in range(M):
            f.write("%d\ts%d\t0\t%d\tA\tG\n" % (CHROMS[j], j, pos[j]))
    with open(prefix + ".fam", "w") as f:
        for i in range(N):
            f.write("%d %d 0 0 %d -9\n" % (i + 1, i + 1, sex[i]))


def _pheno_missing(path):
    rows = [ln.split() for ln in open(path)][1:]
    return np.array([any(v == "NA" for v in r[2:]) for r in rows])


def _set_na(path, samples, col):
    lines = open(path).read().splitlines()
    for i in samples:
        t = lines[1 + i].split(" ")
        t[2 + col] = "NA"
        lines[1 + i] = " ".join(t)
    open(path, "w").write("\n".join(lines) + "\n")


def write_inputs(d):
    """Writes every input the cases need into directory d; returns (calls, het-male calls)."""
    from oracle import bgen as obg, pgen as opg
    from tests.util import u01, write_bed_bim, write_plink
    sex = sexes()
    Q, B, Cn = os.path.join(d, "xq"), os.path.join(d, "xb"), os.path.join(d, "xc")
    g0 = np.zeros((M, N), np.int8)
    write_plink(Q, g0, CHROMS, P=P, seed=SEED, missing_pheno=0.1)                    # (the missing values do not depend on the calls)
    miss = _pheno_missing(Q + ".pheno")
    g = calls(miss)
    write_plink(Q, g, CHROMS, P=P, seed=SEED, missing_pheno=0.1)
    assert (_pheno_missing(Q + ".pheno") == miss).all()
    _set_na(Q + ".pheno", na_y2(miss), 1)
    write_plink(B, g, CHROMS, P=P, seed=SEED + 1, binary=True)
    write_plink(Cn, g, CHROMS, P=P, seed=SEED + 2, counts="poisson")
    for pre in (Q, B, Cn):
        _rewrite(pre, sex)
    # the same .bed with every sex code 0: the autosomal lines
    Z = os.path.join(d, "xq0")
    write_bed_bim(Z, g, CHROMS)
    _rewrite(Z, np.zeros(N, int))
    # het males
    gh = g.copy()
    males = np.flatnonzero(sex == 1)
    for t, row in enumerate(HET_MALE):
        gh[row, males[10 * t:10 * t + 4]] = 1
    H = os.path.join(d, "xh")
    write_bed_bim(H, gh, CHROMS)
    _rewrite(H, sex)
    pos = positions()
    # hard-call .pgen (ALT = A, the allele .bed counts) and its twin without sex codes
    for pre, sx in (("xp", sex), ("xp0", np.zeros(N, int))):
        T = os.path.join(d, pre)
        opg.write_pgen_fixed(T + ".pgen", np.where(g < 0, 3, g).astype(np.uint8))
        with open(T + ".pvar", "w") as f:
            f.write("#CHROM\tPOS\tID\tREF\tALT\n")
            for j in range(M):
                f.write("%d\t%d\ts%d\tG\tA\n" % (CHROMS[j], pos[j], j))
        with open(T + ".psam", "w") as f:
            f.write("#FID\tIID\tSEX\n")
            for i in range(N):
                f.write("%d\t%d\t%s\n" % (i + 1, i + 1, "NA" if sx[i] == 0 else str(sx[i])))
    # 8-bit BGEN (zlib: the device decoder's route): a third of the calls of the random variants smeared into genuine probabilities
    jj, ii = np.arange(M)[:, None], np.arange(N)[None, :]
    hom, het = np.where(g == 2, 255, 0).astype(np.int64), np.where(g == 1, 255, 0).astype(np.int64)
    built = np.zeros(M, bool)
    built[DROP + FLIP + F50] = True
    soft = (u01(900 + SEED, jj, ii) < 0.33) & (g == 2) & ~built[:, None]             # homozygotes smeared towards the heterozygote
    amt = (u01(901 + SEED, jj, ii) * 60).astype(np.int64)
    hom[soft] -= amt[soft]
    het[soft] += amt[soft]
    obg.write_bgen(os.path.join(d, "x.bgen"), np.stack([hom, het], axis=-1).astype(np.uint8), g < 0,
                   [(int(CHROMS[j]), int(pos[j]), "s%d" % j, "A", "G") for j in range(M)], sample_ids=["%d_%d" % (i + 1, i + 1) for i in range(N)], compression=1)
    for name, sx in (("x.sample", sex), ("x0.sample", np.zeros(N, int))):
        with open(os.path.join(d, name), "w") as f:
            f.write("ID_1 ID_2 missing sex\n0 0 0 D\n")
            for i in range(N):
                f.write("%d %d 0 %s\n" % (i + 1, i + 1, "NA" if sx[i] == 0 else str(sx[i])))
    ids = ["%d_%d" % (i + 1, i + 1) for i in range(N)]
    with open(os.path.join(d, "pred.list"), "w") as pl:
        for k in range(1, P + 1):
            fn = os.path.join(d, "x_%d.loco" % k)
            cc.write_loco(fn, ids, 500 + k)
            pl.write("Y%d %s\n" % (k, fn))
    return g, gh


def bgen_dosage_255(g):
    """The integer dosages (units of 1 / 255) write_inputs stored in x.bgen; -1 missing."""
    from tests.util import u01
    jj, ii = np.arange(M)[:, None], np.arange(N)[None, :]
    built = np.zeros(M, bool)
    built[DROP + FLIP + F50] = True
    soft = (u01(900 + SEED, jj, ii) < 0.33) & (g == 2) & ~built[:, None]
    amt = (u01(901 + SEED, jj, ii) * 60).astype(np.int64)
    q = np.where(g == 2, 510, np.where(g == 1, 255, 0)).astype(np.int64)
    q[soft] -= amt[soft]                                                             # 2 (255 - a) + a
    return np.where(g < 0, -1, q)


_Q = ["--phenoFile", "{D}/xq.pheno", "--covarFile", "{D}/xq.covar", "--pred", "{D}/pred.list", "--bsize", "150", "--qt"]
_B = ["--bed", "{D}/xb", "--phenoFile", "{D}/xb.pheno", "--covarFile", "{D}/xb.covar", "--pred", "{D}/pred.list", "--bsize", "150", "--bt"]
CASES = {
    "a_qt_bed_missing": ["--bed", "{D}/xq", "--par-region", "hg19"] + _Q,
    "b_qt_pgen_ref_first": ["--pgen", "{D}/xp", "--ref-first", "--par-region", "b37"] + _Q,
    "c_qt_bgen": ["--bgen", "{D}/x.bgen", "--sample", "{D}/x.sample", "--par-region", "hg19"] + _Q,
    "d_bt_firth": _B + ["--firth", "--approx", "--pThresh", "0.9", "--par-region", "hg19"],
    "p_bt_score": _B + ["--par-region", "hg19"],                                      # no correction: tells which rows of (d) / (e) a correction re-tests
    "e_bt_spa": _B + ["--spa", "--par-region", "hg19"],
    "f_ct": ["--bed", "{D}/xc", "--phenoFile", "{D}/xc.pheno", "--covarFile", "{D}/xc.covar", "--pred", "{D}/pred.list", "--bsize", "150", "--ct", "--par-region", "hg19"],
    "g_qt_rec": ["--bed", "{D}/xq", "--test", "recessive", "--par-region", "hg19"] + _Q,
    "h_qt_custom": ["--bed", "{D}/xq", "--par-region", "5000000,100000000"] + _Q,
    "i_qt_het_male": ["--bed", "{D}/xh", "--par-region", "hg19"] + _Q,
    # sex codes 0: the autosomal rule on every variant
    "a0_qt_bed_nosex": ["--bed", "{D}/xq0", "--par-region", "hg19"] + _Q,
    "b0_qt_pgen_nosex": ["--pgen", "{D}/xp0", "--ref-first", "--par-region", "b37"] + _Q,
    "c0_qt_bgen_nosex": ["--bgen", "{D}/x.bgen", "--sample", "{D}/x0.sample", "--par-region", "hg19"] + _Q,
}
SEX_CASES = [c for c in CASES if c[1] == "_"]
NOSEX_OF = {"a_qt_bed_missing": "a0_qt_bed_nosex", "b_qt_pgen_ref_first": "b0_qt_pgen_nosex", "c_qt_bgen": "c0_qt_bgen_nosex"}
SCORE_OF = {"d_bt_firth": "p_bt_score"}
PTHRESH = {"d_bt_firth": 0.9, "e_bt_spa": 0.05}


def build_of(name):
    a = CASES[name]
    return a[a.index("--par-region") + 1]


def args_of(name, D):
    return ["--step", "2"] + [a.replace("{D}", D) for a in CASES[name]]


def golden(name, k):
    return gzip.open(os.path.join(REF, name, "out_Y%d.regenie.gz" % k), "rt").read().splitlines()


def meta(name):
    import json
    return json.load(open(os.path.join(REF, name, "meta.json")))


# ---- the restatement of the rule (parseSnpfromBed and its like + compute_mac, Geno.cpp:3077-3108) ----------------------------------------------
def mac_rule(G, sex, masks, npar):
    """G [M][n] genotype values (NaN missing) of the analysed samples, sex [n], masks [n][P] bool (trait observed), npar [M] bool.
    -> dict of [M] / [M][P] arrays: autosomal and sex-aware MAC over all analysed samples and per trait."""
    obs = ~np.isnan(G)
    g = np.where(obs, G, 0.0)
    male = (sex == 1)[None, :]
    w = np.where(male & npar[:, None], 0.5, 1.0)
    out = {}
    for key, m in [("all", np.ones((G.shape[1], 1), bool))] + [("trait", masks)]:
        tot = np.stack([(g * m[:, q][None, :]).sum(axis=1) for q in range(m.shape[1])], axis=1)
        mac = np.stack([(g * w * m[:, q][None, :]).sum(axis=1) for q in range(m.shape[1])], axis=1)
        ns = np.stack([(obs & m[:, q][None, :]).sum(axis=1) for q in range(m.shape[1])], axis=1).astype(float)
        nm = np.stack([(obs & male & npar[:, None] & m[:, q][None, :]).sum(axis=1) for q in range(m.shape[1])], axis=1).astype(float)
        out["auto_" + key] = np.minimum(tot, 2 * ns - tot)
        out["sex_" + key] = np.minimum(mac, 2 * ns - nm - mac)
    return out


def analysed(pheno_path):
    """-> in_analysis [N] (a sample without any phenotype leaves the analysis), masks [N][P]."""
    rows = [ln.split() for ln in open(pheno_path)][1:]
    masks = np.array([[v != "NA" for v in r[2:]] for r in rows])
    return masks.any(axis=1), masks


def expected_sets(name, D, g, gh):
    """Per trait, the ids the sex-aware rule keeps and the ids only the autosomal rule keeps, for the inputs of case `name` in directory D."""
    a = CASES[name]
    ph = a[a.index("--phenoFile") + 1].replace("{D}", D)
    ia, masks = analysed(ph)
    if "--bgen" in a:
        q = bgen_dosage_255(g)
        G = np.where(q < 0, np.nan, q / 255.0)
    else:
        gg = gh if "{D}/xh" in a else g
        G = np.where(gg < 0, np.nan, gg.astype(float))
    sex = sexes() if name[1] == "_" else np.zeros(N, int)
    r = mac_rule(G[:, ia], sex[ia], masks[ia], non_par(build_of(name)))
    keep, flipped = [], []
    for k in range(P):
        v_ok = r["sex_all"][:, 0] >= MIN_MAC
        keep.append({"s%d" % j for j in range(M) if v_ok[j] and r["sex_trait"][j, k] >= MIN_MAC})
        flipped.append({"s%d" % j for j in range(M) if r["auto_all"][j, 0] >= MIN_MAC and r["auto_trait"][j, k] >= MIN_MAC and ("s%d" % j) not in keep[k]})
    r["keep"], r["auto_only"] = keep, flipped
    return r
