"""The reference cases of `--step 2 --bt --af-cc` (A1FREQ_CASES A1FREQ_CONTROLS N_CASES N_CONTROLS): the command lines, the generator of their inputs and
a NumPy restatement of the reference's rule -- one definition for tests/golden/make_afcc_ref_outputs.py (which runs regenie itself) and for the tests
(tests/test_afcc_cpu.py: the restatement against regenie's files; tests/test_afcc_cli_gpu.py: the driver against them).

Data: 400 synthetic samples x 300 variants (tests/util.py's writers), chromosome 22 = s0 .. s99, chromosome 23 = s100 .. s299 on both sides of the PAR
bounds of b37; 2 % of the calls missing; males coded 0 / 2 outside the PAR regions.  Three binary traits: Y1 (30 % cases, 8 % NA), Y2 (25 % cases, 5 % NA,
other samples), Y3 (15 cases, no NA: some variants have no or one carrier among its cases).  The same genotypes come as .bed with sex codes 0 (`ab`:
chromosome X then follows the autosomal rule and needs no --par-region) and with sexes (`ax`: the --par-region case), as a hard-call .pgen, a .pgen with a
dosage track and an 8-bit zlib BGEN.  A quantitative and a count phenotype file serve the modes in which the reference switches the option off.
LOCO files are written here (any prediction is a valid offset of Step 2)."""
import gzip
import os

import numpy as np

from tests import condtl_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "ref_outputs", "af_cc")
N, M, P = 400, 300, 3
CHROMS = [22] * 100 + [23] * 200
PAR_B37 = (2699520, 154931044)
SEED = 97
PREV = (0.30, 0.25)
N_CASES_Y3 = 15
NA_RATE = (0.08, 0.05, 0.0)
COND = ["s11", "s47"]
WARNING = "WARNING: disabling option --af-cc (only for BTs in step 2 in native output format split by trait)."
AFCC_COLS = ("A1FREQ_CASES", "A1FREQ_CONTROLS", "N_CASES", "N_CONTROLS")


def positions():
    p1, p2 = PAR_B37
    pos = list(range(1, 101))
    pos += [int(v) for v in np.linspace(60001, p1, 15)]
    pos += [int(v) for v in np.linspace(p1 + 1, p2 - 1, 170)]
    pos += [int(v) for v in np.linspace(p2, p2 + 300000, 15)]
    return np.array(pos, np.int64)


def non_par():
    pos = positions()
    return (np.array(CHROMS) == 23) & (pos > PAR_B37[0]) & (pos < PAR_B37[1])


def sexes():
    from tests.util import u01
    sex = np.where(u01(911, 0, np.arange(N)) < 0.5, 1, 2)
    sex[[3, 88, 301]] = 0
    return sex


def calls():
    """int8 (M, N), -3 missing."""
    from tests.util import synth_dosages
    g = synth_dosages(M, N, miss_rate=0.02, seed=SEED)
    hemi = np.where(g >= 1, np.int8(2), g)
    return np.where(non_par()[:, None] & (sexes() == 1)[None, :], hemi, g).astype(np.int8)


def phenotypes():
    """-> y [N][P] in {0, 1}, missing [N][P] bool."""
    from tests.util import u01
    i = np.arange(N)
    y = np.zeros((N, P), np.int64)
    for k in range(2):
        y[:, k] = u01(920 + k, 0, i) < PREV[k]
    order = np.argsort(u01(925, 0, i), kind="stable")
    y[order[:N_CASES_Y3], 2] = 1
    miss = np.stack([u01(930 + k, 0, i) < NA_RATE[k] for k in range(P)], axis=1)
    return y, miss


def bgen_dosage_255(g):
    """The integer dosages (units of 1 / 255) tests.util.write_synth_bgen(seed=SEED, soft=0.4) stores for the calls g; -1 missing."""
    from tests.util import u01
    j, i = np.arange(M)[:, None], np.arange(N)[None, :]
    hom, het = np.where(g == 2, 255, 0).astype(np.int64), np.where(g == 1, 255, 0).astype(np.int64)
    smear = u01(301 + SEED, j, i) < 0.4
    a = (u01(302 + SEED, j, i) * 90).astype(np.int64)
    b = (u01(303 + SEED, j, i) * (a + 1)).astype(np.int64)
    s2, s1, s0 = smear & (g == 2), smear & (g == 1), smear & (g == 0)
    hom[s2] -= a[s2]; het[s2] += b[s2]
    het[s1] -= a[s1]; hom[s1] += b[s1]
    het[s0] += b[s0]; hom[s0] += a[s0] - b[s0]
    return np.where(g < 0, -1, 2 * hom + het)


def pgen_dosage_16384(g):
    """The integer dosages (units of 1 / 16384) of tests.util.write_synth_pgen(seed=SEED, soft=0.4); -1 missing."""
    from tests.util import u01
    j, i = np.arange(M)[:, None], np.arange(N)[None, :]
    pick = (u01(401 + SEED, j, i) < 0.4) & (g >= 0)
    delta = (u01(402 + SEED, j, i) * 5000).astype(np.int64)
    val = np.where(g == 0, delta, np.where(g == 2, 32768 - delta, 16384 + delta - 2500))
    return np.where(g < 0, -1, np.where(pick, val, g.astype(np.int64) * 16384))


def write_inputs(d):
    """Writes every input the cases need into directory d; returns the calls."""
    from oracle import pgen as opg
    from tests.util import write_bed_bim, write_plink, write_synth_bgen, write_synth_pgen
    g = calls()
    sex = sexes()
    pos = positions()
    y, miss = phenotypes()
    A = os.path.join(d, "ab")
    write_plink(A, g, CHROMS, P=P, seed=SEED, binary=True)                           # .bed / .bim / .fam (sex 0) / .covar; its .pheno is replaced
    with open(os.path.join(d, "a.pheno"), "w") as f:
        f.write("FID IID Y1 Y2 Y3\n")
        for i in range(N):
            f.write("%d %d %s\n" % (i + 1, i + 1, " ".join("NA" if miss[i, k] else str(y[i, k]) for k in range(P))))
    write_plink(os.path.join(d, "aq"), g, CHROMS, P=P, seed=SEED + 1, missing_pheno=0.05)
    write_plink(os.path.join(d, "ac"), g, CHROMS, P=P, seed=SEED + 2, counts="poisson")
    # the same calls with real positions on chromosome X and the sexes: the --par-region case
    X = os.path.join(d, "ax")
    write_bed_bim(X, g, CHROMS)
    with open(X + ".bim", "w") as f:
        for j in range(M):
            f.write("%d\ts%d\t0\t%d\tA\tG\n" % (CHROMS[j], j, pos[j]))
    with open(X + ".fam", "w") as f:
        for i in range(N):
            f.write("%d %d 0 0 %d -9\n" % (i + 1, i + 1, sex[i]))
    # hard-call .pgen (ALT = A, the allele .bed counts), no sex codes
    T = os.path.join(d, "ap")
    opg.write_pgen_fixed(T + ".pgen", np.where(g < 0, 3, g).astype(np.uint8))
    with open(T + ".pvar", "w") as f:
        f.write("#CHROM\tPOS\tID\tREF\tALT\n")
        for j in range(M):
            f.write("%d\t%d\ts%d\tG\tA\n" % (CHROMS[j], j + 1, j))
    with open(T + ".psam", "w") as f:
        f.write("#FID\tIID\tSEX\n")
        for i in range(N):
            f.write("%d\t%d\tNA\n" % (i + 1, i + 1))
    write_synth_pgen(os.path.join(d, "ad"), g, CHROMS, seed=SEED, soft=0.4)
    write_synth_bgen(os.path.join(d, "a"), g, CHROMS, seed=SEED, soft=0.4)
    with open(os.path.join(d, "cond.txt"), "w") as f:
        f.write("\n".join(COND) + "\n")
    ids = ["%d_%d" % (i + 1, i + 1) for i in range(N)]
    with open(os.path.join(d, "pred.list"), "w") as pl:
        for k in range(1, P + 1):
            fn = os.path.join(d, "a_%d.loco" % k)
            cc.write_loco(fn, ids, 700 + k)
            pl.write("Y%d %s\n" % (k, fn))
    check_inputs(g)
    return g


_C = ["--covarFile", "{D}/ab.covar", "--pred", "{D}/pred.list", "--bsize", "100"]
_B = ["--phenoFile", "{D}/a.pheno"] + _C + ["--bt", "--af-cc"]
_BED, _BGEN = ["--bed", "{D}/ab"], ["--bgen", "{D}/a.bgen", "--sample", "{D}/a.sample"]
CASES = {
    "a_bed": _BED + _B,
    "b_bed_firth": _BED + _B + ["--firth", "--approx"],
    "c_bed_spa": _BED + _B + ["--spa"],
    "d_pgen_rec": ["--pgen", "{D}/ap", "--test", "recessive"] + _B,
    "e_pgen_dosage": ["--pgen", "{D}/ad"] + _B,
    "f_bgen": _BGEN + _B,
    "g_bgen_firth": _BGEN + _B + ["--firth", "--approx"],
    "h_bed_cond": _BED + _B + ["--condition-list", "{D}/cond.txt"],
    "i_bed_par": ["--bed", "{D}/ax", "--par-region", "b37"] + _B,
    # the modes in which the reference switches the option off
    "q_qt": _BED + ["--phenoFile", "{D}/aq.pheno", "--covarFile", "{D}/aq.covar", "--pred", "{D}/pred.list", "--bsize", "100", "--qt", "--af-cc"],
    "r_ct": _BED + ["--phenoFile", "{D}/ac.pheno", "--covarFile", "{D}/ac.covar", "--pred", "{D}/pred.list", "--bsize", "100", "--ct", "--af-cc"],
}
ACTIVE = [c for c in CASES if c[0] not in "qr"]
DISABLED = ["q_qt", "r_ct"]
TWINS = ["a_bed", "f_bgen", "q_qt", "r_ct"]          # regenie is also run on these without the option: <name>_plain


def args_of(name, D, af_cc=True):
    a = [x.replace("{D}", D) for x in CASES[name]]
    if not af_cc:
        a.remove("--af-cc")
    return ["--step", "2"] + a


def golden(name, k):
    return gzip.open(os.path.join(REF, name, "out_Y%d.regenie.gz" % k), "rt").read().splitlines()


def meta(name):
    import json
    return json.load(open(os.path.join(REF, name, "meta.json")))


def genotypes_of(name, g):
    """The additive genotype values regenie reads for case `name` (NaN missing), [M][N], as exact integers and their unit: (q, scale)."""
    a = CASES[name]
    if "--bgen" in a:
        return bgen_dosage_255(g), 255
    if "{D}/ad" in a:
        return pgen_dosage_16384(g), 16384
    return np.where(g < 0, -1, g).astype(np.int64), 1


# ---- the restatement of the rule (update_af_cc, Geno.cpp:3069-3075; compute_aaf_info, :3119-3126) --------------------------------------------
def afcc_sums(q, y, mask):
    """q [M][n] integer genotype values (< 0 missing), y [n][P] in {0, 1}, mask [n][P] bool (trait observed) -> integer arrays [M][P]:
    af_sum, ns (all observed samples of the trait), af_case_sum, ns_case."""
    obs = q >= 0
    v = np.where(obs, q, 0).astype(np.int64)
    m = mask.astype(np.int64)
    c = (mask & (y == 1)).astype(np.int64)
    return v @ m, obs.astype(np.int64) @ m, v @ c, obs.astype(np.int64) @ c


def afcc_columns(q, scale, y, mask):
    """-> text arrays [M][P] of the four columns as the reference prints them (six significant digits; counts as integers)."""
    af, ns, afc, nsc = afcc_sums(q, y, mask)
    with np.errstate(divide="ignore", invalid="ignore"):
        f_case = (afc / float(scale)) / (2.0 * nsc)
        f_ctrl = ((af - afc) / float(scale)) / (2.0 * ns - 2.0 * nsc)
    fmt = np.vectorize(lambda x: "%g" % x)
    return fmt(f_case), fmt(f_ctrl), nsc.astype(str), (ns - nsc).astype(str)


def min_mac_kept(q, scale, mask):
    """[M][P] bool: the test passes regenie's default --minMAC 5 by the autosomal rule."""
    obs = q >= 0
    tot = (np.where(obs, q, 0) @ mask.astype(np.int64)) / float(scale)
    ns = obs.astype(np.int64) @ mask.astype(np.int64)
    return np.minimum(tot, 2.0 * ns - tot) >= 5.0


def check_inputs(g):
    """What the data are built to have: no kept test with zero observed cases or zero observed controls (regenie would print a platform-dependent
    `nan`), variants with 0 and with 1 carrier among Y3's cases, traits that differ in their missing values."""
    y, miss = phenotypes()
    mask = ~miss
    assert mask.any(axis=1).all()                                                    # every sample is analysed
    assert len({tuple(mask[:, k]) for k in range(P)}) == P
    assert (y[:, 2] == 1).sum() == N_CASES_Y3
    for q, scale in ((np.where(g < 0, -1, g).astype(np.int64), 1), (bgen_dosage_255(g), 255), (pgen_dosage_16384(g), 16384)):
        af, ns, afc, nsc = afcc_sums(q, y, mask)
        kept = min_mac_kept(q, scale, mask)
        assert (nsc[kept] > 0).all() and ((ns - nsc)[kept] > 0).all()
    carriers = ((g > 0) & (y[:, 2] == 1)[None, :]).sum(axis=1)
    assert (carriers == 0).sum() >= 3 and (carriers == 1).sum() >= 3


def strip_afcc(lines):
    """The lines of an --af-cc file without its four columns."""
    h = lines[0].split(" ")
    drop = {h.index(c) for c in AFCC_COLS}
    return [" ".join(t for k, t in enumerate(ln.split(" ")) if k not in drop) for ln in lines]
