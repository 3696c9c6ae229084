"""The reference cases of the LD mode (`--step 2 --compute-corr`): the command lines, and the generator of the synthetic inputs --
one definition for tests/golden/make_ld_ref_outputs.py (which runs regenie itself on them) and for the tests (which run the driver)."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "tests", "golden", "example")
REF = os.path.join(ROOT, "tests", "golden", "ref_outputs", "ld")


def pack_rows(G):
    """[M][n] calls {0, 1, 2, nan} counting the FIRST .bim allele -> .bed rows."""
    miss = np.isnan(G)
    code = np.where(miss, 1, np.where(G == 2, 0, np.where(G == 1, 2, 3))).astype(np.uint8)
    M, n = G.shape
    code = np.concatenate([code, np.zeros((M, (-n) % 4), np.uint8)], axis=1).reshape(M, -1, 4)
    return (code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6)).astype(np.uint8)


def write_synth(prefix, seed=20240611):
    """600 samples, chromosomes 1 / 2 / 3 with 120 / 300 / 80 variants; chromosome 2 has 2 % missing calls, one monomorphic variant (its 201st)
    and one variant observed in two samples only (its 251st); a covariate file with NAs; 40 samples to remove.  Returns the calls [M][n]."""
    rng = np.random.default_rng(seed)
    n, chroms = 600, [1] * 120 + [2] * 300 + [3] * 80
    M = len(chroms)
    maf = rng.uniform(0.05, 0.5, size=M)
    G = rng.binomial(2, maf[:, None], size=(M, n)).astype(np.float64)
    for j in range(1, M):          # some LD between neighbours
        if rng.random() < 0.5:
            cp = rng.random(n) < 0.7
            G[j, cp] = G[j - 1, cp]
    c2 = 120
    G[c2:c2 + 300][rng.random((300, n)) < 0.02] = np.nan
    G[c2 + 200] = 1.0                                  # monomorphic, no missing call
    G[c2 + 250] = np.nan
    G[c2 + 250, [17, 402]] = [1.0, 2.0]                # observed in two samples only
    with open(prefix + ".bed", "wb") as f:
        f.write(bytes([0x6c, 0x1b, 0x01]))
        f.write(pack_rows(G).tobytes())
    with open(prefix + ".bim", "w") as f:
        for j, c in enumerate(chroms):
            f.write("%d\ts%d\t0\t%d\tA\tG\n" % (c, j + 1, 1000 + 10 * j))
    with open(prefix + ".fam", "w") as f:
        for i in range(n):
            f.write("%d %d 0 0 0 -9\n" % (i + 1, i + 1))
    cov = rng.normal(size=(n, 3))
    with open(prefix + ".covar", "w") as f:
        f.write("FID IID V1 V2 V3\n")
        for i in range(n):
            v = ["%.6f" % x for x in cov[i]]
            if i % 37 == 5:
                v[i % 3] = "NA"
            f.write("%d %d %s\n" % (i + 1, i + 1, " ".join(v)))
    with open(prefix + ".remove", "w") as f:
        for i in rng.choice(n, 40, replace=False):
            f.write("%d %d\n" % (i + 1, i + 1))
    with open(prefix + ".extract150", "w") as f:       # the first 150 variants of chromosome 2 (the degenerate two come later: their correlations
        for j in range(c2, c2 + 150):                  # are rounding noise over rounding noise, which six printed digits cannot pin)
            f.write("s%d\n" % (j + 1))
    return G, chroms


def example_ids(k=None):
    ids = [ln.split()[1] for ln in open(os.path.join(EX, "example.bim"))]
    return ids if k is None else ids[:k]


def write_lists(d):
    """The --extract files of cases 1 and 2."""
    ids = example_ids()
    with open(os.path.join(d, "first400.txt"), "w") as f:
        f.write("\n".join(ids[:400]) + "\n")
    rng = np.random.default_rng(7)
    pick = [ids[i] for i in rng.permutation(len(ids))[:150]]
    pick.insert(10, "absent_A"); pick.insert(77, "absent_B"); pick.append("absent_C")
    with open(os.path.join(d, "forced153.txt"), "w") as f:
        f.write("\n".join(pick) + "\n")


# name -> arguments ({E} example dir, {S} synthetic prefix, {D} the directory of the lists); every case runs with --step 2 --bsize 100
CASES = {
    "c1_example400_bin": ["--bed", "{E}/example", "--covarFile", "{E}/covariates.txt", "--extract", "{D}/first400.txt", "--compute-corr"],
    "c2_forced153_txt": ["--bed", "{E}/example", "--covarFile", "{E}/covariates.txt", "--extract", "{D}/forced153.txt", "--forcein-vars", "--output-corr-text"],
    "c3_synth_chr2_bin": ["--bed", "{S}", "--covarFile", "{S}.covar", "--remove", "{S}.remove", "--chr", "2", "--compute-corr"],
    "c3_synth_chr2_txt": ["--bed", "{S}", "--covarFile", "{S}.covar", "--remove", "{S}.remove", "--chr", "2", "--extract", "{S}.extract150", "--output-corr-text"],
    "c4_range": ["--bed", "{E}/example_3chr", "--range", "2:1-300", "--compute-corr"],
    "c4_chrlist_fails": ["--bed", "{E}/example_3chr", "--chrList", "1,3", "--compute-corr"],
}


def args_of(name, S, D):
    return ["--step", "2", "--bsize", "100"] + [a.replace("{E}", EX).replace("{S}", S).replace("{D}", D) for a in CASES[name]]


def read_bed(prefix):
    """-> calls [M][n_file] (nan = missing) counting the first .bim allele, variant ids, chromosomes, positions, sample ids."""
    bim = [ln.split() for ln in open(prefix + ".bim")]
    fam = [ln.split() for ln in open(prefix + ".fam")]
    n, M = len(fam), len(bim)
    raw = np.fromfile(prefix + ".bed", dtype=np.uint8)[3:].reshape(M, (n + 3) // 4)
    c = np.stack([(raw >> s) & 3 for s in (0, 2, 4, 6)], axis=-1).reshape(M, -1)[:, :n]
    G = np.where(c == 1, np.nan, np.where(c == 0, 2.0, np.where(c == 2, 1.0, 0.0)))
    return G, [b[1] for b in bim], [int(b[0]) for b in bim], [int(b[3]) for b in bim], [(f[0], f[1]) for f in fam]


def dense_case(name, S, D):
    """The dense inputs of print_ld for a case: G [n][M] over the analysed samples with the columns in output order (a forced-in column
    is zero), X [n][C], params.n_samples, the column ids."""
    a = args_of(name, S, D)
    opt = {a[i]: a[i + 1] for i in range(len(a) - 1) if a[i].startswith("--")}
    G, ids, chroms, pos, fam = read_bed(opt["--bed"])
    keep = np.ones(len(fam), bool)
    if "--remove" in opt:
        rm = {tuple(ln.split()[:2]) for ln in open(opt["--remove"])}
        keep = np.array([f not in rm for f in fam])
    fam_k = [f for f, k in zip(fam, keep) if k]
    n_samples = len(fam_k)
    cov, ok = None, np.ones(n_samples, bool)
    if "--covarFile" in opt:
        rows = {}
        for ln in list(open(opt["--covarFile"]))[1:]:
            t = ln.split()
            rows[(t[0], t[1])] = t[2:]
        ok = np.array([f in rows and "NA" not in rows[f] for f in fam_k])
        cov = np.array([[float(v) for v in rows[f]] for f, k in zip(fam_k, ok) if k])
    vkeep = np.ones(len(ids), bool)
    if "--chr" in opt:
        vkeep &= np.array(chroms) == int(opt["--chr"])
    if "--extract" in opt:
        order = []
        for ln in open(opt["--extract"]):
            if ln.split() and ln.split()[0] not in order:
                order.append(ln.split()[0])
        vkeep &= np.isin(ids, order)
    Gk = G[:, keep][:, ok]
    idx = {ids[j]: j for j in range(len(ids)) if vkeep[j]}
    cols = order if "--forcein-vars" in a else [ids[j] for j in range(len(ids)) if vkeep[j]]
    n = Gk.shape[1]
    Gd = np.zeros((n, len(cols)))
    for c, vid in enumerate(cols):
        if vid in idx:
            Gd[:, c] = Gk[idx[vid]]
    from tests.ld_restate import covar_basis
    return Gd, covar_basis(cov, n), n_samples, cols
