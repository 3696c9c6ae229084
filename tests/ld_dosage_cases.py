"""The reference cases of the LD mode on dosage input (`--step 2 --compute-corr --bgen`): the command lines and the generator of the
synthetic BGEN -- one definition for tests/golden/make_ld_dosage_ref_outputs.py (which runs regenie itself on them), for
tests/test_ld_dosage_restate_cpu.py (the fp64 restatement against regenie's files) and for tests/test_ld_dosage_cli_gpu.py (the driver)."""
import os

import numpy as np

from tests import ld_cases as lc

ROOT = lc.ROOT
EX = lc.EX
REF = os.path.join(ROOT, "tests", "golden", "ref_outputs", "ld_dosage")


def write_synth(prefix, seed=20250318):
    """600 samples, chromosomes 1 / 2 / 3 with 120 / 300 / 80 variants of genuinely fractional 8-bit probabilities; on chromosome 2
    2 % of the samples are missing per variant and its 201st variant is monomorphic; the same data zlib-compressed (prefix.bgen) and
    uncompressed (prefix_raw.bgen) and zstd-compressed (prefix_zstd.bgen); a covariate file with NAs; 40 samples to remove; an extract of 150 without the monomorphic one."""
    from oracle.bgen import write_bgen
    rng = np.random.default_rng(seed)
    n, chroms = 600, [1] * 120 + [2] * 300 + [3] * 80
    M = len(chroms)
    maf = rng.uniform(0.05, 0.5, size=M)
    g = rng.binomial(2, maf[:, None], size=(M, n))
    for j in range(1, M):          # some LD between neighbours
        if rng.random() < 0.5:
            cp = rng.random(n) < 0.7
            g[j, cp] = g[j - 1, cp]
    conf = rng.uniform(0.55, 1.0, size=(M, n))
    split = rng.uniform(0.0, 1.0, size=(M, n))
    p = np.empty((M, n, 3))
    for k in range(3):
        other = (1 - conf) * np.where((k - g) % 3 == 1, split, 1 - split)
        p[:, :, k] = np.where(g == k, conf, other)
    # probs[..., 0] = P(two copies of the first allele), probs[..., 1] = P(het)
    b0 = np.rint(255 * p[:, :, 2]).astype(np.int64)
    b1 = np.minimum(np.rint(255 * p[:, :, 1]).astype(np.int64), 255 - b0)
    probs = np.stack([b0, b1], axis=-1).astype(np.uint8)
    missing = np.zeros((M, n), bool)
    c2 = 120
    missing[c2:c2 + 300] = rng.random((300, n)) < 0.02
    probs[c2 + 200] = [0, 255]                         # monomorphic (every sample a certain het), no missing sample
    missing[c2 + 200] = False
    variants = [(c, 1000 + 10 * j, "s%d" % (j + 1), "A", "G") for j, c in enumerate(chroms)]
    ids = ["%d_%d" % (i + 1, i + 1) for i in range(n)]
    write_bgen(prefix + ".bgen", probs, missing, variants, sample_ids=ids, compression=1)
    write_bgen(prefix + "_raw.bgen", probs, missing, variants, sample_ids=ids, compression=0)
    rewrite_zstd(prefix + "_raw.bgen", prefix + "_zstd.bgen")
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
    with open(prefix + ".extract150", "w") as f:       # the first 150 variants of chromosome 2: the monomorphic one comes later
        for j in range(c2, c2 + 150):
            f.write("s%d\n" % (j + 1))


def rewrite_zstd(src, dst):
    """An uncompressed BGEN (oracle.bgen.write_bgen, compression 0) with every probability block zstd-compressed (flag bits 2):
    oracle.bgen writes zlib or nothing; libzstd is loaded the way oracle.bgen loads it to read such files."""
    import ctypes
    import struct
    from oracle.bgen import BgenOracle
    lib = ctypes.CDLL("libzstd.so.1")
    lib.ZSTD_compressBound.restype = ctypes.c_size_t
    lib.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
    lib.ZSTD_compress.restype = ctypes.c_size_t
    lib.ZSTD_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    lib.ZSTD_isError.argtypes = [ctypes.c_size_t]
    bg = BgenOracle(src)
    assert bg.compression == 0
    d = bg.data
    offset, lh = struct.unpack_from("<II", d, 0)
    (flags,) = struct.unpack_from("<I", d, lh)
    out = bytearray(d[:4 + offset])
    struct.pack_into("<I", out, lh, (flags & ~3) | 2)
    for v in bg.variants:
        (c,) = struct.unpack_from("<I", d, v["data"])
        blk = d[v["data"] + 4:v["data"] + 4 + c]
        cap = lib.ZSTD_compressBound(len(blk))
        buf = ctypes.create_string_buffer(cap)
        k = lib.ZSTD_compress(buf, cap, blk, len(blk), 3)
        assert not lib.ZSTD_isError(k)
        out += d[v["offset"]:v["data"]] + struct.pack("<II", k + 4, len(blk)) + buf.raw[:k]
    with open(dst, "wb") as f:
        f.write(bytes(out))


def write_cond(d):
    """The --condition-list of case d6: two of the first 400 variants of the example."""
    ids = lc.example_ids()
    with open(os.path.join(d, "cond2.txt"), "w") as f:
        f.write("%s\n%s\n" % (ids[100], ids[250]))


def write_synth_pgen(prefix, seed=20250319):
    """300 samples, 150 variants of chromosome 1 as a .pgen whose every variant carries a dosage track (a 16-bit value per sample):
    multiples of 1 / 16384 that are not multiples of 1 / 255, 1.5 % of the entries missing (no dosage, hard call missing); covariates."""
    from oracle import pgen as opg
    rng = np.random.default_rng(seed)
    m, n = 150, 300
    maf = rng.uniform(0.05, 0.5, size=m)
    g = rng.binomial(2, maf[:, None], size=(m, n))
    for j in range(1, m):
        if rng.random() < 0.5:
            cp = rng.random(n) < 0.7
            g[j, cp] = g[j - 1, cp]
    vals = np.clip(g * 16384 + rng.integers(-6000, 6001, size=(m, n)), 0, 32768)
    vals += (vals % 257 == 0) & (vals < 32768)          # (a multiple of 1 / 255 in these units is a multiple of 16384 / 255: keep off the near ones too)
    miss = rng.random((m, n)) < 0.015
    geno = np.where(miss, 3, np.rint(vals / 16384.0)).astype(np.uint8)
    dosage = {j: (0x40, np.nonzero(~miss[j])[0], vals[j][~miss[j]].astype(np.uint16)) for j in range(m)}
    opg.write_pgen(prefix + ".pgen", geno, [0] * m, wide_vrtypes=True, dosage=dosage)
    opg.write_pvar_psam(prefix, [1] * m, n)
    cov = rng.normal(size=(n, 2))
    with open(prefix + ".covar", "w") as f:
        f.write("FID IID V1 V2\n")
        for i in range(n):
            f.write("%d %d %.6f %.6f\n" % (i + 1, i + 1, cov[i, 0], cov[i, 1]))


# name -> arguments ({E} example dir, {S} synthetic prefix, {D} the directory of the lists); every case runs with --step 2 --bsize 100
CASES = {
    "d1_example400_bin": ["--bgen", "{E}/example.bgen", "--covarFile", "{E}/covariates.txt", "--extract", "{D}/first400.txt", "--compute-corr"],
    "d2_forced153_txt": ["--bgen", "{E}/example.bgen", "--ref-first", "--covarFile", "{E}/covariates.txt", "--extract", "{D}/forced153.txt", "--forcein-vars",
                         "--output-corr-text"],
    "d3_synth_chr2_bin": ["--bgen", "{S}.bgen", "--covarFile", "{S}.covar", "--remove", "{S}.remove", "--chr", "2", "--compute-corr"],
    "d3_synth_chr2_txt": ["--bgen", "{S}.bgen", "--covarFile", "{S}.covar", "--remove", "{S}.remove", "--chr", "2", "--extract", "{S}.extract150",
                          "--output-corr-text"],
    "d6_example400_cond_bin": ["--bgen", "{E}/example.bgen", "--covarFile", "{E}/covariates.txt", "--extract", "{D}/first400.txt", "--compute-corr",
                               "--condition-list", "{D}/cond2.txt"],
    "d5_pgen_bin": ["--pgen", "{S}_pgen", "--covarFile", "{S}_pgen.covar", "--compute-corr"],
    "d5_pgen_txt": ["--pgen", "{S}_pgen", "--covarFile", "{S}_pgen.covar", "--output-corr-text"],
}


def args_of(name, S, D):
    return ["--step", "2", "--bsize", "100"] + [a.replace("{E}", EX).replace("{S}", S).replace("{D}", D) for a in CASES[name]]


def dense_case(name, S, D):
    """The dense inputs of print_ld for a case: G [n][M] dosages over the analysed samples (nan = missing) with the columns in output
    order (a forced-in column is zero), X [n][C], params.n_samples, the column ids."""
    from oracle.bgen import BgenOracle
    from tests.ld_restate import covar_basis
    a = args_of(name, S, D)
    opt = {a[i]: a[i + 1] for i in range(len(a) - 1) if a[i].startswith("--")}
    if "--pgen" in opt:      # every sample and variant kept, covariates without NAs
        from oracle import pgen as opg
        pg = opg.PgenOracle(opt["--pgen"] + ".pgen")
        ids = [ln.split()[2] for ln in list(open(opt["--pgen"] + ".pvar"))[1:]]
        Gd = np.stack([pg.dosages(j) for j in range(len(ids))], axis=1).astype(np.float64)
        Gd = np.where(Gd == -3.0, np.nan, Gd)
        cov = np.array([[float(v) for v in ln.split()[2:]] for ln in list(open(opt["--covarFile"]))[1:]])
        return Gd, covar_basis(cov, Gd.shape[0]), Gd.shape[0], ids
    bg = BgenOracle(opt["--bgen"])
    ids = [v["rsid"] for v in bg.variants]
    chroms = [int(v["chrom"]) for v in bg.variants]
    fam = [tuple(s.split("_")) if "_" in s else (s, s) for s in bg.sample_ids]
    keep = np.ones(len(fam), bool)
    if "--remove" in opt:
        rm = {tuple(ln.split()[:2]) for ln in open(opt["--remove"])}
        keep = np.array([f not in rm for f in fam])
    fam_k = [f for f, k in zip(fam, keep) if k]
    n_samples = len(fam_k)
    rows = {}
    for ln in list(open(opt["--covarFile"]))[1:]:
        t = ln.split()
        rows[(t[0], t[1])] = t[2:]
    ok = np.array([f in rows and "NA" not in rows[f] for f in fam_k])
    cov = np.array([[float(v) for v in rows[f]] for f, k in zip(fam_k, ok) if k])
    vkeep = np.ones(len(ids), bool)
    if "--chr" in opt:
        vkeep &= np.array(chroms) == int(opt["--chr"])
    order = []
    if "--extract" in opt:
        for ln in open(opt["--extract"]):
            if ln.split() and ln.split()[0] not in order:
                order.append(ln.split()[0])
        vkeep &= np.isin(ids, order)
    if "--condition-list" in opt:      # the listed variants become covariates and leave the matrix
        cond = [ln.split()[0] for ln in open(opt["--condition-list"]) if ln.split()]
        extra = []
        for vid in cond:
            dv = bg.dosages(ids.index(vid), ref_first="--ref-first" in a)[keep][ok]
            assert not (dv == -3.0).any()
            extra.append(dv)
        cov = np.column_stack([cov] + extra)
        vkeep &= ~np.isin(ids, cond)
    idx = {ids[j]: j for j in range(len(ids)) if vkeep[j]}
    cols = order if "--forcein-vars" in a else [ids[j] for j in range(len(ids)) if vkeep[j]]
    n = int(ok.sum())
    Gd = np.zeros((n, len(cols)))
    for c, vid in enumerate(cols):
        if vid in idx:
            d = bg.dosages(idx[vid], ref_first="--ref-first" in a)[keep][ok]
            Gd[:, c] = np.where(d == -3.0, np.nan, d)
    return Gd, covar_basis(cov, n), n_samples, cols
