"""Conditional analysis (`--step 2 --condition-list`) where no GPU is needed: the option parser's messages, the errors that end a run before the device
comes in, the conditioning columns of the host preparation (regenie_amd/host/driver_inputs.cpp condition_variants, compiled with g++ without the
device library as tests/test_host_prep_cpu.py does) against a numpy restatement of the reference's read_snp / read_snps_* with mean imputation, and
one case end to end through the host-emulated driver build of tests/hipcpu/emubuild.py against regenie's own files."""
import ctypes as C
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from tests import condtl_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "regenie_amd", "bin", "regenie-amd")


@pytest.fixture(scope="module", autouse=True)
def _built():
    from regenie_amd import build
    build.build()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("condtl"))
    return d, cc.write_inputs(d)


def _run(args, cwd):
    return subprocess.run([BIN] + args + ["--out", "o"], cwd=str(cwd), capture_output=True, text=True, timeout=120)


def _error(r):
    lines = [ln for ln in (r.stdout + r.stderr).splitlines() if ln.startswith("ERROR: ")]
    assert r.returncode == 1 and len(lines) == 1, r.stdout[-2000:] + r.stderr[-2000:]
    return lines[0][len("ERROR: "):]


# ---- the parser: one case per message (Regenie.cpp:714-722, :1159-1160, :1350-1363) --------------------------------------------------------
def test_parser_messages(inputs, tmp_path):
    D, _ = inputs
    base = cc.args_of("a_qt_bed", D)
    i = base.index("--condition-list")
    plain, lst = base[:i] + base[i + 2:], base[i + 1]
    T = os.path.join(D, "second")
    cases = [
        (plain + ["--condition-file", "bed," + T], "must use --condition-list if using --condition-file."),
        (base + ["--condition-file", T], "invalid option input for --condition-file"),
        (base + ["--condition-file", "bed," + T + ",x"], "invalid option input for --condition-file"),
        (base + ["--condition-file", "vcf," + T], "invalid file format for --condition-file (either bed/bge/pgen)"),
        (plain + ["--condition-list", os.path.join(D, "absent.txt")], os.path.join(D, "absent.txt") + " doesn't exist for option --condition-list"),
        (base + ["--condition-file", "bed," + os.path.join(D, "absent")], os.path.join(D, "absent.bed") + " doesn't exist for option --condition-file"),
        (base + ["--condition-file", "pgen," + os.path.join(D, "syn")], os.path.join(D, "syn.pgen") + " doesn't exist for option --condition-file"),
        (base + ["--condition-file", "bgen," + os.path.join(D, "absent.bgen")], os.path.join(D, "absent.bgen") + " doesn't exist for option --condition-file"),
        (base + ["--condition-file", "bgen," + T + ".bgen", "--condition-file-sample", os.path.join(D, "absent.sample")],
         os.path.join(D, "absent.sample") + " doesn't exist for option --condition-file-sample"),
        (base + ["--condition-file", "bed," + T, "--condition-file-sample", T + ".sample"], "--condition-file-sample goes with --condition-file bgen,FILE."),
    ]
    for args, message in cases:
        assert _error(_run(args, tmp_path)) == message, args
    s1 = ["--step", "1", "--bed", os.path.join(cc.EX, "example_3chr"), "--phenoFile", os.path.join(cc.EX, "phenotype.txt"), "--bsize", "100", "--condition-list", lst]
    msg = _error(_run(s1, tmp_path))
    assert msg.startswith("--condition-list in step 1") and "is not built" in msg
    assert _run(base + ["--max-condition-vars"], tmp_path).returncode == 1


# ---- errors of the list and of the look-up: they end the run before the device comes in ------------------------------------------------------
@pytest.mark.parametrize("name", cc.ERROR_CASES)
def test_errors_of_the_reference(inputs, tmp_path, name):
    meta = json.load(open(os.path.join(cc.REF, name, "meta.json")))
    r = _run(cc.args_of(name, inputs[0]), tmp_path)
    assert "ERROR: " + _error(r) == meta["error"][0] and r.returncode == meta["returncode"]


def test_errors_of_the_list_and_the_cap(inputs, tmp_path):
    D, _ = inputs
    base = cc.args_of("a_qt_bed", D)
    i = base.index("--condition-list")

    def with_list(text, extra=()):
        fn = str(tmp_path / "list.txt")
        open(fn, "w").write(text)
        return base[:i] + ["--condition-list", fn] + base[i + 2:] + list(extra)
    assert _error(_run(with_list(""), tmp_path)) == "no variants for conditional analysis given in file " + str(tmp_path / "list.txt")
    assert _error(_run(with_list("nobody\nnothing\n"), tmp_path)) == "none of the variants were found in the genotype file"
    assert _error(_run(with_list("inf_120\nmog_3\n"), tmp_path)) == "1 of the variants could not be found in the genotype file"      # mog_3: chromosome 1, --chr 2
    assert _error(_run(with_list("inf_120\n\ninf_75\n"), tmp_path)) == "incorrectly formatted file (" + str(tmp_path / "list.txt") + ")"
    # a second file that lacks one variant, or every sample of the run
    h = cc.args_of("h_file_bed", D)
    j = h.index("--condition-list")
    open(str(tmp_path / "l2.txt"), "w").write("s130\ns131\n")
    assert _error(_run(h[:j] + ["--condition-list", str(tmp_path / "l2.txt")] + h[j + 2:], tmp_path)) == "1 of the variants could not be found in the genotype file"
    open(str(tmp_path / "l3.txt"), "w").write("s131\n")
    assert _error(_run(h[:j] + ["--condition-list", str(tmp_path / "l3.txt")] + h[j + 2:], tmp_path)) == "none of the conditional variants were found in the genotype file"
    for ext in (".bed", ".bim"):
        os.symlink(os.path.join(D, "second" + ext), str(tmp_path / ("other" + ext)))
    with open(str(tmp_path / "other.fam"), "w") as f:
        f.write("".join("x%d x%d 0 0 0 -9\n" % (k, k) for k in range(cc.SYN["N"] + cc.N_EXTRA)))
    k = h.index("--condition-file")
    assert _error(_run(h[:k] + ["--condition-file", "bed," + str(tmp_path / "other")] + h[k + 2:], tmp_path)) == "none of the analyzed samples are present in the file"
    # the cap: 62 covariates + 3 conditioning variants + the intercept
    c = list(base)
    c[c.index("--covarFile") + 1] = os.path.join(D, "ex_cov62.txt")
    msg = _error(_run(c, tmp_path))
    assert "62 covariates" in msg and "3 conditioning variants" in msg and "at most 64" in msg
    assert not [fn for fn in os.listdir(str(tmp_path)) if fn.endswith(".regenie")]


# ---- the conditioning columns against numpy --------------------------------------------------------------------------------------------------
HARNESS = r'''
#include "driver.h"
extern "C" const char* rg_last_error(const rg_ctx*) { return "no device library in this harness"; }
using namespace rgdrv;
static std::string g_err;
static std::vector<double> g_cols, g_X;
static std::vector<std::string> g_ids;
extern "C" const char* ct_error() { return g_err.c_str(); }
static void quiet(const std::function<void()>& fn) {      // the run's log lines go to <out>.log only
  std::cout.flush(); fflush(stdout);
  const int saved = dup(1), nul = open("/dev/null", O_WRONLY);
  dup2(nul, 1); close(nul);
  try { fn(); g_err.clear(); } catch (const std::exception& e) { g_err = e.what(); }
  std::cout.flush(); fflush(stdout); dup2(saved, 1); close(saved); sout.f.close();
}
// parse_args + read_bim_fam + condition_variants on a lone intercept with the given covariate-data mask: out[0] = N, out[1] = columns
extern "C" int ct_columns(int argc, char** argv, const uint8_t* in_cov, int64_t* out) {
  quiet([&]() {
    Run r;
    r.p = parse_args(argc, argv);
    sout.f.open(r.p.out + ".log");
    read_bim_fam(r);
    std::vector<uint8_t> m(in_cov, in_cov + r.N);
    std::vector<double> Xraw((size_t)r.N, 1.0);
    int ncols = 1;
    condition_variants(r, m, Xraw, ncols);
    g_cols.assign(Xraw.begin() + r.N, Xraw.end());
    g_ids.clear();
    for (auto& kv : r.cond_snps) g_ids.push_back(kv.first);
    out[0] = r.N; out[1] = ncols - 1; out[2] = (int64_t)r.snp_ids.size();
    for (auto& id : r.snp_ids) if (r.cond_snps.count(id)) out[2] = -1;      // a conditioning variant left among the tested ones
  });
  return g_err.empty() ? 0 : -1;
}
// the whole preparation: out[0] = N, out[1] = C (columns of the orthonormal basis), out[2] = n_cond
extern "C" int ct_basis(int argc, char** argv, int64_t* out) {
  quiet([&]() {
    Run r;
    r.p = parse_args(argc, argv);
    sout.f.open(r.p.out + ".log");
    read_bim_fam(r);
    read_pheno_cov(r);
    g_X = r.X;
    out[0] = r.N; out[1] = r.C; out[2] = r.n_cond;
  });
  return g_err.empty() ? 0 : -1;
}
extern "C" const double* ct_cols() { return g_cols.data(); }
extern "C" const double* ct_X() { return g_X.data(); }
extern "C" const char* ct_id(int k) { return g_ids[k].c_str(); }
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("condtlprep")
    (d / "h.cpp").write_text(HARNESS)
    so = d / "libct.so"
    host, csrc = os.path.join(ROOT, "regenie_amd", "host"), os.path.join(ROOT, "regenie_amd", "csrc")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-w", "-I" + host] + [os.path.join(host, f) for f in ("driver_common.cpp", "driver_inputs.cpp", "driver_models.cpp")]
                       + [os.path.join(csrc, f) for f in ("pgen_api.cpp", "bgen_api.cpp")] + [str(d / "h.cpp"), "-o", str(so), "-lz", "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(str(so))
    L.ct_cols.restype = L.ct_X.restype = C.c_void_p
    L.ct_error.restype = L.ct_id.restype = C.c_char_p
    return L


def _argv(args):
    return C.c_int(len(args) + 1), (C.c_char_p * (len(args) + 1))(b"regenie-amd", *[a.encode() for a in args])


def columns(L, args, in_cov):
    out = (C.c_int64 * 3)()
    m = np.ascontiguousarray(in_cov, np.uint8)
    rc = L.ct_columns(*_argv(args), m.ctypes.data_as(C.c_void_p), out)
    assert rc == 0, L.ct_error().decode()
    N, nc, left = int(out[0]), int(out[1]), int(out[2])
    cols = np.ctypeslib.as_array(C.cast(L.ct_cols(), C.POINTER(C.c_double)), shape=(nc * N,)).copy().reshape(nc, N)
    return cols, [L.ct_id(C.c_int(k)).decode() for k in range(nc)], left


def impute(raw, in_cov):
    """read_snp with mean imputation (Geno.cpp:3988-3992) / mean_impute_g (:3190-3193): raw [N] with -3 = no call; the mean runs over the samples with
    covariate data that have a call, samples without covariate data get 0."""
    raw = np.asarray(raw, np.float64)
    ok = in_cov & (raw != -3)
    mu = raw[ok].sum() / ok.sum()
    return np.where(in_cov, np.where(raw == -3, mu, raw), 0.0)


def _in_cov(n, seed):
    m = np.ones(n, bool)
    m[np.random.default_rng(seed).choice(n, n // 15, replace=False)] = False
    return m


def _bed_calls(prefix):
    from tests.ld_cases import read_bed
    G, ids, _, _, fam = read_bed(prefix)
    return np.where(np.isnan(G), -3.0, G), ids, ["%s_%s" % f for f in fam]


def _common(D, tmp_path, extra):
    return ["--step", "2", "--phenoFile", os.path.join(D, "syn.pheno"), "--pred", "unused", "--bsize", "100", "--out", str(tmp_path / "o")] + extra


@pytest.mark.parametrize("ref_first", [False, True])
def test_columns_from_the_main_bed_file(lib, inputs, tmp_path, ref_first):
    """example_3chr with 17 missing calls in one conditioning variant; the list in file order 75, 120, 260 comes out in id order 120, 260, 75; the calls
    count the first .bim allele, the other one with --ref-first (read_snp_bed, Geno.cpp:4023)."""
    D, _ = inputs
    G, ids, _ = _bed_calls(os.path.join(D, "ex3m"))
    m = _in_cov(G.shape[1], 1)
    args = ["--step", "2", "--bed", os.path.join(D, "ex3m"), "--phenoFile", os.path.join(cc.EX, "phenotype.txt"), "--pred", "unused", "--bsize", "100", "--chr", "2",
            "--condition-list", os.path.join(D, "cond_ex_shuffled.txt"), "--out", str(tmp_path / "o")] + (["--ref-first"] if ref_first else [])
    cols, names, left = columns(lib, args, m)
    assert names == sorted(cc.EX_COND) == cc.EX_COND and left == 397
    nmiss = 0
    for c, v in zip(cols, names):
        raw = G[ids.index(v)]
        nmiss += int((raw == -3).sum())
        raw = np.where((raw != -3) & ref_first, 2 - raw, raw)
        assert np.array_equal(c, impute(raw, m)), v
    assert nmiss == cc.EX_MISSING[1]


@pytest.mark.parametrize("fmt", ["pgen", "bgen", "bgen_ref_first"])
def test_columns_from_the_main_dosage_files(lib, inputs, tmp_path, fmt):
    """.pgen with a dosage track: PgenReader::Read's values, --ref-first or not; BGEN: the dosage of the first allele, of the second with --ref-first."""
    from oracle import bgen as obg, pgen as opg
    D, g = inputs
    m = _in_cov(cc.SYN["N"], 2)
    if fmt == "pgen":
        src, rd = ["--pgen", os.path.join(D, "syn_p"), "--ref-first"], opg.PgenOracle(os.path.join(D, "syn_p.pgen"))
        raw_of = lambda j: rd.dosages(j)                      # noqa: E731
    else:
        src, rd = ["--bgen", os.path.join(D, "syn.bgen"), "--sample", os.path.join(D, "syn.sample")] + (["--ref-first"] if fmt == "bgen_ref_first" else []), obg.BgenOracle(os.path.join(D, "syn.bgen"))
        raw_of = lambda j: np.nan_to_num(np.asarray(rd.dosages(j, ref_first=fmt == "bgen_ref_first"), np.float64), nan=-3.0)      # noqa: E731
    cols, names, left = columns(lib, _common(D, tmp_path, src + ["--chr", "2", "--condition-list", os.path.join(D, "cond_syn.txt")]), m)
    assert names == cc.SYN_COND and left == 197
    soft = 0
    for c, v in zip(cols, names):
        raw = np.asarray(raw_of(int(v[1:])), np.float64)
        raw = np.where(raw < 0, -3.0, raw)
        assert (raw == -3).sum() > 0
        soft += int(((raw != np.round(raw)) & (raw != -3)).sum())
        assert np.allclose(c, impute(raw, m), rtol=1e-14, atol=0), v
    assert soft > 100                                         # genuine dosages


@pytest.mark.parametrize("fmt", ["bed", "pgen", "bgen"])
def test_columns_from_a_second_file_with_permuted_samples(lib, inputs, tmp_path, fmt):
    """--condition-file: 650 samples in another order, 8 variants in another order; the columns follow the run's samples and the ids' order, the calls
    are the file's own (first .bim allele / ALT / first BGEN allele) with or without --ref-first, and samples of the run the file lacks get the mean."""
    from oracle import bgen as obg
    D, g = inputs
    n = cc.SYN["N"]
    m = _in_cov(n, 3)
    T = os.path.join(D, "second")
    G2, vids, fids = _bed_calls(T)
    if fmt == "bgen":
        rd = obg.BgenOracle(T + ".bgen")
        G2 = np.array([np.nan_to_num(np.asarray(rd.dosages(j), np.float64), nan=-3.0) for j in range(len(vids))])
        assert ((G2 != np.round(G2)) & (G2 >= 0)).sum() > 100
    where = {f: i for i, f in enumerate(fids)}
    # --remove shrinks the run: the columns are indexed by the run's samples, not by the main file's
    with open(str(tmp_path / "rm.txt"), "w") as f:
        f.write("".join("%d %d\n" % (k, k) for k in range(5, 45)))
    keep = np.array([not (5 <= k + 1 < 45) for k in range(n)])
    second = {"bed": ["--condition-file", "bed," + T], "pgen": ["--condition-file", "pgen," + T],
              "bgen": ["--condition-file", "bgen," + T + ".bgen", "--condition-file-sample", T + ".sample"]}[fmt]
    args = _common(D, tmp_path, ["--bed", os.path.join(D, "syn"), "--ref-first", "--remove", str(tmp_path / "rm.txt"), "--chr", "2",
                                 "--condition-list", os.path.join(D, "cond_syn.txt")] + second)
    cols, names, left = columns(lib, args, m[keep])
    assert names == cc.SYN_COND and left == 197 and cols.shape == (3, int(keep.sum()))
    run_ids = ["%d_%d" % (k + 1, k + 1) for k in range(n) if keep[k]]
    for c, v in zip(cols, names):
        raw = G2[vids.index(v)][[where[s] for s in run_ids]]
        assert np.allclose(c, impute(raw, m[keep]), rtol=1e-14, atol=0), v
        if fmt != "bgen":                                     # the shared samples carry the main file's calls
            assert np.array_equal(raw, g[int(v[1:])][keep].astype(np.float64))


def test_basis_holds_the_conditioning_columns(lib, inputs, tmp_path):
    """The whole preparation of case (a): the orthonormal basis spans the intercept, the three covariates and the three mean-imputed columns."""
    D, _ = inputs
    a = cc.args_of("a_qt_bed", D) + ["--out", str(tmp_path / "o")]
    out = (C.c_int64 * 3)()
    assert lib.ct_basis(*_argv(a), out) == 0, lib.ct_error().decode()
    N, Cc, nc = (int(x) for x in out)
    assert (N, Cc, nc) == (500, 7, 3)
    X = np.ctypeslib.as_array(C.cast(lib.ct_X(), C.POINTER(C.c_double)), shape=(Cc * N,)).copy().reshape(Cc, N).T
    G, ids, _ = _bed_calls(os.path.join(D, "ex3m"))
    cov = np.loadtxt(os.path.join(cc.EX, "covariates.txt"), skiprows=1)[:, 2:]
    want = np.column_stack([np.ones(N), cov] + [impute(G[ids.index(v)], np.ones(N, bool)) for v in cc.EX_COND])
    assert np.abs(X.T @ X - np.eye(Cc)).max() < 1e-9 and np.abs(X @ (X.T @ want) - want).max() < 1e-9 * np.abs(want).max()
    assert "n_cov = 3" in open(str(tmp_path / "o.log")).read()      # the log's covariate count leaves the conditioning variants out


# ---- case (c) end to end on the host-emulated kernels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c_bt_firth", "c_bt_spa"])
def test_binary_trait_case_on_the_emulated_kernels_against_regenie(emulated_driver, inputs, tmp_path, name):
    D, _ = inputs
    r = subprocess.run([emulated_driver] + cc.args_of(name, D) + ["--out", "o"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "    +conditioning on variants in [%s] n_used = 3" % os.path.join(D, "cond_ex.txt") in r.stdout.splitlines()
    for k in (1, 2):
        got = open(str(tmp_path / ("o_Y%d.regenie" % k))).read().splitlines()
        ref = gzip.open(os.path.join(cc.REF, name, "out_Y%d.regenie.gz" % k), "rt").read().splitlines()
        assert len(ref) == 398
        print("condtl %s Y%d on the emulated kernels: %d lines not byte-identical" % (name, k, cc.compare_regenie_files(got, ref, "%s Y%d" % (name, k))))


@pytest.fixture(scope="module")
def emulated_driver(tmp_path_factory):
    from tests.hipcpu.emubuild import build_bt_step2_driver
    return build_bt_step2_driver(str(tmp_path_factory.mktemp("hostbt")))
