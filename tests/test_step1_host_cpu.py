"""The parts of `--step 1` that make no device call (regenie_amd/host/driver_step1_plan.cpp: plan_step1, split_l0, LocoWriter), compiled with g++
into a harness WITHOUT the device library and held to the oracle (oracle/regenie_step1.py) on the example data: blocks, folds, ridge grids and
penalties of the plan; the .loco / .prs files, table lines and list entries of the writer; the master file and variant lists of --split-l0."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import regenie_step1 as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = os.path.join(ROOT, "tests", "golden", "example")
HARNESS = r'''
#include "driver_step1.h"
extern "C" const char* rg_last_error(const rg_ctx*) { return "no device library in this harness"; }
using namespace rgdrv;
struct H { Run r; Step1Plan pl; std::unique_ptr<LocoWriter> w; int saved = -1; };
static std::string g_err;
static void back(H* h) { std::cout.flush(); fflush(stdout); dup2(h->saved, 1); close(h->saved); sout.f.close(); }
extern "C" const char* s1_error() { return g_err.c_str(); }
extern "C" void* s1_open(int argc, char** argv) {      // rgdrv::run up to the plan (or through --split-l0); the log lines go to <out>.log only
  H* h = new H;
  std::cout.flush(); fflush(stdout);
  h->saved = dup(1);
  const int nul = open("/dev/null", O_WRONLY);
  dup2(nul, 1); close(nul);
  try {
    h->r.p = parse_args(argc, argv);
    sout.f.open(h->r.p.out + ".log");
    read_bim_fam(h->r);
    if (h->r.p.split_l0) { split_l0(h->r); return h; }
    read_pheno_cov(h->r);
    h->pl = plan_step1(h->r);
    return h;
  } catch (const std::exception& e) { g_err = e.what(); back(h); delete h; return nullptr; }
}
extern "C" void s1_close(void* hv) { H* h = (H*)hv; back(h); delete h; }
extern "C" void s1_ints(void* hv, int64_t* o) {
  const Step1Plan& pl = ((H*)hv)->pl;
  o[0] = pl.B; o[1] = pl.M; o[2] = pl.R0; o[3] = pl.R1; o[4] = pl.L; o[5] = pl.use_loocv; o[6] = pl.nchr; o[7] = pl.NCS; o[8] = ((H*)hv)->r.P; o[9] = (int64_t)pl.cv_sizes.size();
}
extern "C" void s1_blocks(void* hv, int64_t* o) { int k = 0; for (auto& b : ((H*)hv)->pl.blocks) { o[k++] = b.chrom; o[k++] = b.start; o[k++] = b.bs; } }
extern "C" const double* s1_dvec(void* hv, int which) { const Step1Plan& pl = ((H*)hv)->pl; return (which == 0 ? pl.h0 : which == 1 ? pl.h1 : which == 2 ? pl.lambda : which == 3 ? pl.tau : pl.ct_rate).data(); }
extern "C" const int32_t* s1_ivec(void* hv, int which) { const Step1Plan& pl = ((H*)hv)->pl; return (which == 0 ? pl.cv_sizes : which == 1 ? pl.cols_per_chr : which == 2 ? pl.bbeg : pl.pbeg).data(); }
extern "C" const int* s1_chroms(void* hv) { return ((H*)hv)->pl.chroms.data(); }
extern "C" int s1_emit(void* hv, int q, const double* cs, int best, int conv, const double* pq) {
  H* h = (H*)hv;
  try { if (!h->w) h->w.reset(new LocoWriter(h->r, h->pl)); h->w->emit(q, cs, best, conv, pq); return 0; } catch (const std::exception& e) { g_err = e.what(); return 1; }
}
extern "C" void s1_lists(void* hv) { ((H*)hv)->w->write_lists(); }
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("step1host")
    src = d / "h.cpp"
    src.write_text(HARNESS)
    so = d / "libs1.so"
    host, csrc = os.path.join(ROOT, "regenie_amd", "host"), os.path.join(ROOT, "regenie_amd", "csrc")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-w", "-I" + host]
                       + [os.path.join(host, f) for f in ("driver_common.cpp", "driver_inputs.cpp", "driver_models.cpp", "driver_step1_plan.cpp")]
                       + [os.path.join(csrc, f) for f in ("pgen_api.cpp", "bgen_api.cpp")] + [str(src), "-o", str(so), "-lz", "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(str(so))
    for f in ("s1_open", "s1_dvec", "s1_ivec", "s1_chroms"):
        getattr(L, f).restype = C.c_void_p
    L.s1_error.restype = C.c_char_p
    return L


def _open(L, args):
    argv = (C.c_char_p * (len(args) + 1))(b"regenie-amd", *[a.encode() for a in args])
    h = L.s1_open(C.c_int(len(args) + 1), argv)
    return (C.c_void_p(h), None) if h else (None, L.s1_error().decode())


def _arr(ptr, n, dt):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(dt)), shape=(n,)).copy() if n else np.zeros(0)


def _plan(L, h):
    o = (C.c_int64 * 10)()
    L.s1_ints(h, o)
    B, M, R0, R1, Lc, loocv, nchr, NCS, P, nfold = [int(x) for x in o]
    blk = (C.c_int64 * (3 * B))()
    L.s1_blocks(h, blk)
    return dict(B=B, M=M, R0=R0, R1=R1, L=Lc, use_loocv=bool(loocv), nchr=nchr, NCS=NCS, P=P,
                blocks=[tuple(int(x) for x in blk[3 * b:3 * b + 3]) for b in range(B)],
                h0=_arr(L.s1_dvec(h, 0), R0, C.c_double), h1=_arr(L.s1_dvec(h, 1), R1, C.c_double), lam=_arr(L.s1_dvec(h, 2), R0, C.c_double),
                tau=_arr(L.s1_dvec(h, 3), P * R1, C.c_double).reshape(P, R1), ct_rate=_arr(L.s1_dvec(h, 4), P, C.c_double),
                cv_sizes=_arr(L.s1_ivec(h, 0), nfold, C.c_int32), cols=_arr(L.s1_ivec(h, 1), nchr, C.c_int32), chroms=_arr(L.s1_chroms(h), nchr, C.c_int))


def _ulp_equal(a, b):      # to the last bit or to 1 ulp
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= np.spacing(np.abs(b))))


def _count_pheno(path, zero_first=0):
    """a count phenotype for the example's samples; its first `zero_first` samples hold zeros"""
    rng = np.random.default_rng(7)
    rows = [ln.split() for ln in open(os.path.join(E, "phenotype.txt")).read().split("\n")[1:] if ln]
    with open(path, "w") as f:
        f.write("FID IID Y1\n")
        for k, t in enumerate(rows):
            f.write("%s %s %d\n" % (t[0], t[1], 0 if k < zero_first else rng.poisson(2.0)))


PLAN_CASES = {
    "bsize100": (dict(bsize=100), []),
    "bsize37": (dict(bsize=37), []),
    "nb5": (dict(bsize=37, n_block=5), ["--nb", "5"]),
    "cv7": (dict(bsize=100, cv_folds=7), ["--cv", "7"]),
    "loocv": (dict(bsize=37, loocv=True), ["--loocv"]),
    "bt_below_5000": (dict(bsize=100, bt=True), ["--bt"]),
    "setl0_setl1": (dict(bsize=100, setl0=[0.5, 0.1, 0.9, 0.5], setl1=[0.75, 0.25, 0.25]), ["--setl0", "0.5,0.1,0.9,0.5", "--setl1", "0.75,0.25,0.25"]),
    "ct": (dict(bsize=37, ct=True), ["--ct"]),
}


@pytest.mark.parametrize("case", sorted(PLAN_CASES))
def test_step1_plan_equals_oracle(lib, tmp_path, case):
    kw, extra = PLAN_CASES[case]
    pheno = os.path.join(E, "phenotype_bin.txt" if kw.get("bt") else "phenotype.txt")
    if kw.get("ct"):
        pheno = str(tmp_path / "counts.txt")
        _count_pheno(pheno)
    opt = orc.Step1Options(bed=os.path.join(E, "example_3chr"), pheno_file=pheno, covar_file=os.path.join(E, "covariates.txt"), **kw)
    bim, chrom, offs, snp_ids, prep = orc.load_inputs(opt)
    h, err = _open(lib, ["--step", "1", "--bed", opt.bed, "--phenoFile", pheno, "--covarFile", opt.covar_file, "--bsize", str(opt.bsize), "--out", str(tmp_path / "o")] + extra)
    assert h is not None, err
    try:
        pl = _plan(lib, h)
    finally:
        lib.s1_close(h)
    blocks = orc.chrom_blocks(chrom, bim.chr_read, opt.bsize, opt.n_block)
    assert pl["blocks"] == [tuple(int(x) for x in b) for b in blocks] and pl["B"] == len(blocks) and pl["M"] == chrom.size
    if case in ("bsize37", "nb5"):
        assert any(b[2] != 37 for b in blocks) or case == "nb5"          # 37 does not divide the chromosomes
    use_loocv = opt.loocv or (opt.bt and prep.n_analyzed < 5000)
    assert pl["use_loocv"] == use_loocv
    if not use_loocv:
        assert np.array_equal(pl["cv_sizes"], orc.set_folds(prep.ind_in_analysis, opt.cv_folds))
    h0 = np.unique(np.asarray(opt.setl0, np.float64)) if opt.setl0 is not None else orc.set_ridge_params(opt.n_ridge_l0)
    h1 = np.unique(np.asarray(opt.setl1, np.float64)) if opt.setl1 is not None else orc.set_ridge_params(opt.n_ridge_l1)
    assert _ulp_equal(pl["h0"], h0) and _ulp_equal(pl["h1"], h1)
    assert _ulp_equal(pl["lam"], chrom.size * (1 - h0) / h0)
    Lc = len(blocks) * h0.size
    assert pl["L"] == Lc and pl["NCS"] == (6 if (opt.bt or opt.ct) else 5)
    for q in range(pl["P"]):
        want = orc.tau_count(h1, Lc, prep.Y_raw[:, q], prep.Neff[q]) if opt.ct else orc.tau_from_h(h1, Lc, opt.bt)
        assert _ulp_equal(pl["tau"][q], want), (case, q)
        if opt.ct:
            assert _ulp_equal(pl["ct_rate"][q], prep.Y_raw[:, q].sum() / prep.Neff[q])
    cc = orc.chr_columns(blocks, bim.chr_read, h0.size)
    assert list(pl["chroms"]) == [c for c, _, _ in cc] and list(pl["cols"]) == [nn for _, _, nn in cc]


def test_step1_plan_errors(lib, tmp_path):
    base = ["--step", "1", "--bed", os.path.join(E, "example_3chr"), "--covarFile", os.path.join(E, "covariates.txt"), "--bsize", "100", "--out", str(tmp_path / "o")]
    h, err = _open(lib, base + ["--phenoFile", os.path.join(E, "phenotype.txt"), "--l0", "1"])
    assert h is None and "number of ridge parameters must be at least 2 (=1)" in err
    zeros = str(tmp_path / "zeros.txt")
    _count_pheno(zeros, zero_first=120)                     # the first of 5 folds (100 samples) holds no count
    h, err = _open(lib, base + ["--phenoFile", zeros, "--ct"])
    assert h is None and err == "one of the folds has only zero counts for phenotype 'Y1'. Either use smaller #folds (option --cv) or use LOOCV (option --loocv)."
    # binary traits take K folds from 5,000 samples on: a synthetic set whose cases all lie in the first half
    from tests.util import synth_dosages, write_plink
    S = str(tmp_path / "big")
    write_plink(S, synth_dosages(40, 5200, miss_rate=0.0, seed=3), [1] * 40, P=1, seed=3, binary=True, missing_pheno=False)
    rows = [ln.split() for ln in open(S + ".pheno").read().split("\n") if ln]
    with open(S + ".pheno", "w") as f:
        f.write(" ".join(rows[0]) + "\n")
        for k, t in enumerate(rows[1:]):
            f.write("%s %s %d\n" % (t[0], t[1], 1 if (k < 2600 and k % 3 == 0) else 0))
    h, err = _open(lib, ["--step", "1", "--bed", S, "--phenoFile", S + ".pheno", "--covarFile", S + ".covar", "--bsize", "20", "--bt", "--out", str(tmp_path / "b")])
    assert h is None and err == "one of the folds has only cases/controls for phenotype '%s'. Either use smaller #folds (option --cv) or use LOOCV (option --loocv)." % rows[0][2]


@pytest.mark.parametrize("bt", [False, True])
def test_loco_writer_equals_oracle(lib, tmp_path, bt):
    """One trait of two, with missing values, a few samples removed, drawn predictions and a drawn cumsum table: the files and lines of the writer."""
    rng = np.random.default_rng(11 + bt)
    pheno = str(tmp_path / "ph.txt")
    if bt:
        pheno = os.path.join(E, "phenotype_bin_wNA.txt")
    else:
        lines = open(os.path.join(E, "phenotype.txt")).read().split("\n")
        with open(pheno, "w") as f:
            f.write("\n".join(ln if k % 17 else " ".join(ln.split()[:2] + ["NA", ln.split()[3]]) for k, ln in enumerate(lines) if ln).replace("FID IID NA", "FID IID Y1") + "\n")
    rm = os.path.join(E, "fid_iid_to_remove.txt")
    opt = orc.Step1Options(bed=os.path.join(E, "example_3chr"), pheno_file=pheno, covar_file=os.path.join(E, "covariates.txt"), bsize=100, bt=bt, remove=[rm])
    bim, chrom, offs, snp_ids, prep = orc.load_inputs(opt)
    assert prep.n_analyzed < len(orc.read_fam(opt.bed + ".fam")) and prep.mask[prep.ind_in_analysis, 0].all() == (not bt)      # (Step 1 imputes a quantitative trait's missing values: no NA there)
    out = str(tmp_path / "w")
    h, err = _open(lib, ["--step", "1", "--bed", opt.bed, "--phenoFile", pheno, "--covarFile", opt.covar_file, "--bsize", "100", "--remove", rm,
                         "--print-prs", "--out", out] + (["--bt"] if bt else []))
    assert h is not None, err
    try:
        pl = _plan(lib, h)
        N, R1, nchr = prep.Y.shape[0], pl["R1"], pl["nchr"]
        blocks = orc.chrom_blocks(chrom, bim.chr_read, 100)
        chrcols = orc.chr_columns(blocks, bim.chr_read, pl["R0"])
        assert nchr == len(chrcols) == 3
        pred = rng.normal(size=(nchr, N)) * 10.0 ** rng.integers(-6, 3, size=(nchr, N))
        y, ph = rng.normal(size=400), rng.normal(size=(R1, 400))
        cs = np.stack([ph.sum(1), np.full(R1, y.sum()), (ph * ph).sum(1), np.full(R1, (y * y).sum()), (ph * y).sum(1), rng.uniform(100, 300, R1)])[:pl["NCS"]]
        best = 3
        csc, pc = np.ascontiguousarray(cs), np.ascontiguousarray(pred)
        assert lib.s1_emit(h, 0, csc.ctypes.data_as(C.c_void_p), best, 1, pc.ctypes.data_as(C.c_void_p)) == 0, lib.s1_error()
        lib.s1_lists(h)
    finally:
        lib.s1_close(h)
    loco = orc.loco_from_predictions(pred.T, chrcols, 23)
    orc.write_loco(str(tmp_path / "ref.loco"), list(prep.ids), prep.ind_in_analysis, prep.mask[:, 0], loco)
    want = open(str(tmp_path / "ref.loco"), "rb").read()
    assert open(out + "_1.loco", "rb").read() == want and (b"NA" in want) == bt
    log = open(out + ".log").read()
    table = orc.cv_table(np.vstack([cs, np.zeros((6 - cs.shape[0], R1))]), prep.Neff[0], pl["L"], pl["tau"][0], bt, best)
    assert "phenotype 1 (Y1) : \n" + "\n".join(table) + "\n  * making predictions...writing LOCO predictions...done\n\n" in log
    assert table[best].endswith("<- min value") and sum(t.endswith("<- min value") for t in table) == 1
    # the .prs file: the header of the .loco file and one row `0 v1 v2 ... ` of the whole-genome predictions; the lists: `<trait> <full path>`
    order = [i for i in sorted(range(N), key=lambda i: prep.ids[i]) if prep.ind_in_analysis[i]]
    tot = np.zeros(N)
    for c in range(nchr):
        tot += pred[c]
    prs = open(out + "_1.prs").read().split("\n")
    assert prs[0] == want.decode().split("\n")[0] and prs[2] == "" and len(prs) == 3
    assert prs[1] == "0 " + "".join((orc.cpp_double(tot[i]) if prep.mask[i, 0] else "NA") + " " for i in order)
    assert open(out + "_pred.list").read() == "Y1 %s_1.loco\n" % out and open(out + "_prs.list").read() == "Y1 %s_1.prs\n" % out
    assert "List of blup files written to: [%s_pred.list]\n" % out in log


def test_split_l0_without_a_device(lib, tmp_path):
    """The command of tests/test_cli_gpu.py::test_cli_split_l0_equals_single_run: the same master file and variant lists, no device."""
    base = ["--step", "1", "--bed", os.path.join(E, "example"), "--exclude", os.path.join(E, "snplist_rm.txt"), "--covarFile", os.path.join(E, "covariates.txt"),
            "--phenoFile", os.path.join(E, "phenotype_bin.txt"), "--remove", os.path.join(E, "fid_iid_to_remove.txt"), "--bsize", "100", "--bt", "--lowmem", "--lowmem-prefix", "tmp_rg"]
    pre = str(tmp_path / "fit_bin_parallel")
    h, err = _open(lib, base + ["--split-l0", pre + ",4", "--out", str(tmp_path / "l0")])
    assert h is not None, err
    lib.s1_close(h)
    master = open(pre + ".master").read().split("\n")
    assert master[0] == "994 100" and master[5] == ""
    assert [ln.split(" ") for ln in master[1:5]] == [[pre + "_job%d" % (j + 1), nb, ns] for j, (nb, ns) in enumerate((("3", "300"), ("3", "300"), ("2", "200"), ("2", "194")))]
    rmv = set(open(os.path.join(E, "snplist_rm.txt")).read().split())
    kept = [ln.split()[1] for ln in open(os.path.join(E, "example.bim")) if ln.split()[1] not in rmv]
    got = [open("%s_job%d.snplist" % (pre, j)).read().split("\n") for j in range(1, 5)]
    assert all(g[-1] == "" for g in got) and [len(g) - 1 for g in got] == [300, 300, 200, 194]
    assert sum((g[:-1] for g in got), []) == kept
    log = open(str(tmp_path / "l0.log")).read()
    assert " * running level 0 in parallel across 10 genotype blocks\n   -using 4 jobs\n" in log and log.endswith("\nEnd of run\n")
    h, err = _open(lib, base + ["--split-l0", pre + "x,1", "--out", str(tmp_path / "l1")])
    assert h is None and err == "number of jobs must be >1."
    h, err = _open(lib, base + ["--split-l0", pre + "y,25", "--out", str(tmp_path / "l2")])
    assert h is not None, err
    lib.s1_close(h)
    assert "   -WARNING: Number of jobs cannot be greater than number of blocks.\n   -using 10 jobs\n" in open(str(tmp_path / "l2.log")).read()
    assert len(open(pre + "y.master").read().split("\n")) == 12 and os.path.exists(pre + "y_job10.snplist") and not os.path.exists(pre + "y_job11.snplist")
