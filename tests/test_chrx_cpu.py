"""Step 2 on chromosome X with males, without a device: `--par-region` as the driver parses it (the driver's own host sources, compiled with g++ as
tests/test_host_prep_cpu.py does), the sex codes its readers keep, the NumPy restatement of the reference's minor-allele-count rule
(tests/chrx_cases.py) against the kept / dropped sets of regenie's own files, and the conditions the fixtures are built to meet."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import chrx_cases as xc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HARNESS = r'''
#include "driver.h"
extern "C" const char* rg_last_error(const rg_ctx*) { return "no device library in this harness"; }
using namespace rgdrv;
static std::string g_err;
extern "C" const char* cx_error() { return g_err.c_str(); }
// parse_args alone: out = {par_set, par1_max, par2_min}; 0 on success
extern "C" int cx_parse(int argc, char** argv, int64_t* out) {
  try { Params p = parse_args(argc, argv); out[0] = p.par_set; out[1] = p.par1_max; out[2] = p.par2_min; return 0; }
  catch (const std::exception& e) { g_err = e.what(); return 1; }
}
// parse_args + read_bim_fam: the sex code of every sample of the file into sex[cap]; returns their number, -1 on error
extern "C" int64_t cx_sex(int argc, char** argv, uint8_t* sex, int64_t cap, int* has_male) {
  std::cout.flush(); fflush(stdout);
  const int saved = dup(1), nul = open("/dev/null", O_WRONLY);
  dup2(nul, 1); close(nul);
  int64_t n = -1;
  try {
    Run r;
    r.p = parse_args(argc, argv);
    read_bim_fam(r);
    n = (int64_t)r.sex.size();
    for (int64_t i = 0; i < n && i < cap; ++i) sex[i] = r.sex[i];
    *has_male = r.has_male;
  } catch (const std::exception& e) { g_err = e.what(); }
  std::cout.flush(); fflush(stdout); dup2(saved, 1); close(saved);
  return n;
}
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("chrx_host")
    (d / "h.cpp").write_text(HARNESS)
    host, csrc = os.path.join(ROOT, "regenie_amd", "host"), os.path.join(ROOT, "regenie_amd", "csrc")
    r = subprocess.run(["g++", "-O0", "-std=c++17", "-shared", "-fPIC", "-w", "-I" + host] + [os.path.join(host, f) for f in ("driver_common.cpp", "driver_inputs.cpp", "driver_models.cpp")]
                       + [os.path.join(csrc, f) for f in ("pgen_api.cpp", "bgen_api.cpp")] + [str(d / "h.cpp"), "-o", str(d / "libcx.so"), "-lz", "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(str(d / "libcx.so"))
    L.cx_error.restype = C.c_char_p
    L.cx_sex.restype = C.c_int64
    return L


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("chrx_in"))
    g, gh = xc.write_inputs(d)
    return d, g, gh


def _argv(args):
    return C.c_int(len(args) + 1), (C.c_char_p * (len(args) + 1))(b"regenie-amd", *[a.encode() for a in args])


BASE = ["--step", "2", "--bed", "x", "--phenoFile", "p", "--pred", "l", "--bsize", "10"]


def _parse(L, extra, base=BASE):
    out = (C.c_int64 * 3)()
    rc = L.cx_parse(*_argv(base + extra), out)
    return (None, L.cx_error().decode()) if rc else (tuple(int(v) for v in out), None)


@pytest.mark.parametrize("code,bounds", [("b36", (2709520, 154584238)), ("hg18", (2709520, 154584238)), ("b37", (2699520, 154931044)), ("hg19", (2699520, 154931044)),
                                         ("hg38", (2781479, 155701383)), ("b38", (2781479, 155701383)), ("5000000,100000000", (4999999, 100000001)),
                                         ("7,7", (6, 8)), ("1,2", (0, 3))])
def test_par_region_build_codes(lib, code, bounds):
    got, err = _parse(lib, ["--par-region", code])
    assert err is None and got == (1,) + bounds
    assert xc.par_bounds(code) == bounds


@pytest.mark.parametrize("code", ["hg17", "", "100", "100,", ",100", "0,100", "100,0", "200,100", "-5,100", "a,b", "hg19,hg38"])
def test_par_region_bad_forms_are_the_reference_s_error(lib, code):
    got, err = _parse(lib, ["--par-region", code])
    assert got is None and "invalid build code given" in err and "b36|b37|b38|hg18|hg19|hg38" in err
    with pytest.raises(ValueError):
        xc.par_bounds(code)


def test_par_region_other_rules(lib):
    assert _parse(lib, [])[0] == (0, 0, 0)                                                   # not given: nothing is assumed
    got, err = _parse(lib, ["--par-region"])
    assert got is None and "needs a value" in err
    got, err = _parse(lib, ["--par-region", "hg19"], base=["--step", "1", "--bed", "x", "--phenoFile", "p", "--bsize", "10"])
    assert got is None and "step 2" in err
    for opt in (["--skip-dosage-comp"], ["--sex-specific", "male"]):
        got, err = _parse(lib, ["--par-region", "hg19"] + opt)
        assert got is None and opt[0] in err and "not built" in err


def test_readers_keep_the_sex_codes(lib, inputs):
    d = inputs[0]
    want = xc.sexes()
    tail = ["--phenoFile", "p", "--pred", "l", "--bsize", "10", "--step", "2"]
    for src, exp in ((["--bed", d + "/xq"], want), (["--pgen", d + "/xp"], want), (["--bgen", d + "/x.bgen", "--sample", d + "/x.sample"], want),
                     (["--bed", d + "/xq0"], 0 * want), (["--pgen", d + "/xp0"], 0 * want), (["--bgen", d + "/x.bgen", "--sample", d + "/x0.sample"], 0 * want)):
        sex = np.zeros(xc.N, np.uint8)
        hm = C.c_int(-1)
        n = lib.cx_sex(*_argv(src + tail), sex.ctypes.data_as(C.c_void_p), C.c_int64(xc.N), C.byref(hm))
        assert n == xc.N, (src, lib.cx_error())
        assert np.array_equal(sex, exp) and hm.value == int((exp == 1).any()), src


def test_rule_restated(inputs):
    """The rule on a case small enough to do by hand: 3 females (0, 1, 2), 3 males (0, 2, 2), one male call missing."""
    G = np.array([[0, 1, 2, 0, 2, 2, np.nan]])
    sex = np.array([2, 2, 0, 1, 1, 1, 1])
    masks = np.array([[1, 1], [1, 1], [1, 0], [1, 1], [1, 1], [1, 0], [1, 1]], bool)
    r = xc.mac_rule(G, sex, masks, np.array([True]))
    assert r["auto_all"][0, 0] == min(7, 12 - 7) and r["sex_all"][0, 0] == min(5.0, 12 - 3 - 5.0)        # mac = 3 + 0.5 * 4, nmales = 3 observed
    assert list(r["auto_trait"][0]) == [5.0, min(3, 8 - 3)] and list(r["sex_trait"][0]) == [4.0, min(2.0, 8 - 2 - 2.0)]
    r = xc.mac_rule(G, sex, masks, np.array([False]))
    assert r["sex_all"][0, 0] == r["auto_all"][0, 0] and list(r["sex_trait"][0]) == list(r["auto_trait"][0])


@pytest.mark.parametrize("name", list(xc.CASES))
def test_fixtures_kept_and_dropped_sets_follow_the_rule(inputs, name):
    d, g, gh = inputs
    r = xc.expected_sets(name, d, g, gh)
    m = xc.meta(name)
    assert m["returncode"] == 0 and tuple(m["bounds"]) == xc.par_bounds(m["par_region"]) and "--par-region" in m["cmd"]
    ids = [[ln.split(" ")[2] for ln in xc.golden(name, k + 1)[1:]] for k in range(xc.P)]
    for k in range(xc.P):
        assert len(ids[k]) > 150 and ids[k] == sorted(ids[k], key=lambda v: int(v[1:]))
        if name == "g_qt_rec":
            assert set(ids[k]) <= r["keep"][k] and len(ids[k]) >= len(r["keep"][k]) - 5      # the recessive test's own filters drop a few more
        else:
            assert set(ids[k]) == r["keep"][k], sorted(set(ids[k]) ^ r["keep"][k])


@pytest.mark.parametrize("name", xc.SEX_CASES)
def test_fixture_conditions(inputs, name):
    """What makes the fixtures tell the sex-aware rule from a lifted refusal: recomputed from the inputs, compared with regenie's files and meta.json."""
    d, g, gh = inputs
    r = xc.expected_sets(name, d, g, gh)
    c = xc.meta(name)["conditions"]
    npar = xc.non_par(xc.build_of(name))
    ids = [{ln.split(" ")[2] for ln in xc.golden(name, k + 1)[1:]} for k in range(xc.P)]
    dropped = ["s%d" % j for j in range(xc.M) if npar[j] and r["auto_all"][j, 0] >= xc.MIN_MAC and r["sex_all"][j, 0] < xc.MIN_MAC]
    assert len(dropped) >= 10 and dropped == c["dropped_variants"] and not (set(dropped) & (ids[0] | ids[1]))
    male = xc.sexes() == 1
    gg = gh if name == "i_qt_het_male" else g
    alt_m = sum(int((gg[int(v[1:])][male] > 0).sum()) for v in dropped)
    alt_f = sum(int((gg[int(v[1:])][~male] > 0).sum()) for v in dropped)
    assert alt_m > 3 * alt_f                                                                 # their alternate alleles lie mostly in males
    flipped = [["s%d" % j, k + 1] for j in range(xc.M) for k in range(xc.P)
               if r["sex_all"][j, 0] >= xc.MIN_MAC and r["auto_trait"][j, k] >= xc.MIN_MAC and r["sex_trait"][j, k] < xc.MIN_MAC]
    assert flipped == c["flipped_tests"]
    if "{D}/xq.pheno" in xc.CASES[name]:
        assert len(flipped) >= 5 and all(v not in ids[k - 1] and v in ids[2 - k] for v, k in flipped)
    if name == "d_bt_firth":
        pairs = c["firth_pairs_autosomal_ge_50_sex_aware_lt_50"]
        assert pairs and all(a >= 50 > s and int(v[1:]) in xc.F50 and (g[int(v[1:])] > 0).sum() <= xc.N // 2 for v, k, a, s in pairs)
        for v, k, a, s in pairs:
            assert r["auto_trait"][int(v[1:]), k - 1] == a and r["sex_trait"][int(v[1:]), k - 1] == s
    if name in xc.NOSEX_OF:
        assert c["par_variants_tested"] >= 10 and c["chr22_variants_tested"] == 100
        same = 0
        for k in range(xc.P):
            other = {ln.split(" ")[2]: ln for ln in xc.golden(xc.NOSEX_OF[name], k + 1)[1:]}
            for ln in xc.golden(name, k + 1)[1:]:
                v = ln.split(" ")[2]
                if not npar[int(v[1:])]:
                    assert other[v] == ln
                    same += 1
        assert same == c["lines_identical_to_nosex_run"] and same >= 2 * 100 + 10
    if name == "i_qt_het_male":
        assert xc.meta(name)["het_male_variants"] == ["s%d" % j for j in xc.HET_MALE]
