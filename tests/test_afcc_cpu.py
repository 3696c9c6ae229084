"""`--af-cc` without a GPU: the NumPy restatement of update_af_cc / compute_aaf_info (tests/afcc_cases.py) against regenie's own files
(tests/golden/ref_outputs/af_cc/, written by tests/golden/make_afcc_ref_outputs.py), the fixtures of the modes in which the reference switches the
option off, and the driver's option parser through the host-only build tests/test_host_prep_cpu.py uses."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import afcc_cases as ac

ROOT = ac.ROOT


@pytest.fixture(scope="module")
def inputs():
    g = ac.calls()
    ac.check_inputs(g)
    y, miss = ac.phenotypes()
    return g, y, ~miss


@pytest.mark.parametrize("name", ac.ACTIVE)
def test_restatement_reproduces_the_four_columns_of_every_line(inputs, name):
    g, y, mask = inputs
    q, scale = ac.genotypes_of(name, g)
    f_case, f_ctrl, n_case, n_ctrl = ac.afcc_columns(q, scale, y, mask)
    checked = 0
    for k in range(ac.P):
        lines = ac.golden(name, k + 1)
        h = lines[0].split(" ")
        ia, inn, iid = h.index("A1FREQ"), h.index("N"), h.index("ID")
        assert h[ia + 1:ia + 3] == list(ac.AFCC_COLS[:2]) and h[inn + 1:inn + 3] == list(ac.AFCC_COLS[2:])
        for ln in lines[1:]:
            t = ln.split(" ")
            j = int(t[iid][1:])
            assert (t[ia + 1], t[ia + 2], t[inn + 1], t[inn + 2]) == (f_case[j, k], f_ctrl[j, k], n_case[j, k], n_ctrl[j, k]), (name, k, ln)
            assert int(t[inn]) == int(t[inn + 1]) + int(t[inn + 2])
            checked += 1
    assert checked == sum(ac.meta(name)["lines"]) and checked > 800


def test_every_line_of_a_corrected_file_has_the_columns():
    """Firth / SPA-corrected lines carry the columns like any other (print_sum_stats_single is the one writer)."""
    for name in ("b_bed_firth", "c_bed_spa", "g_bgen_firth"):
        for k in range(1, ac.P + 1):
            lines, plain = ac.golden(name, k), ac.golden("a_bed" if "bed" in name else "f_bgen", k)
            assert len(lines) == len(plain)
            h = lines[0].split(" ")
            ia, inn = h.index("A1FREQ"), h.index("N")
            changed = 0
            for a, b in zip(lines[1:], plain[1:]):
                ta, tb = a.split(" "), b.split(" ")
                assert ta[:inn + 4] == tb[:inn + 4]                      # up to TEST: identical to the uncorrected run
                changed += ta != tb
            assert changed > 0, name


@pytest.mark.parametrize("name", ac.DISABLED)
def test_disabled_modes_equal_the_run_without_the_option(name):
    assert ac.meta(name)["warning"] and not ac.meta(name + "_plain")["warning"]
    for k in range(1, ac.P + 1):
        lines = ac.golden(name, k)
        assert lines == ac.golden(name + "_plain", k)
        assert not set(ac.AFCC_COLS) & set(lines[0].split(" "))


@pytest.mark.parametrize("name", ["a_bed", "f_bgen"])
def test_the_option_changes_nothing_but_its_columns(name):
    for k in range(1, ac.P + 1):
        assert ac.strip_afcc(ac.golden(name, k)) == ac.golden(name + "_plain", k)


# ---- the driver's parser (host-only build: parse_args needs no device) ---------------------------------------------------------------------------
HARNESS = r'''
#include "driver.h"
extern "C" const char* rg_last_error(const rg_ctx*) { return "no device library in this harness"; }
using namespace rgdrv;
static std::string g_err;
extern "C" const char* pa_error() { return g_err.c_str(); }
// -> -1: parse_args threw (pa_error), else bit 0 = af_cc, bit 1 = bt
extern "C" int pa_flags(int argc, char** argv) {
  try { const Params p = parse_args(argc, argv); std::cout.flush(); return (p.af_cc ? 1 : 0) | (p.bt ? 2 : 0); }
  catch (const std::exception& e) { g_err = e.what(); std::cout.flush(); return -1; }
}
'''


@pytest.fixture(scope="module")
def parser(tmp_path_factory):
    d = tmp_path_factory.mktemp("afcc_parse")
    src = d / "h.cpp"
    src.write_text(HARNESS)
    so = d / "libpa.so"
    host, csrc = os.path.join(ROOT, "regenie_amd", "host"), os.path.join(ROOT, "regenie_amd", "csrc")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-w", "-I" + host] + [os.path.join(host, f) for f in ("driver_common.cpp", "driver_inputs.cpp", "driver_models.cpp")]
                       + [os.path.join(csrc, f) for f in ("pgen_api.cpp", "bgen_api.cpp")] + [str(src), "-o", str(so), "-lz", "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(str(so))
    L.pa_error.restype = C.c_char_p
    return L


def _parse(L, args, capfd):
    argv = (C.c_char_p * (len(args) + 1))(b"regenie-amd", *[a.encode() for a in args])
    capfd.readouterr()
    rc = L.pa_flags(C.c_int(len(args) + 1), argv)
    out = capfd.readouterr().out
    return rc, out, L.pa_error().decode()


_COMMON = ["--bed", "x", "--phenoFile", "x.pheno", "--bsize", "100"]


def test_parser_keeps_the_option_for_binary_traits_in_step_2(parser, capfd):
    rc, out, err = _parse(parser, ["--step", "2", "--bt", "--af-cc", "--pred", "p.list"] + _COMMON, capfd)
    assert rc == 3, err
    assert ac.WARNING not in out
    rc, out, err = _parse(parser, ["--step", "2", "--bt", "--af-cc", "--firth", "--approx", "--pred", "p.list"] + _COMMON, capfd)
    assert rc == 3 and ac.WARNING not in out, err
    rc, out, err = _parse(parser, ["--step", "2", "--bt", "--pred", "p.list"] + _COMMON, capfd)
    assert rc == 2, err


@pytest.mark.parametrize("mode", [["--step", "2", "--qt", "--pred", "p.list"], ["--step", "2", "--ct", "--pred", "p.list"], ["--step", "2", "--pred", "p.list"],
                                  ["--step", "1", "--bt"], ["--step", "1", "--qt"], ["--step", "2", "--compute-corr"]])
def test_parser_disables_the_option_elsewhere_with_the_reference_warning(parser, capfd, mode):
    rc, out, err = _parse(parser, mode + ["--af-cc"] + _COMMON, capfd)
    assert rc >= 0 and not (rc & 1), err
    assert out.count(ac.WARNING + "\n") == 1
    rc, out, err = _parse(parser, mode + _COMMON, capfd)
    assert rc >= 0 and ac.WARNING not in out, err


def test_parser_still_refuses_the_dosage_compensation_options(parser, capfd):
    for opt in (["--skip-dosage-comp"], ["--sex-specific", "male"]):
        rc, out, err = _parse(parser, ["--step", "2", "--bt", "--af-cc", "--pred", "p.list"] + opt + _COMMON, capfd)
        assert rc == -1 and "is not built" in err
