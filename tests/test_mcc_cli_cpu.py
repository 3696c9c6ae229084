"""`regenie-amd --step 2 --qt --mcc [--mcc-thr p] [--mcc-skew s]`: what the host driver decides before any device is touched (checkable without a
GPU) -- the options, the reference's two error texts (tests/golden/ref_outputs/mcc/*/meta.json) and the skewness line of the log."""
import json
import os
import subprocess

import pytest

from tests import mcc_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "regenie_amd", "bin", "regenie-amd")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from regenie_amd import build
    build.build()
    d = str(tmp_path_factory.mktemp("mcc"))
    mc.write_inputs(d)
    return d


def _drive(args, cwd):
    return subprocess.run([BIN] + args + ["--out", "o"], cwd=str(cwd), capture_output=True, text=True, timeout=120)


def _meta(name):
    return json.load(open(os.path.join(mc.REF, name, "meta.json")))


@pytest.mark.parametrize("name", mc.ERROR_CASES)
def test_mcc_errors_of_the_reference(inputs, tmp_path, name):
    meta = _meta(name)
    assert meta["returncode"] == 1 and len(meta["error"]) == 1
    r = _drive(mc.args_of(name, inputs), tmp_path)
    assert r.returncode == 1, r.stdout[-2000:]
    assert meta["error"][0] in (r.stdout + r.stderr).splitlines(), r.stdout[-2000:]
    assert not [fn for fn in os.listdir(str(tmp_path)) if fn.endswith(".regenie")]


def test_mcc_thr_outside_the_unit_interval_is_taken_as_the_reference_takes_it(inputs, tmp_path):
    """regenie's range check of --mcc-thr (`thr > 1 && thr <= 0`) never fires: it runs `--mcc-thr 1.5` to the end (checked with its binary).  No
    option error here either; the run ends at the device or completes."""
    a = mc.args_of("b_bed_thr", inputs)
    for val in ("0", "1.5"):
        r = _drive(a + ["--mcc-thr", val], tmp_path)
        out = r.stdout + r.stderr
        assert r.returncode == 0 or "ERROR: no MI355X" in out, out[-2000:]
        assert "--mcc-thr" not in "".join(ln for ln in out.splitlines() if ln.startswith("ERROR"))


@pytest.mark.parametrize("name", ["a_bed_all", "b_bed_thr", "c_bed_skew", "d_bgen_all"])
def test_mcc_options_are_known_and_the_skewness_line_is_the_reference_s(inputs, tmp_path, name):
    """The run ends at the device (without one: the driver's "no MI355X" error), after the phenotypes are read and the line is logged."""
    r = _drive(mc.args_of(name, inputs), tmp_path)
    out = r.stdout + r.stderr
    assert "unrecognised option" not in out, out[-2000:]
    assert r.returncode == 0 or "ERROR: no MI355X" in out, out[-2000:]
    meta = _meta(name)
    assert len(meta["log"]) == 1 and meta["log"][0] in out.splitlines(), out[-3000:]


def test_mcc_skew_above_every_trait_switches_the_test_off(inputs, tmp_path):
    a = mc.args_of("c_bed_skew", inputs)
    a[a.index("--mcc-skew") + 1] = "1000"
    r = _drive(a, tmp_path)
    assert "   -computing phenotypic skewness: 0 phenotypes will use the MCC test" in (r.stdout + r.stderr).splitlines(), r.stdout[-2000:]


def test_mcc_is_ignored_for_binary_traits_apart_from_the_log_line(inputs, tmp_path):
    a = mc.args_of("a_bed_all", inputs)
    a[a.index("--qt")] = "--bt"
    a[a.index("--phenoFile") + 1] = os.path.join(mc.EX, "phenotype_bin.txt")
    r = _drive(a, tmp_path)
    out = r.stdout + r.stderr
    assert r.returncode == 0 or "ERROR: no MI355X" in out, out[-2000:]
    assert "   -computing phenotypic skewness: 2 phenotypes will use the MCC test" in out.splitlines(), out[-3000:]


def test_mcc_with_count_traits_logs_the_line_and_nothing_else(inputs, tmp_path):
    """regenie --ct --mcc prints the skewness line and runs the count-trait test (checked with its binary)."""
    a = mc.args_of("a_bed_all", inputs)
    a[a.index("--qt")] = "--ct"
    r = _drive(a, tmp_path)
    out = r.stdout + r.stderr
    assert r.returncode == 0 or "ERROR: no MI355X" in out, out[-2000:]
    assert "   -computing phenotypic skewness: 2 phenotypes will use the MCC test" in out.splitlines(), out[-3000:]


def test_mcc_with_compute_corr_is_silent(inputs, tmp_path):
    """Under --compute-corr regenie reads no phenotype and skips the skewness step with it (Pheno.cpp:109: the block sits inside
    `if(!params->getCorMat)`; its binary prints no skewness line for this command): no line here either."""
    r = _drive(["--step", "2", "--bed", os.path.join(mc.EX, "example_3chr"), "--covarFile", os.path.join(mc.EX, "covariates.txt"), "--bsize", "100",
                "--chr", "2", "--compute-corr", "--mcc"], tmp_path)
    out = r.stdout + r.stderr
    assert r.returncode == 0 or "ERROR: no MI355X" in out, out[-2000:]
    assert "phenotypic skewness" not in out


def test_mcc_all_missing_trait_stops_the_run_at_any_skew(inputs, tmp_path):
    """compute_skew runs for every trait whatever --mcc-skew is: a trait without a value is skew_pheno's error."""
    lines = open(os.path.join(inputs, "pheno_skew.txt")).read().splitlines()
    with open(str(tmp_path / "p.txt"), "w") as f:
        f.write(lines[0] + "\n")
        for ln in lines[1:]:
            t = ln.split()
            f.write("%s %s %s NA\n" % (t[0], t[1], t[2]))
    a = mc.args_of("a_bed_all", inputs)
    a[a.index("--phenoFile") + 1] = str(tmp_path / "p.txt")
    r = _drive(a, tmp_path)
    out = r.stdout + r.stderr
    assert r.returncode != 0
    assert "ERROR" in out and "no MI355X" not in out, out[-2000:]
