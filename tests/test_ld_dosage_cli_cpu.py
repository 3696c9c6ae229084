"""`regenie-amd --step 2 --compute-corr --ld-dosages` without a GPU: dosage input stays refused in LD mode unless --ld-dosages is given
(tests/test_ld_cli_cpu.py pins the refusals); with it the run announces the reference's dosage mode and ends at the device."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "regenie_amd", "bin", "regenie-amd")
E = os.path.join(ROOT, "tests", "golden", "example")


def _run(args, cwd):
    return subprocess.run([BIN, "--step", "2", "--bsize", "100", "--out", "o"] + args, cwd=str(cwd), capture_output=True, text=True, timeout=120)


def test_ld_dosages_goes_with_compute_corr_and_dosage_input(tmp_path):
    r = _run(["--bgen", E + "/example.bgen", "--ld-dosages"], tmp_path)
    assert r.returncode != 0 and "ERROR: --ld-dosages goes with --compute-corr / --output-corr-text." in r.stdout + r.stderr
    r = _run(["--bed", E + "/example", "--compute-corr", "--ld-dosages"], tmp_path)
    assert r.returncode != 0 and "ERROR: --ld-dosages needs dosage input" in r.stdout + r.stderr, r.stdout[-2000:]
    assert not os.path.exists(str(tmp_path / "o.corr"))


def test_bgen_runs_in_dosage_mode_up_to_the_device(tmp_path):
    r = _run(["--bgen", E + "/example.bgen", "--covarFile", E + "/covariates.txt", "--compute-corr", "--ld-dosages"], tmp_path)
    out = r.stdout + r.stderr
    assert "is not built" not in out, out[-2000:]
    assert " * computing correlation matrix in dosage mode (storing R^2 values)" in out, out[-2000:]
    assert r.returncode == 0 or "ERROR: no MI355X" in out, out[-2000:]


def test_pgen_dosage_track_runs_in_dosage_mode_up_to_the_device(tmp_path):
    from oracle import pgen as opg
    rng = np.random.default_rng(2)
    m, n = 30, 50
    g = rng.integers(0, 3, size=(m, n)).astype(np.uint8)
    pre = str(tmp_path / "d")
    opg.write_pgen(pre + ".pgen", g, [0] * m, wide_vrtypes=True, dosage_variant=4)
    opg.write_pvar_psam(pre, [1] * m, n)
    r = _run(["--pgen", pre, "--output-corr-text", "--ld-dosages"], tmp_path)
    out = r.stdout + r.stderr
    assert "is not built" not in out, out[-2000:]
    assert " * computing correlation matrix in dosage mode\n" in out, out[-2000:]
    assert r.returncode == 0 or "ERROR: no MI355X" in out, out[-2000:]
