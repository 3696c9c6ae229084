"""`regenie-amd --step 2 --compute-corr`: what the host driver decides before any device is touched (checkable without a GPU)."""
import os
import subprocess

import pytest

from tests import ld_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "regenie_amd", "bin", "regenie-amd")
E = lc.EX


@pytest.fixture(scope="module", autouse=True)
def _built():
    from regenie_amd import build
    build.build()


def _run(args, cwd):
    return subprocess.run([BIN, "--step", "2", "--bsize", "100", "--out", "o"] + args, cwd=str(cwd), capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args, message", [
    (["--bed", E + "/example", "--compute-corr", "--exclude", E + "/snplist_rm.txt"], "cannot use --exclude with --compute-corr (use --extract instead)"),
    (["--bed", E + "/example_3chr", "--compute-corr"], "can only compute LD matrix for a single chromosome (use --chr/--chrList/--range)."),
    (["--bed", E + "/example_3chr", "--compute-corr", "--chrList", "1,3"], "can only compute LD matrix for a single chromosome (use --chr/--chrList/--range)."),
    (["--bed", E + "/example", "--compute-corr", "--ld-extract", E + "/snplist_rm.txt"], "--ld-extract (burden masks in the LD matrix) is not built"),
    (["--bed", E + "/example", "--compute-corr", "--skip-scaleG"], "--skip-scaleG (the LD matrix of unscaled genotypes) is not built"),
    (["--bed", E + "/example", "--compute-corr", "--sparse-thr", "0.1"], "--sparse-thr (the sparsified LD matrix, which needs --skip-scaleG) is not built"),
    (["--bgen", E + "/example.bgen", "--compute-corr"], "--compute-corr with dosage input (--bgen) is not built"),
    (["--bed", E + "/example", "--compute-corr", "--gpus", "2"], "--compute-corr on more than one GPU (--gpus) is not built"),
    (["--bed", E + "/example", "--compute-corr", "--range", "1-100"], "wrong format for --range (must be CHR:MINPOS-MAXPOS)."),
    (["--bed", E + "/example", "--compute-corr", "--range", "1:-5-100"], "wrong format for --range (must be CHR:MINPOS-MAXPOS)."),
    (["--bed", E + "/example", "--compute-corr", "--chr", "77"], "invalid chromosome specified by --chr/--chrList."),
    (["--bed", E + "/example_3chr", "--compute-corr", "--range", "2:900000-900001"], "no variant left to include in analysis."),
])
def test_ld_mode_refusals(tmp_path, args, message):
    r = _run(args, tmp_path)
    assert r.returncode != 0
    assert "ERROR: " + message in r.stdout + r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    assert not os.path.exists(str(tmp_path / "o.corr"))


def test_ld_mode_needs_no_phenotype_and_filters_log(tmp_path):
    """No --phenoFile / --pred; the range filter's log line and the column count are the reference's (250 variants in 2:1-300)."""
    r = _run(["--bed", E + "/example_3chr", "--covarFile", E + "/covariates.txt", "--compute-corr", "--range", "2:1-300"], tmp_path)
    out = r.stdout
    # the run ends at the device (without one: the driver's "no MI355X" error), after everything asserted here has been logged
    assert r.returncode == 0 or "ERROR: no MI355X" in out, out[-2000:] + r.stderr[-2000:]
    assert "   -number of variants after filtering on range = 250\n" in out
    assert " * number of individuals used in analysis = 500\n" in out
    assert "  + n_snps = 250\n" in out and "(storing R^2 values)" in out
    assert "phenotypes" not in out.split("Fitting null model")[-1].split(" * covariates")[0]      # no phenotype file is asked for or read


def test_ld_mode_refuses_a_pgen_with_a_dosage_track(tmp_path):
    """The other form of dosage input: a .pgen one variant of which carries a dosage track (params.dosage_mode, Geno.cpp:1124) -- refused by
    the LD unit before any device call."""
    import numpy as np
    from oracle import pgen as opg
    rng = np.random.default_rng(2)
    m, n = 30, 50
    g = rng.integers(0, 3, size=(m, n)).astype(np.uint8)
    pre = str(tmp_path / "d")
    opg.write_pgen(pre + ".pgen", g, [0] * m, wide_vrtypes=True, dosage_variant=4)
    opg.write_pvar_psam(pre, [1] * m, n)
    assert opg.PgenOracle(pre + ".pgen").dosage_present
    r = _run(["--pgen", pre, "--compute-corr"], tmp_path)
    assert r.returncode != 0
    assert "ERROR: --compute-corr with dosage input (a .pgen with a dosage track) is not built" in r.stdout + r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    assert not os.path.exists(str(tmp_path / "o.corr"))
