"""`regenie-amd --step 2 --compute-corr` with --skip-scaleG / --sparse-thr: what the host driver decides before any device is touched
(checkable without a GPU).  tests/test_ld_cli_cpu.py pins the start of the two refusals that stay; here their full text, the range
check of the reference (Regenie.cpp:919-924), and that the text form of the unscaled matrix gets past option parsing."""
import os
import subprocess

import pytest

from tests import ld_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "regenie_amd", "bin", "regenie-amd")
E = lc.EX

SKIP = ("--skip-scaleG (the LD matrix of unscaled genotypes) is not built for the binary .corr file, whose 16-bit R^2 body has no meaning for "
        "unscaled values: add --output-corr-text.")
SPARSE = ("--sparse-thr (the sparsified LD matrix, which needs --skip-scaleG) is not built without --skip-scaleG "
          "(regenie: \"cannot use --sparse-thr without --skip-scaleG\").")


@pytest.fixture(scope="module", autouse=True)
def _built():
    from regenie_amd import build
    build.build()


def _run(args, cwd):
    return subprocess.run([BIN, "--step", "2", "--bsize", "100", "--out", "o"] + args, cwd=str(cwd), capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args, message", [
    (["--output-corr-text", "--skip-scaleG", "--sparse-thr", "1.5"], "invalid value passed in --sparse-thr (must be in [0,1)"),
    (["--output-corr-text", "--skip-scaleG", "--sparse-thr", "1"], "invalid value passed in --sparse-thr (must be in [0,1)"),
    (["--output-corr-text", "--skip-scaleG", "--sparse-thr", "-0.1"], "invalid value passed in --sparse-thr (must be in [0,1)"),
    (["--compute-corr", "--skip-scaleG"], SKIP),
    (["--compute-corr", "--skip-scaleG", "--sparse-thr", "0.1"], SKIP),      # (the reference writes text lines into a binary-mode file here)
    (["--compute-corr", "--sparse-thr", "0.1"], SPARSE),
    (["--output-corr-text", "--sparse-thr", "0.1"], SPARSE),
    (["--output-corr-text", "--skip-scaleG", "--ld-extract", E + "/snplist_rm.txt"], "--ld-extract (burden masks in the LD matrix) is not built"),
    (["--output-corr-text", "--skip-scaleG", "--test", "dominant"], "--test dominant / recessive with --compute-corr (the LD matrix of recoded genotypes) is not built."),
    (["--output-corr-text", "--skip-scaleG", "--gpus", "2"], "--compute-corr on more than one GPU (--gpus) is not built"),
])
def test_gtg_usage_errors(tmp_path, args, message):
    r = _run(["--bed", E + "/example"] + args, tmp_path)
    assert r.returncode != 0
    assert "ERROR: " + message in r.stdout + r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    assert not os.path.exists(str(tmp_path / "o.corr"))


@pytest.mark.parametrize("extra", [[], ["--sparse-thr", "0"], ["--sparse-thr", "0.2"]])
def test_gtg_text_mode_gets_past_option_parsing(tmp_path, extra):
    """The run ends at the device (without one: the driver's "no MI355X" error), after the mode has been announced."""
    r = _run(["--bed", E + "/example_3chr", "--covarFile", E + "/covariates.txt", "--output-corr-text", "--skip-scaleG", "--range", "2:1-300"] + extra, tmp_path)
    out = r.stdout
    assert r.returncode == 0 or "ERROR: no MI355X" in out, out[-2000:] + r.stderr[-2000:]
    assert "is not built" not in out and "invalid value" not in out
    assert " * computing correlation matrix in hard-call mode\n  + output to text file [" in out
    assert "  + n_snps = 250\n" in out
