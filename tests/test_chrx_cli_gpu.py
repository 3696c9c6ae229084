"""`regenie-amd --step 2 --par-region BUILD` on chromosome X with males, on the GPU, against the files regenie itself wrote for the same command
lines (tests/golden/ref_outputs/chrx, tests/golden/make_chrx_ref_outputs.py; the cases: tests/chrx_cases.py).

Comparison, as tests/test_dom_rec_cli_gpu.py: per trait file the same lines in the same order; the lines of the uncorrected tests byte-identical to
regenie's; only a row a correction re-tested (`--firth --approx`, `--spa`: the score test's p-value below --pThresh) may differ, and then within
tests/condtl_cases.py compare_regenie_files, unchanged.  Hard-call and count cases: every line byte-identical or within that helper's rule.
Every run here ends in the refusal of chromosome X at a driver without the feature."""
import os
import subprocess

import pytest

from tests import chrx_cases as xc
from tests import condtl_cases as cc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "regenie_amd", "bin", "regenie-amd")
CHI2 = {0.9: 0.0157908, 0.05: 3.8414588}


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("chrx"))
    xc.write_inputs(d)
    return d


def _drive(args, cwd, out="o"):
    return subprocess.run([BIN] + args + ["--out", out], cwd=str(cwd), capture_output=True, text=True, timeout=300)


def _retested(name, k):
    """Ids of the rows a correction re-tests in trait k (tests/test_dom_rec_cli_gpu.py's rule at this case's --pThresh)."""
    if name in xc.SCORE_OF:
        rows = [ln.split(" ") for ln in xc.golden(xc.SCORE_OF[name], k)[1:]]
        return {t[2] for t in rows if t[-3] != "NA" and float(t[-3]) > CHI2[xc.PTHRESH[name]]}
    if "spa" in name:
        return {t[2] for t in (ln.split(" ") for ln in xc.golden(name, k)[1:]) if t[-1] == "TEST_FAIL" or t[-3] == "NA" or float(t[-3]) > CHI2[xc.PTHRESH[name]]}
    return set()


def _compare(tmp_path, name, prefix="o"):
    total = lines = 0
    for k in range(1, xc.P + 1):
        got = open(str(tmp_path / ("%s_Y%d.regenie" % (prefix, k)))).read().splitlines()
        ref = xc.golden(name, k)
        assert [ln.split(" ")[:5] for ln in got] == [ln.split(" ")[:5] for ln in ref], (name, k)      # the set and the order of the lines
        total += cc.compare_regenie_files(got, ref, "%s Y%d" % (name, k))
        lines += len(ref) - 1
        retested = _retested(name, k)
        for a, b in zip(got[1:], ref[1:]):
            assert a == b or b.split(" ")[2] in retested, (name, a, b)
    print("chrx %s: %d of %d result lines not byte-identical to regenie's" % (name, total, lines))


def _het_male_ids(stderr):
    ids = []
    for ln in stderr.splitlines():
        if "genotype is 1 for a male on chrX" in ln:
            ids += ln[ln.index("[") + 1:ln.index("]")].split(";")
    return ids


@pytest.mark.parametrize("name", list(xc.CASES))
def test_cli_chrx_against_reference_files(inputs, tmp_path, name):
    r = _drive(xc.args_of(name, inputs), tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = xc.meta(name)
    if name[1] == "_":
        assert "non-PAR region is (%d, %d)" % tuple(m["bounds"]) in r.stdout
    assert _het_male_ids(r.stderr) == m["het_male_variants"]
    _compare(tmp_path, name)


@pytest.mark.parametrize("name", ["a_qt_bed_missing", "c_qt_bgen", "d_bt_firth"])
def test_cli_chrx_two_parts_on_one_device(inputs, tmp_path, name):
    r = _drive(xc.args_of(name, inputs) + ["--gpus", "2", "--single-device"], tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "GPU 1 : blocks" in r.stdout
    _compare(tmp_path, name)


def test_cli_chrx_refusals(inputs, tmp_path):
    a = xc.args_of("b_qt_pgen_ref_first", inputs)
    i = a.index("--par-region")
    r = _drive(a[:i] + a[i + 2:], tmp_path)                           # .pgen, males, no --par-region
    assert r.returncode != 0 and "non-PAR" in r.stdout and "--par-region hg38|hg19|hg18|b37|b36|<end_par1>,<start_par2>" in r.stdout, r.stdout[-2000:]
    r = _drive(xc.args_of("a_qt_bed_missing", inputs) + ["--skip-dosage-comp"], tmp_path)
    assert r.returncode != 0 and "--skip-dosage-comp" in r.stdout and "not built" in r.stdout, r.stdout[-2000:]
    r = _drive(a[:i] + ["--par-region", "hg17"] + a[i + 2:], tmp_path)
    assert r.returncode != 0 and "invalid build code given" in r.stdout
