"""`regenie-amd --step 2 --test dominant|recessive [--minHOMs N]` on the GPU against the files regenie itself wrote for the same command lines
(tests/golden/ref_outputs/dom_rec, tests/golden/make_dom_rec_ref_outputs.py; the cases: tests/dom_rec_cases.py).

Comparison: the lines of the uncorrected tests must be byte-identical to regenie's, as every additive route's are (profiles/condtl.md, profiles/mcc.md).
Only a row a correction re-tested (`--firth --approx`, `--spa`: the score test's p-value below --pThresh = 0.05, so its printed CHISQ is above the
chi-square(1) 0.95 quantile or the test failed) may differ, and then within tests/condtl_cases.py compare_regenie_files -- the rule the condtl / mcc
CLI tests apply (text columns as text; `--spa` 3e-5, approximate Firth 2e-4: regenie's own stopping tolerance).  The count is printed per case."""
import json
import os
import subprocess

import pytest

from tests import condtl_cases as cc
from tests import dom_rec_cases as dc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "regenie_amd", "bin", "regenie-amd")
CHI2_95 = 3.8414588


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dom_rec"))
    dc.write_inputs(d)
    return d


def _drive(args, cwd, out="o"):
    return subprocess.run([BIN] + args + ["--out", out], cwd=str(cwd), capture_output=True, text=True, timeout=300)


def _meta(name):
    return json.load(open(os.path.join(dc.REF, name, "meta.json")))


def _retested(name, k):
    """Ids of the rows a correction re-tests in trait k: the score test's p-value below --pThresh = 0.05, read off regenie's file for the same command
    without the correction (the corrected CHISQ itself can land on either side of the quantile).  `--spa` has no such twin here: its rule is the
    printed CHISQ, as in compare_regenie_files."""
    if name in dc.SCORE_OF:
        rows = [ln.split(" ") for ln in dc.golden(dc.SCORE_OF[name], k)[1:]]
        return {t[2] for t in rows if t[-3] != "NA" and float(t[-3]) > CHI2_95}
    if "spa" in name:
        return {t[2] for t in (ln.split(" ") for ln in dc.golden(name, k)[1:]) if t[-1] == "TEST_FAIL" or t[-3] == "NA" or float(t[-3]) > CHI2_95}
    return set()


def _compare(tmp_path, name, prefix="o"):
    total = lines = 0
    for k in (1, 2):
        got = open(str(tmp_path / ("%s_Y%d.regenie" % (prefix, k)))).read().splitlines()
        ref = dc.golden(name, k)
        total += cc.compare_regenie_files(got, ref, "%s Y%d" % (name, k))
        lines += len(ref) - 1
        retested = _retested(name, k)
        for a, b in zip(got[1:], ref[1:]):
            assert a == b or b.split(" ")[2] in retested, (name, a, b)
    print("dom_rec %s: %d of %d result lines not byte-identical to regenie's" % (name, total, lines))


@pytest.mark.parametrize("name", dc.FILE_CASES)
def test_cli_dom_rec_against_reference_files(inputs, tmp_path, name):
    r = _drive(dc.args_of(name, inputs), tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for ln in _meta(name)["log"]:
        assert ln in r.stdout.splitlines(), (ln, r.stdout[-3000:])
    _compare(tmp_path, name)


def test_cli_dom_rec_two_parts_write_the_one_gpu_bytes(inputs, tmp_path):
    a = dc.args_of("b_qt_rec_minhoms", inputs)
    r1, r2 = _drive(a, tmp_path, out="one"), _drive(a + ["--gpus", "2", "--single-device"], tmp_path, out="two")
    assert r1.returncode == 0 and r2.returncode == 0, r1.stdout[-2000:] + r2.stdout[-2000:] + r2.stderr[-1000:]
    assert "GPU 1 : blocks" in r2.stdout
    for k in (1, 2):
        assert open(str(tmp_path / ("one_Y%d.regenie" % k)), "rb").read() == open(str(tmp_path / ("two_Y%d.regenie" % k)), "rb").read()
