"""`regenie-amd --step 2 --qt --mcc ...` on the GPU against the files regenie itself wrote for the same command lines
(tests/golden/ref_outputs/mcc, tests/golden/make_mcc_ref_outputs.py; the cases: tests/mcc_cases.py).

Comparison: tests/condtl_cases.py compare_regenie_files -- byte-identical lines expected, a line that is not must match to the printed digits at
2e-5 (the project's rule for uncorrected rows).  The count of lines that are not byte-identical is printed per case."""
import gzip
import json
import os
import subprocess

import pytest

from tests import mcc_cases as mc
from tests.condtl_cases import compare_regenie_files

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "regenie_amd", "bin", "regenie-amd")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("mcc"))
    mc.write_inputs(d)
    return d


def _drive(args, cwd, out="o"):
    return subprocess.run([BIN] + args + ["--out", out], cwd=str(cwd), capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("name", mc.FILE_CASES)
def test_cli_mcc_against_reference_files(inputs, tmp_path, name):
    r = _drive(mc.args_of(name, inputs), tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    meta = json.load(open(os.path.join(mc.REF, name, "meta.json")))
    assert meta["log"][0] in r.stdout.splitlines()
    total = 0
    for k in (1, 2):
        got = open(str(tmp_path / ("o_Y%d.regenie" % k))).read().splitlines()
        ref = gzip.open(os.path.join(mc.REF, name, "out_Y%d.regenie.gz" % k), "rt").read().splitlines()
        total += compare_regenie_files(got, ref, "%s Y%d" % (name, k))
    print("mcc %s: %d result lines not byte-identical to regenie's" % (name, total))


def test_cli_mcc_two_parts_equal_one(inputs, tmp_path):
    """Case (a) with --gpus 2 (the flags of the multi-GPU Step-2 tests of tests/test_cli_gpu.py): the same bytes as on one GPU."""
    world = ["--gpus", "2"] + ([] if os.environ.get("RG_TEST_REAL_GPUS") == "1" else ["--single-device"])
    a = mc.args_of("a_bed_all", inputs)
    a[a.index("--bsize") + 1] = "70"
    one, two = _drive(a, tmp_path, "one"), _drive(a + world, tmp_path, "two")
    assert one.returncode == 0 and two.returncode == 0, one.stdout[-2000:] + two.stdout[-3000:] + two.stderr[-2000:]
    assert "GPU 1 : blocks" in two.stdout
    for k in (1, 2):
        x, y = open(str(tmp_path / ("one_Y%d.regenie" % k)), "rb").read(), open(str(tmp_path / ("two_Y%d.regenie" % k)), "rb").read()
        assert x == y and x.count(b"\n") == 401


def test_cli_plain_qt_did_not_move(tmp_path):
    """Without --mcc: the command of tests/test_cli_gpu.py's test_cli_step2_qt_against_reference_output (qt_bed_3chr) against the golden that
    test uses."""
    R = os.path.join(ROOT, "tests", "golden", "ref_outputs")
    with open(str(tmp_path / "pred.list"), "w") as pl:
        for k in (1, 2):
            fn = str(tmp_path / ("ref_%d.loco" % k))
            open(fn, "wb").write(gzip.open(os.path.join(R, "qt_kfold_3chr", "out_%d.loco.gz" % k), "rb").read())
            pl.write("Y%d %s\n" % (k, fn))
    r = _drive(["--step", "2", "--bed", os.path.join(mc.EX, "example_3chr"), "--phenoFile", os.path.join(mc.EX, "phenotype.txt"),
                "--covarFile", os.path.join(mc.EX, "covariates.txt"), "--qt", "--pred", str(tmp_path / "pred.list"), "--bsize", "200"], tmp_path, "s2")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "phenotypic skewness" not in r.stdout
    for k in (1, 2):
        got = open(str(tmp_path / ("s2_Y%d.regenie" % k)), "rb").read()
        ref = gzip.open(os.path.join(R, "step2", "qt_bed_3chr_Y%d.regenie.gz" % k), "rb").read()
        differ = sum(a != b for a, b in zip(got.splitlines(), ref.splitlines()))
        print("plain --qt Y%d: %d lines not byte-identical to the golden" % (k, differ))
        assert got == ref
