"""`regenie-amd --step 2 --qt --apply-rerint | --apply-rerint-cov ...` on the GPU against the files regenie itself wrote for the same command lines
(tests/golden/ref_outputs/rerint, tests/golden/make_rerint_ref_outputs.py; the cases: tests/rerint_cases.py).

Comparison: tests/condtl_cases.py compare_regenie_files, as tests/test_mcc_cli_gpu.py -- a line that is not byte-identical must match to the printed
digits at 2e-5.  On top of it the cap of this feature: ZERO lines that are not byte-identical.  The NumPy restatement met that cap against regenie's
files on the CPU when the fixtures were generated (every restated case: 0 rows), so a flipped last digit here is a finding about the device's
arithmetic, not about the cases."""
import gzip
import os
import subprocess

import pytest

from tests import rerint_cases as rc
from tests.condtl_cases import compare_regenie_files

pytestmark = pytest.mark.gpu
BIN = os.path.join(rc.ROOT, "regenie_amd", "bin", "regenie-amd")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("rerint"))
    rc.write_inputs(d)
    return d


def _drive(args, cwd, out="o"):
    return subprocess.run([BIN] + args + ["--out", out], cwd=str(cwd), capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("name", list(rc.CASES))
def test_cli_rerint_against_reference_files(inputs, tmp_path, name):
    r = _drive(rc.args_of(name, inputs), tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    total = 0
    for k in (1, 2):
        got = open(str(tmp_path / ("o_Y%d.regenie" % k))).read().splitlines()
        ref = gzip.open(os.path.join(rc.REF, name, "out_Y%d.regenie.gz" % k), "rt").read().splitlines()
        total += compare_regenie_files(got, ref, "%s Y%d" % (name, k))
    print("rerint %s: %d result lines not byte-identical to regenie's" % (name, total))
    if name in rc.QT_CASES:
        assert total == 0, (name, total)


def test_cli_binary_traits_with_the_option_are_the_run_without_it(inputs, tmp_path):
    """Case (g): the driver's own files of `--bt --apply-rerint` and of the same command without the option, byte for byte."""
    a, b = _drive(rc.args_of("g_bt_ignored", inputs), tmp_path, "with"), _drive(rc.args_of("g0_bt_plain", inputs), tmp_path, "without")
    assert a.returncode == 0 and b.returncode == 0, a.stdout[-2000:] + b.stdout[-2000:]
    for k in (1, 2):
        x, y = open(str(tmp_path / ("with_Y%d.regenie" % k)), "rb").read(), open(str(tmp_path / ("without_Y%d.regenie" % k)), "rb").read()
        assert x == y and x.count(b"\n") == 401


def test_cli_rerint_two_parts_equal_one(inputs, tmp_path):
    """Case (b) with --gpus 2 (the flags of the multi-GPU Step-2 tests of tests/test_cli_gpu.py): every part transforms the residuals on its own
    context, and the files are the bytes of the one-GPU run."""
    world = ["--gpus", "2"] + ([] if os.environ.get("RG_TEST_REAL_GPUS") == "1" else ["--single-device"])
    a = rc.args_of("b_bed_cov_cat", inputs)
    a[a.index("--bsize") + 1] = "70"
    one, two = _drive(a, tmp_path, "one"), _drive(a + world, tmp_path, "two")
    assert one.returncode == 0 and two.returncode == 0, one.stdout[-2000:] + two.stdout[-3000:] + two.stderr[-2000:]
    assert "GPU 1 : blocks" in two.stdout
    for k in (1, 2):
        x, y = open(str(tmp_path / ("one_Y%d.regenie" % k)), "rb").read(), open(str(tmp_path / ("two_Y%d.regenie" % k)), "rb").read()
        assert x == y and x.count(b"\n") == 401
