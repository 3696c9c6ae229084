"""`--apply-rerint` / `--apply-rerint-cov` without a GPU: what the host driver decides about the options before any device is touched (regenie's
rules, Regenie.cpp:433-434 and :1251-1252: dropped under --bt and under nothing else, both together an error wherever the flags survive -- step 1
and --ct included --, no effect and no log line outside step 2 of a quantitative trait), and the NumPy restatement of the transformation
(tests/rerint_restate.py) pushed through the Step-2 oracle against the files regenie itself wrote (tests/golden/ref_outputs/rerint).

Bound of the file comparison, as tests/test_mcc_restate_cpu.py: the files carry 6 significant digits, so an exact evaluation sits within 5e-6 of a
printed value; 1e-5 leaves the restatement's own rounding a second half-digit.  The number of rows whose printed digits differ is printed too: it
is asserted to be 0 on every case with a quantitative trait (a - f, h): the cap tests/test_rerint_cli_gpu.py holds the device to."""
import gzip
import os
import subprocess
from statistics import NormalDist

import numpy as np
import pytest

from tests import rerint_cases as rc
from tests import rerint_restate as rr

BIN = os.path.join(rc.ROOT, "regenie_amd", "bin", "regenie-amd")
BOTH = "ERROR: must select one of the two options, --apply-rerint or --apply-rerint-cov"


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from regenie_amd import build
    build.build()
    d = str(tmp_path_factory.mktemp("rerint"))
    rc.write_inputs(d)
    return d


def _drive(args, cwd):
    r = subprocess.run([BIN] + args + ["--out", "o"], cwd=str(cwd), capture_output=True, text=True, timeout=120)
    return r, r.stdout + r.stderr


def _reached_the_device(r, out):
    return r.returncode == 0 or "ERROR: no MI355X" in out


@pytest.mark.parametrize("name", ["a_bed_rerint", "b_bed_cov_cat", "c_bgen_cov", "d_pgen_rerint"])
def test_options_are_accepted_for_quantitative_traits(inputs, tmp_path, name):
    r, out = _drive(rc.args_of(name, inputs), tmp_path)
    assert "unrecognised option" not in out, out[-2000:]
    assert _reached_the_device(r, out), out[-2000:]


def test_both_options_is_the_reference_s_error(inputs, tmp_path):
    r, out = _drive(rc.args_of("a_bed_rerint", inputs) + ["--apply-rerint-cov"], tmp_path)
    assert r.returncode == 1 and BOTH in out.splitlines(), out[-2000:]
    assert not [fn for fn in os.listdir(str(tmp_path)) if fn.endswith(".regenie")]


def test_binary_traits_drop_the_options_even_both(inputs, tmp_path):
    """`!vm.count("bt")`: under --bt neither flag is set, so the pair is no error either."""
    for extra in ([], ["--apply-rerint-cov"]):
        r, out = _drive(rc.args_of("g_bt_ignored", inputs) + extra, tmp_path)
        assert "unrecognised option" not in out and BOTH not in out, out[-2000:]
        assert _reached_the_device(r, out), out[-2000:]


def test_count_traits_keep_the_flags_and_so_the_error(inputs, tmp_path):
    """Only --bt clears the flags: with --ct one option runs (compute_res_count never reads it), both are the error."""
    a = rc.args_of("a_bed_rerint", inputs)
    a[a.index("--qt")] = "--ct"
    r, out = _drive(a, tmp_path)
    assert "unrecognised option" not in out and _reached_the_device(r, out), out[-2000:]
    r, out = _drive(a + ["--apply-rerint-cov"], tmp_path)
    assert r.returncode == 1 and BOTH in out.splitlines(), out[-2000:]


def test_step_1_takes_the_options_and_ignores_them(inputs, tmp_path):
    """regenie sets the flags in step 1 too and nothing there reads them (Data::compute_res alone does): one option changes nothing, both are
    the same error as in step 2."""
    a = ["--step", "1", "--bed", os.path.join(rc.EX, "example_3chr"), "--phenoFile", os.path.join(rc.EX, "phenotype.txt"),
         "--covarFile", os.path.join(rc.EX, "covariates.txt"), "--bsize", "100", "--qt"]
    for opt in ("--apply-rerint", "--apply-rerint-cov"):
        r, out = _drive(a + [opt], tmp_path)
        assert "unrecognised option" not in out and "rerint" not in "".join(ln for ln in out.splitlines() if ln.startswith(("ERROR", "WARNING"))), out[-2000:]
        assert _reached_the_device(r, out), out[-2000:]
    r, out = _drive(a + ["--apply-rerint", "--apply-rerint-cov"], tmp_path)
    assert r.returncode == 1 and BOTH in out.splitlines(), out[-2000:]


def test_regenie_ignores_the_option_for_binary_traits():
    for k in (1, 2):
        a, b = (gzip.open(os.path.join(rc.REF, n, "out_Y%d.regenie.gz" % k), "rb").read() for n in ("g_bt_ignored", "g0_bt_plain"))
        assert a == b and a.count(b"\n") == 401


def test_ranks_are_rint_pheno_s():
    """Blocks of ties share the mean of their positions; kc = 3 / 8 over nvals + 1 / 4."""
    v = np.array([0.5, -1.0, 0.5, 2.0, 0.5, -1.0, 3.0])
    q, r = rr.rint(v)
    assert r.tolist() == [4.0, 1.5, 4.0, 6.0, 4.0, 1.5, 7.0]
    inv = NormalDist().inv_cdf
    assert np.allclose(q, [inv((x - 0.375) / 7.25) for x in r], rtol=1e-14, atol=0)
    assert np.array_equal(rr.rint(v[::-1])[1], r[::-1])


def test_a_constant_trait_is_the_sd_error():
    X = np.ones((40, 1)) / np.sqrt(40.0)
    with pytest.raises(ValueError, match="some phenotype residuals has sd=0."):
        rr.transform(np.full((40, 1), 1.25), X, np.ones((40, 1)), 1)


@pytest.mark.parametrize("name", rc.RESTATED)
def test_restatement_through_the_oracle_reproduces_regenie_files(name):
    res = rr.restate_case(name)
    for k in (1, 2):
        gold, r = rr.golden_columns(name, k), res[k - 1]
        assert len(gold["SE"]) == len(r["logp"]) == (397 if "--condition-list" in rc.CASES[name] else 400) and not np.isnan(r["logp"]).any()
        for col, key in (("LOG10P", "logp"), ("SE", "se"), ("BETA", "beta"), ("CHISQ", "chisq")):
            dev = float(np.max(np.abs(r[key] - gold[col]) / np.abs(gold[col])))
            print("%s Y%d %s: max relative deviation %.3g" % (name, k, col, dev))
            assert dev < 1e-5, (name, k, col, dev)
    d = rr.differing_rows(name)
    print("%s: %d rows whose printed digits differ" % (name, d))
    assert d == 0, (name, d)      # what the cases were chosen for: tests/test_rerint_cli_gpu.py holds the device to the same cap


def test_the_transformation_moves_the_statistics():
    """Case (a) against the same command without the option (tests/golden/ref_outputs/mcc has none; the plain score test of the restatement):
    the fixture is not one the untransformed residuals would reproduce."""
    import tempfile
    from oracle import regenie_step2_qt as s2o
    with tempfile.TemporaryDirectory() as tmp:
        G, X, res0, mask, _ = rr.case_arrays("a_bed_rerint", tmp)
    sd = np.sqrt((res0 ** 2).sum(axis=0)) / np.sqrt(mask.sum(axis=0) - X.shape[1])
    plain = s2o.score_qt_block_ref(G, X, res0 / sd, mask, sd)
    gold = rr.golden_columns("a_bed_rerint", 1)
    assert float(np.max(np.abs(plain["chisq"][:, 0] - gold["CHISQ"]) / gold["CHISQ"])) > 1e-2
