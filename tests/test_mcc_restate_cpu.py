"""The NumPy restatement of the moment-matched test (tests/mcc_restate.py) against the LOG10P and SE columns regenie itself printed for cases (a)
and (d) of tests/mcc_cases.py -- an independent fp64 evaluation next to the reference, on the CPU.  The figures are recorded in profiles/mcc.md.
Bound: the files carry 6 significant digits, so an exact evaluation sits within 5e-6 of a printed value; 1e-5 leaves the restatement's own
rounding (sums of ~460 terms, a gamma tail) a second half-digit."""
import numpy as np
import pytest

from tests import mcc_restate as mr


@pytest.fixture(scope="module", params=["a_bed_all", "d_bgen_all"])
def case(request):
    return request.param, mr.restate_case(request.param)


def test_restatement_reproduces_regenie_columns(case):
    name, res = case
    for k in (1, 2):
        gold, r = mr.golden_columns(name, k), res[k - 1]
        keep = ~np.isnan(r["logp"])
        assert keep.sum() == len(gold["SE"]) == 400
        for col, key in (("LOG10P", "logp"), ("SE", "se"), ("BETA", "beta"), ("CHISQ", "chisq")):
            dev = float(np.max(np.abs(r[key][keep] - gold[col]) / np.abs(gold[col])))
            print("%s Y%d %s: max relative deviation %.3g" % (name, k, col, dev))
            assert dev < 1e-5, (name, k, col, dev)


def test_no_golden_row_is_outside_the_gamma_fit(case):
    name, res = case
    for r in res:
        keep = ~np.isnan(r["skew"])
        assert (r["skew"][keep] > 0).all() and ((r["p"][keep] > 0) & (r["p"][keep] < 1)).all()
