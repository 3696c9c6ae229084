"""The fixtures of tests/golden/ref_outputs/ld_dosage (regenie's own files in dosage mode) against the fp64 restatement of
tests/ld_restate.py fed with the dosages of oracle.bgen.BgenOracle, by the rules the GPU test holds the driver to: it shows that the
seeds of tests/ld_dosage_cases.py keep the reference itself within the cap of 3 values inside the rounding band."""
import gzip
import json
import os

import numpy as np
import pytest

from tests import ld_cases as lc
from tests import ld_dosage_cases as dc
from tests import ld_restate as lr


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ldd"))
    dc.write_synth(os.path.join(d, "synth"))
    dc.write_synth_pgen(os.path.join(d, "synth_pgen"))
    lc.write_lists(d)
    dc.write_cond(d)
    return os.path.join(d, "synth"), d


def _ref(name, fn):
    return gzip.open(os.path.join(dc.REF, name, fn + ".gz"), "rb").read()


@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_reference_ran_in_dosage_mode(name):
    meta = json.load(open(os.path.join(dc.REF, name, "meta.json")))
    assert meta["returncode"] == 0 and meta["dosage_mode"]


@pytest.mark.parametrize("name", ["d1_example400_bin", "d3_synth_chr2_bin", "d5_pgen_bin", "d6_example400_cond_bin"])
def test_restatement_gives_the_reference_binary(inputs, name):
    G, X, n_samples, cols = dc.dense_case(name, *inputs)
    N, M, ref = lr.read_corr_bin(_ref(name, "out.corr"))
    assert (N, M) == (n_samples, len(cols))
    assert _ref(name, "out.corr.snplist").decode().split() == cols
    q, v = lr.quantise(lr.ld_corr(G, X))
    lr.check_binary(q, ref, v)


@pytest.mark.parametrize("name", ["d2_forced153_txt", "d3_synth_chr2_txt", "d5_pgen_txt"])
def test_restatement_gives_the_reference_text(inputs, name):
    G, X, _, cols = dc.dense_case(name, *inputs)
    assert _ref(name, "out.corr.snplist").decode().split() == cols
    R = lr.ld_corr(G, X)
    text = "\n".join(" ".join("%.6g" % (v + 0.0) for v in row) for row in R)
    lr.check_text(text, _ref(name, "out.corr").decode())
