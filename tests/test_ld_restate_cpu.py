"""tests/ld_restate.py (print_ld on dense numpy arrays) held to the reference's own output files (tests/golden/ref_outputs/ld, written by
regenie itself through tests/golden/make_ld_ref_outputs.py) under the rules the driver is held to: the GPU tests use the restatement at
sizes no fixture covers."""
import gzip
import os

import numpy as np
import pytest

from tests import ld_cases as lc
from tests import ld_restate as lr


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ld"))
    lc.write_synth(os.path.join(d, "synth"))
    lc.write_lists(d)
    return os.path.join(d, "synth"), d


def _ref(name, fn):
    return gzip.open(os.path.join(lc.REF, name, fn + ".gz"), "rb").read()


@pytest.mark.parametrize("name", ["c1_example400_bin", "c3_synth_chr2_bin"])
@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_restatement_reproduces_the_binary_file(inputs, name, dtype):
    G, X, n_samples, cols = lc.dense_case(name, *inputs)
    ns, M, ref = lr.read_corr_bin(_ref(name, "out.corr"))
    assert (ns, M) == (n_samples, len(cols)) and _ref(name, "out.corr.snplist").decode().split() == cols
    _, v64 = lr.quantise(lr.ld_corr(G, X))
    got, _ = lr.quantise(lr.ld_corr(G, X, dtype))
    lr.check_binary(got, ref, v64)


@pytest.mark.parametrize("name", ["c2_forced153_txt", "c3_synth_chr2_txt"])
@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_restatement_reproduces_the_text_file(inputs, name, dtype):
    G, X, _, cols = lc.dense_case(name, *inputs)
    assert _ref(name, "out.corr.snplist").decode().split() == cols
    R = np.asarray(lr.ld_corr(G, X, dtype), dtype=np.float64)
    text = "\n".join(" ".join("%.6g" % v for v in row) for row in R)
    lr.check_text(text, _ref(name, "out.corr").decode())
    if name == "c2_forced153_txt":
        assert _ref(name, "out.corr.forcedIn.snplist").decode().split() == ["absent_A", "absent_B", "absent_C"]
