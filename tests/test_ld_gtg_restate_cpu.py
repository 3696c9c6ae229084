"""tests/ld_gtg_restate.py (the `--skip-scaleG` branches of print_ld on dense numpy arrays) held to the reference's own output files
(tests/golden/ref_outputs/ld_gtg, written by regenie itself through tests/golden/make_ld_gtg_ref_outputs.py): the header line
byte-identical, dense entries and sd values within one unit of the sixth printed digit, the kept pairs exactly the reference's.  It also
guards the thresholds of the sparse cases: no pair's restated |r| lies within 1e-9 of the threshold, which is what lets the GPU tests ask
for exactly the reference's pairs."""
import gzip
import os

import numpy as np
import pytest

from tests import ld_cases as lc
from tests import ld_gtg_cases as gc
from tests import ld_gtg_restate as gr
from tests import ld_restate as lr


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ld_gtg"))
    lc.write_synth(os.path.join(d, "synth"))
    lc.write_lists(d)
    return os.path.join(d, "synth"), d


def _ref(name, fn):
    return gzip.open(os.path.join(gc.REF, name, fn + ".gz"), "rb").read()


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_restatement_reproduces_the_dense_file(inputs, dtype):
    name = "a_example400_gtg"
    G, X, n_samples, cols = gc.dense_case(name, *inputs)
    assert _ref(name, "out.corr.snplist").decode().split() == cols
    got, ref = gr.text_dense(gr.gtg(G, X, dtype), n_samples), _ref(name, "out.corr").decode()
    assert not ref.endswith("\n")
    assert got.split("\n", 1)[0] == ref.split("\n", 1)[0] == "%d %d" % (len(cols), n_samples)
    lr.check_text(got.split("\n", 1)[1], ref.split("\n", 1)[1])


@pytest.mark.parametrize("name", sorted(gc.SPARSE))
@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_restatement_reproduces_the_sparse_file(inputs, name, dtype):
    thr = gc.SPARSE[name]
    G, X, n_samples, cols = gc.dense_case(name, *inputs)
    assert _ref(name, "out.corr.snplist").decode().split() == cols
    sd, row, col, val, every = gr.sparse_of(gr.gtg(G, X, dtype), dtype(thr))
    gap = float(np.min(np.abs(np.abs(every) - dtype(thr))))
    print("%s: %d of %d pairs kept, the nearest |r| is %.3g from the threshold %g" % (name, len(row), len(every), gap, thr))
    assert gap > 1e-9, "a pair sits on the threshold: choose another threshold for this case"
    ref = _ref(name, "out.corr").decode()
    assert ref.startswith(gr.header(len(cols), n_samples))
    assert gr.check_sparse(gr.text_sparse(sd, row, col, val, n_samples), ref) == len(row)
    if name == "b_forced153_thr20":      # a forced-in column: sd = sqrt(numtol), no pair
        forced = [cols.index(v) for v in _ref(name, "out.corr.forcedIn.snplist").decode().split()]
        assert len(forced) == 3 and np.all(np.asarray(sd, dtype=np.float64)[forced] == np.sqrt(lr.NUMTOL))
        assert not np.isin(row, forced).any() and not np.isin(col, forced).any()
