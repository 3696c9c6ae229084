"""`regenie-amd --step 2 --compute-corr --bgen` on the GPU against the files regenie itself wrote in dosage mode for the same command
lines (plus the driver's own --ld-dosages, without which dosage input stays refused in LD mode; tests/golden/ref_outputs/ld_dosage, tests/golden/make_ld_dosage_ref_outputs.py), by the rules of tests/test_ld_cli_gpu.py: the
variant lists and the two header integers byte-identical; every 16-bit R^2 value equal, except values the fp64 restatement puts within
1e-6 of a rounding boundary (those may differ by exactly 1, at most 3 per case); text entries within one unit of the sixth digit."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import ld_cases as lc
from tests import ld_dosage_cases as dc
from tests import ld_restate as lr

pytestmark = pytest.mark.gpu
BIN = os.path.join(dc.ROOT, "regenie_amd", "bin", "regenie-amd")


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


def _drive(name, inputs, tmp_path, swap=None):
    args = dc.args_of(name, *inputs)
    if swap:
        args = swap(args)
    return subprocess.run([BIN] + args + ["--ld-dosages", "--out", "o"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("name", ["d1_example400_bin", "d3_synth_chr2_bin", "d5_pgen_bin", "d6_example400_cond_bin"])
def test_cli_binary_corr_against_reference(inputs, tmp_path, name):
    """d3_synth_chr2_bin holds a monomorphic column: it is to be read as the docstring of
    tests/test_ld_cli_gpu.py::test_cli_binary_corr_against_reference explains."""
    r = _drive(name, inputs, tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert " * computing correlation matrix in dosage mode (storing R^2 values)" in r.stdout
    assert "** Computing LD matrix **" in r.stdout and "  -> splitting across " in r.stdout
    assert open(str(tmp_path / "o.corr.snplist"), "rb").read() == _ref(name, "out.corr.snplist")
    got, ref = open(str(tmp_path / "o.corr"), "rb").read(), _ref(name, "out.corr")
    assert got[:8] == ref[:8] and len(got) == len(ref)
    G, X, _, _ = dc.dense_case(name, *inputs)
    _, v64 = lr.quantise(lr.ld_corr(G, X))
    lr.check_binary(np.frombuffer(got[8:], np.uint16), np.frombuffer(ref[8:], np.uint16), v64)
    assert not os.path.exists(str(tmp_path / "o.corr.forcedIn.snplist"))


@pytest.mark.parametrize("name", ["d2_forced153_txt", "d3_synth_chr2_txt", "d5_pgen_txt"])
def test_cli_text_corr_against_reference(inputs, tmp_path, name):
    r = _drive(name, inputs, tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert " * computing correlation matrix in dosage mode\n" in r.stdout
    assert open(str(tmp_path / "o.corr.snplist"), "rb").read() == _ref(name, "out.corr.snplist")
    text = open(str(tmp_path / "o.corr")).read()
    lr.check_text(text, _ref(name, "out.corr").decode())
    R = np.array([[float(t) for t in ln.split()] for ln in text.split("\n")])
    assert np.array_equal(R, R.T)
    if name == "d2_forced153_txt":
        assert open(str(tmp_path / "o.corr.forcedIn.snplist"), "rb").read() == _ref(name, "out.corr.forcedIn.snplist")
        assert "WARNING: there were variants not found in the data; these were kept in the LD matrix." in r.stdout


@pytest.mark.parametrize("kind", ["zstd", "raw"])
def test_cli_host_route_gives_the_device_route_bytes(inputs, tmp_path, kind):
    """d4: the same synthetic data written with zstd compression (and, beside it, without any), which the host threads inflate and walk:
    byte-identical to the driver's own output on the zlib file, which the device decoder serves."""
    (tmp_path / "z").mkdir()
    (tmp_path / kind).mkdir()
    r1 = _drive("d3_synth_chr2_bin", inputs, tmp_path / "z")
    r2 = _drive("d3_synth_chr2_bin", inputs, tmp_path / kind, lambda a: [x.replace("synth.bgen", "synth_%s.bgen" % kind) for x in a])
    assert r1.returncode == 0 and r2.returncode == 0, r2.stdout[-3000:] + r2.stderr[-3000:]
    assert "     - 3 blocks decoded on the device, 0 on the host\n" in r1.stdout
    assert "     - 0 blocks decoded on the device, 3 on the host\n" in r2.stdout
    for fn in ("o.corr", "o.corr.snplist"):
        assert open(str(tmp_path / "z" / fn), "rb").read() == open(str(tmp_path / kind / fn), "rb").read(), fn
