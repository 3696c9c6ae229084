"""`regenie-amd --step 2 --output-corr-text --skip-scaleG [--sparse-thr t]` on the GPU against the files regenie itself wrote for the same
command lines (tests/golden/ref_outputs/ld_gtg, tests/golden/make_ld_gtg_ref_outputs.py).  Equality rules: the variant lists and the
header line byte-identical; dense entries and the sd line within one unit of the sixth printed digit (tests/ld_restate.py: check_text);
the (i, j) columns of the triplets exactly equal, their values within one unit of the sixth printed digit
(tests/ld_gtg_restate.py: check_sparse; tests/test_ld_gtg_restate_cpu.py guards the thresholds that make exact equality a fair demand)."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import ld_cases as lc
from tests import ld_gtg_cases as gc
from tests import ld_gtg_restate as gr
from tests import ld_restate as lr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "regenie_amd", "bin", "regenie-amd")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ld_gtg"))
    lc.write_synth(os.path.join(d, "synth"))
    lc.write_lists(d)
    return os.path.join(d, "synth"), d


def _ref(name, fn):
    return gzip.open(os.path.join(gc.REF, name, fn + ".gz"), "rb").read()


def _drive(name, inputs, tmp_path, swap=None):
    args = gc.args_of(name, *inputs)
    if swap:
        args = swap(args)
    return subprocess.run([BIN] + args + gc.DRIVER_EXTRA.get(name, []) + ["--out", "o"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_cli_gtg_against_reference(inputs, tmp_path, name):
    r = _drive(name, inputs, tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "(=GtG)" in r.stdout
    assert open(str(tmp_path / "o.corr.snplist"), "rb").read() == _ref(name, "out.corr.snplist")
    got, ref = open(str(tmp_path / "o.corr")).read(), _ref(name, "out.corr").decode()
    assert got.split("\n", 1)[0] == ref.split("\n", 1)[0]
    if name in gc.SPARSE:
        gr.check_sparse(got, ref)
    else:
        assert not got.endswith("\n")
        lr.check_text(got.split("\n", 1)[1], ref.split("\n", 1)[1])
    forced = str(tmp_path / "o.corr.forcedIn.snplist")
    if name == "b_forced153_thr20":
        assert open(forced, "rb").read() == _ref(name, "out.corr.forcedIn.snplist")
        sd = got.split("\n")[1].split(" ")
        cols = _ref(name, "out.corr.snplist").decode().split()
        assert [sd[cols.index(v)] for v in ("absent_A", "absent_B", "absent_C")] == ["0.001"] * 3      # sqrt(numtol)
    else:
        assert not os.path.exists(forced)


def test_cli_gtg_pgen_hardcalls_give_the_bed_bytes(inputs, tmp_path):
    """Case (c) as a hard-call .pgen: byte-identical to the driver's own .bed output."""
    from oracle import pgen as opg
    name = "c_synth_chr2_thr05"
    S, d = inputs
    G, ids, chroms, pos, fam = lc.read_bed(S)
    P = os.path.join(d, "synth_pgen")
    alt = np.where(np.isnan(G), 3, G).astype(np.uint8)      # .pgen codes (ALT count, 3 = missing); the first .bim allele is written as ALT
    opg.write_pgen_fixed(P + ".pgen", alt)
    with open(P + ".pvar", "w") as f:
        f.write("#CHROM\tPOS\tID\tREF\tALT\n")
        for j in range(len(ids)):
            f.write("%d\t%d\t%s\tG\tA\n" % (chroms[j], pos[j], ids[j]))
    with open(P + ".psam", "w") as f:
        f.write("#FID\tIID\tSEX\n")
        for a, b in fam:
            f.write("%s\t%s\t0\n" % (a, b))
    (tmp_path / "bed").mkdir()
    (tmp_path / "pgen").mkdir()
    r1 = _drive(name, inputs, tmp_path / "bed")

    def swap(args):
        i = args.index("--bed")
        return args[:i] + ["--pgen", P] + args[i + 2:]
    r2 = _drive(name, inputs, tmp_path / "pgen", swap)
    assert r1.returncode == 0 and r2.returncode == 0, r2.stdout[-3000:] + r2.stderr[-3000:]
    assert "(=GtG)" in r2.stdout
    for fn in ("o.corr", "o.corr.snplist"):
        a, b = open(str(tmp_path / "bed" / fn), "rb").read(), open(str(tmp_path / "pgen" / fn), "rb").read()
        assert a == b and len(a) > 0, fn
