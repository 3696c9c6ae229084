"""`regenie-amd --step 2 --compute-corr` on the GPU against the files regenie itself wrote for the same command lines
(tests/golden/ref_outputs/ld, tests/golden/make_ld_ref_outputs.py).  Equality rules (tests/ld_restate.py): the variant lists and the two
header integers byte-identical; every 16-bit R^2 value equal, except values the fp64 restatement puts within 1e-6 of a rounding boundary
(those may differ by exactly 1, at most 3 per case); text entries within one unit of the sixth printed digit."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import ld_cases as lc
from tests import ld_restate as lr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "regenie_amd", "bin", "regenie-amd")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ld"))
    G, chroms = lc.write_synth(os.path.join(d, "synth"))
    lc.write_lists(d)
    return os.path.join(d, "synth"), d


def _ref(name, fn):
    return gzip.open(os.path.join(lc.REF, name, fn + ".gz"), "rb").read()


def _drive(name, inputs, tmp_path, swap=None):
    args = lc.args_of(name, *inputs)
    if swap:
        args = swap(args)
    r = subprocess.run([BIN] + args + ["--out", "o"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    return r


@pytest.mark.parametrize("name", ["c1_example400_bin", "c3_synth_chr2_bin"])
def test_cli_binary_corr_against_reference(inputs, tmp_path, name):
    """c3_synth_chr2_bin holds the two degenerate columns (a monomorphic variant, a variant observed in two samples).  The monomorphic one has
    LD_ii = rounding noise: the fixture pins it because that noise came out <= 0 in regenie's run and comes out <= 0 here, so both sides put
    sqrt(numtol) on the diagonal and the column's R^2 values quantise to 0.  Were the noise to land above 0 on either side (another
    summation order, another basis), that column's correlations would be noise over noise and could differ without either program being
    wrong: a failure confined to column 201 of this case is to be read that way, any other difference is not."""
    r = _drive(name, inputs, tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert open(str(tmp_path / "o.corr.snplist"), "rb").read() == _ref(name, "out.corr.snplist")
    got, ref = open(str(tmp_path / "o.corr"), "rb").read(), _ref(name, "out.corr")
    assert got[:8] == ref[:8] and len(got) == len(ref)
    G, X, _, _ = lc.dense_case(name, *inputs)
    _, v64 = lr.quantise(lr.ld_corr(G, X))
    lr.check_binary(np.frombuffer(got[8:], np.uint16), np.frombuffer(ref[8:], np.uint16), v64)
    assert not os.path.exists(str(tmp_path / "o.corr.forcedIn.snplist"))


@pytest.mark.parametrize("name", ["c2_forced153_txt", "c3_synth_chr2_txt"])
def test_cli_text_corr_against_reference(inputs, tmp_path, name):
    r = _drive(name, inputs, tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert open(str(tmp_path / "o.corr.snplist"), "rb").read() == _ref(name, "out.corr.snplist")
    lr.check_text(open(str(tmp_path / "o.corr")).read(), _ref(name, "out.corr").decode())
    if name == "c2_forced153_txt":
        assert open(str(tmp_path / "o.corr.forcedIn.snplist"), "rb").read() == _ref(name, "out.corr.forcedIn.snplist")
        assert "WARNING: there were variants not found in the data; these were kept in the LD matrix." in r.stdout


@pytest.mark.parametrize("name", ["c3_synth_chr2_bin", "c3_synth_chr2_txt"])
def test_cli_pgen_hardcalls_give_the_bed_bytes(inputs, tmp_path, name):
    """The same data as a hard-call .pgen: byte-identical to the driver's own .bed output."""
    from oracle import pgen as opg
    S, d = inputs
    G, ids, chroms, pos, fam = lc.read_bed(S)
    P = os.path.join(d, "synth_pgen")
    if not os.path.exists(P + ".pgen"):
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
    for fn in ("o.corr", "o.corr.snplist"):
        assert open(str(tmp_path / "bed" / fn), "rb").read() == open(str(tmp_path / "pgen" / fn), "rb").read(), fn


def test_cli_range_and_chrlist(inputs, tmp_path):
    r = _drive("c4_range", inputs, tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    snps = open(str(tmp_path / "o.corr.snplist"), "rb").read()
    assert snps == _ref("c4_range", "out.corr.snplist") and len(snps.split()) == 250
    (tmp_path / "b").mkdir()
    r = _drive("c4_chrlist_fails", inputs, tmp_path / "b")
    assert r.returncode != 0 and "ERROR: can only compute LD matrix for a single chromosome (use --chr/--chrList/--range)." in r.stdout + r.stderr


def test_cli_step2_qt_chr_filter_against_reference(tmp_path):
    """--chr outside LD mode: `--step 2 --qt --chr 2` against regenie's .regenie files, compared as tests/test_cli_gpu.py's
    test_cli_step2_qt_against_reference_output compares them."""
    E, R = lc.EX, os.path.join(ROOT, "tests", "golden", "ref_outputs")
    with open(str(tmp_path / "pred.list"), "w") as pl:
        for k in (1, 2):
            fn = str(tmp_path / ("ref_%d.loco" % k))
            open(fn, "wb").write(gzip.open(os.path.join(R, "qt_kfold_3chr", "out_%d.loco.gz" % k), "rb").read())
            pl.write("Y%d %s\n" % (k, fn))
    r = subprocess.run([BIN, "--step", "2", "--bed", os.path.join(E, "example_3chr"), "--phenoFile", os.path.join(E, "phenotype.txt"),
                        "--covarFile", os.path.join(E, "covariates.txt"), "--qt", "--pred", str(tmp_path / "pred.list"), "--out", "s2", "--bsize", "200",
                        "--chr", "2"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for k in (1, 2):
        got = open(str(tmp_path / ("s2_Y%d.regenie" % k))).read().splitlines()
        ref = _ref("c5_qt_chr2", "out_Y%d.regenie" % k).decode().splitlines()
        assert got[0] == ref[0] and len(got) == len(ref) and len(ref) > 100
        same = 0
        for a, b in zip(got[1:], ref[1:]):
            ta, tb = a.split(" "), b.split(" ")
            assert ta[:8] == tb[:8] and ta[12] == tb[12] == "NA", (a, b)
            for x, y in zip(ta[8:12], tb[8:12]):
                assert float(x) == pytest.approx(float(y), rel=2e-5, abs=2e-9), (a, b)
            same += a == b
        assert same >= 0.9 * (len(ref) - 1), same
