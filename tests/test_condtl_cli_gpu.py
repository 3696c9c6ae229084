"""`regenie-amd --step 2 --condition-list ...` on the GPU against the files regenie itself wrote for the same command lines
(tests/golden/ref_outputs/condtl, tests/golden/make_condtl_ref_outputs.py; the cases: tests/condtl_cases.py), and against the driver's own run
with the same genotype columns handed in as ordinary covariates.

Comparison with regenie's files: tests/condtl_cases.py compare_regenie_files, the rule tests/test_cli_gpu.py applies to each route.  The count of lines
that are not byte-identical is printed per case (profiles/condtl.md holds the last run's)."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from tests import condtl_cases as cc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "regenie_amd", "bin", "regenie-amd")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("condtl"))
    cc.write_inputs(d)
    return d


def _drive(args, cwd, out="o"):
    return subprocess.run([BIN] + args + ["--out", out], cwd=str(cwd), capture_output=True, text=True, timeout=300)


def _meta(name):
    return json.load(open(os.path.join(cc.REF, name, "meta.json")))


@pytest.mark.parametrize("name", cc.FILE_CASES)
def test_cli_condtl_against_reference_files(inputs, tmp_path, name):
    r = _drive(cc.args_of(name, inputs), tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    meta = _meta(name)
    log = r.stdout.replace(inputs, "{D}").splitlines()
    for ln in meta["log"]:
        if "conditioning on variants" in ln or "-n_used" in ln or "-extracting variants" in ln or "specified by --exclude" in ln:
            assert ln in log, (ln, r.stdout[-3000:])
    total = 0
    for k in range(1, cc.traits_of(name) + 1):
        got = open(str(tmp_path / ("o_Y%d.regenie" % k))).read().splitlines()
        ref = gzip.open(os.path.join(cc.REF, name, "out_Y%d.regenie.gz" % k), "rt").read().splitlines()
        total += cc.compare_regenie_files(got, ref, "%s Y%d" % (name, k))
        assert not [ln for ln in got[1:] if ln.split(" ")[2] in cc.EX_COND + cc.SYN_COND]
    print("condtl %s: %d result lines not byte-identical to regenie's" % (name, total))


def test_cli_condtl_list_order_and_duplicates_do_not_matter(inputs, tmp_path):
    """(b): the list out of order, one id twice, a second token on a line -- regenie wrote the files of (a), and so does the driver."""
    for k in (1, 2):
        assert gzip.open(os.path.join(cc.REF, "a_qt_bed", "out_Y%d.regenie.gz" % k), "rb").read() == \
            gzip.open(os.path.join(cc.REF, "b_qt_bed_shuffled", "out_Y%d.regenie.gz" % k), "rb").read()
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    ra, rb = _drive(cc.args_of("a_qt_bed", inputs), tmp_path / "a"), _drive(cc.args_of("b_qt_bed_shuffled", inputs), tmp_path / "b")
    assert ra.returncode == 0 and rb.returncode == 0, ra.stdout[-2000:] + rb.stdout[-2000:]
    for k in (1, 2):
        assert open(str(tmp_path / "a" / ("o_Y%d.regenie" % k)), "rb").read() == open(str(tmp_path / "b" / ("o_Y%d.regenie" % k)), "rb").read()


@pytest.mark.parametrize("name", cc.ERROR_CASES)
def test_cli_condtl_errors_of_the_reference(inputs, tmp_path, name):
    r = _drive(cc.args_of(name, inputs), tmp_path)
    meta = _meta(name)
    assert meta["returncode"] == 1 and len(meta["error"]) == 1
    assert r.returncode == meta["returncode"], r.stdout[-2000:]
    assert meta["error"][0] in (r.stdout + r.stderr).splitlines(), r.stdout[-2000:]
    assert not [fn for fn in os.listdir(str(tmp_path)) if fn.endswith(".regenie")]


def test_cli_condtl_compute_corr_drops_the_conditioning_variants(inputs, tmp_path):
    r = _drive(cc.args_of("k_corr", inputs), tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    snps = open(str(tmp_path / "o.corr.snplist"), "rb").read()
    assert snps == gzip.open(os.path.join(cc.REF, "k_corr", "out.corr.snplist.gz"), "rb").read()
    ids = snps.decode().split()
    assert len(ids) == 397 and not set(ids) & set(cc.EX_COND)
    assert [ln for ln in r.stdout.splitlines() if "+conditioning on variants in [" in ln and ln.endswith("n_used = 3")]
    # the matrix itself: the run that gets the same columns as covariates and the same variants through --extract
    _covariates_with_genotypes(inputs, str(tmp_path / "cov6.txt"))
    with open(str(tmp_path / "keep.txt"), "w") as f:
        f.write("\n".join(ids) + "\n")
    a = cc.args_of("k_corr", inputs)
    i = a.index("--condition-list")
    a = a[:i] + a[i + 2:]
    a[a.index("--covarFile") + 1] = str(tmp_path / "cov6.txt")
    a[a.index("--bed") + 1] = os.path.join(cc.EX, "example_3chr")
    r2 = _drive(a + ["--extract", str(tmp_path / "keep.txt")], tmp_path, out="plain")
    b = cc.args_of("k_corr", inputs)
    b[b.index("--bed") + 1] = os.path.join(cc.EX, "example_3chr")
    r3 = _drive(b, tmp_path, out="cond")
    assert r2.returncode == 0 and r3.returncode == 0, r2.stdout[-2000:] + r3.stdout[-2000:]
    assert open(str(tmp_path / "plain.corr"), "rb").read() == open(str(tmp_path / "cond.corr"), "rb").read()


def _covariates_with_genotypes(inputs, path):
    """The example's covariate file with the calls (0 / 1 / 2 copies of the first .bim allele) of the conditioning variants of example_3chr -- which
    has no missing call -- appended in ascending id order."""
    from tests.ld_cases import read_bed
    G, ids, _, _, fam = read_bed(os.path.join(cc.EX, "example_3chr"))
    assert not np.isnan(G).any()
    rows = {tuple(ln.split()[:2]): ln.split()[2:] for ln in list(open(os.path.join(cc.EX, "covariates.txt")))[1:]}
    with open(path, "w") as f:
        f.write("FID IID V1 V2 V3 " + " ".join("G%d" % (k + 1) for k in range(len(cc.EX_COND))) + "\n")
        for i, s in enumerate(fam):
            f.write("%s %s %s %s\n" % (s[0], s[1], " ".join(rows[s]), " ".join("%d" % G[ids.index(v), i] for v in sorted(cc.EX_COND))))


@pytest.mark.parametrize("world", [[], ["--gpus", "2", "--single-device"]])
def test_cli_condtl_equals_the_same_columns_as_covariates(inputs, tmp_path, world):
    """No reference in this one: conditioning on variants without a missing call is the run that gets their calls as three more covariate columns
    (ascending id order) and --exclude's them -- byte-identical .regenie files, on one GPU and on two parts."""
    _covariates_with_genotypes(inputs, str(tmp_path / "cov6.txt"))
    a = cc.args_of("a_qt_bed", inputs)
    a[a.index("--bed") + 1] = os.path.join(cc.EX, "example_3chr")
    i = a.index("--condition-list")
    b = a[:i] + ["--exclude", a[i + 1]] + a[i + 2:]
    b[b.index("--covarFile") + 1] = str(tmp_path / "cov6.txt")
    ra, rb = _drive(a + world, tmp_path, out="cond"), _drive(b + world, tmp_path, out="plain")
    assert ra.returncode == 0 and rb.returncode == 0, ra.stdout[-2000:] + ra.stderr[-1000:] + rb.stdout[-2000:]
    if world:
        assert "GPU 1 : blocks" in ra.stdout
    for k in (1, 2):
        x, y = open(str(tmp_path / ("cond_Y%d.regenie" % k)), "rb").read(), open(str(tmp_path / ("plain_Y%d.regenie" % k)), "rb").read()
        assert x == y and x.count(b"\n") == 398


def test_cli_condtl_covariate_cap(inputs, tmp_path):
    """62 covariates + 3 conditioning variants + the intercept = 66 columns > RG_S2_MAX_COV: said before any work on the GPU, no output file."""
    a = cc.args_of("a_qt_bed", inputs)
    a[a.index("--covarFile") + 1] = os.path.join(inputs, "ex_cov62.txt")
    r = _drive(a, tmp_path)
    assert r.returncode == 1, r.stdout[-2000:]
    err = [ln for ln in r.stdout.splitlines() if ln.startswith("ERROR")]
    assert len(err) == 1 and "62 covariates" in err[0] and "3 conditioning variants" in err[0] and "at most 64" in err[0], err
    assert sorted(os.listdir(str(tmp_path))) == ["o.log"]
