"""`regenie-amd --step 2 --bt --af-cc` on the GPU against the files regenie itself wrote for the same command lines (tests/golden/ref_outputs/af_cc,
tests/golden/make_afcc_ref_outputs.py; the cases: tests/afcc_cases.py).  Every line of every file is compared byte for byte; the number of lines
that differ is printed before the assertion.  Every run with the option ends at `unrecognised option '--af-cc'` on a driver without the feature."""
import os
import subprocess

import pytest

from tests import afcc_cases as ac

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "regenie_amd", "bin", "regenie-amd")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("afcc"))
    ac.write_inputs(d)
    return d


def _drive(args, cwd, out="o", env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([BIN] + args + ["--out", out], cwd=str(cwd), capture_output=True, text=True, timeout=300, env=e)


def _files(tmp_path, prefix="o"):
    return [open(str(tmp_path / ("%s_Y%d.regenie" % (prefix, k)))).read().splitlines() for k in range(1, ac.P + 1)]


def _compare(got, name):
    bad, first = 0, None
    for k in range(ac.P):
        ref = ac.golden(name, k + 1)
        assert len(got[k]) == len(ref), (name, k, len(got[k]), len(ref))
        for a, b in zip(got[k], ref):
            if a != b:
                bad += 1
                first = first or (k + 1, a, b)
    print("af_cc %s: %d of %d lines not byte-identical to regenie's%s" % (name, bad, sum(len(f) for f in got), "" if not first else "; first: %r" % (first,)))
    assert bad == 0, (name, bad, first)


@pytest.mark.parametrize("name", ac.ACTIVE)
def test_cli_afcc_against_reference_files(inputs, tmp_path, name):
    r = _drive(ac.args_of(name, inputs), tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert ac.WARNING not in r.stdout
    _compare(_files(tmp_path), name)


@pytest.mark.parametrize("name", ac.DISABLED)
def test_cli_afcc_disabled_modes_warn_and_write_no_columns(inputs, tmp_path, name):
    r = _drive(ac.args_of(name, inputs), tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(ac.WARNING + "\n") == 1
    got = _files(tmp_path)
    r = _drive(ac.args_of(name, inputs, af_cc=False), tmp_path, out="p")
    assert r.returncode == 0 and ac.WARNING not in r.stdout
    assert got == _files(tmp_path, "p")                              # byte-identical to the run without the option
    _compare(got, name)


@pytest.mark.parametrize("name", ["a_bed", "f_bgen", "i_bed_par"])
def test_cli_afcc_two_parts_on_one_device(inputs, tmp_path, name):
    r = _drive(ac.args_of(name, inputs), tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r2 = _drive(ac.args_of(name, inputs) + ["--gpus", "2", "--single-device"], tmp_path, out="g2")
    assert r2.returncode == 0, r2.stdout[-3000:] + r2.stderr[-3000:]
    assert "GPU 1 : blocks" in r2.stdout
    assert _files(tmp_path, "g2") == _files(tmp_path)


@pytest.mark.parametrize("env", [{"RG_S2_BGEN_HOST": "1"}, {"RG_S2_BGEN_ROWS": "1"}])
@pytest.mark.parametrize("name", ["f_bgen", "g_bgen_firth"])
def test_cli_afcc_bgen_host_routes_equal_the_device_route(inputs, tmp_path, name, env):
    r = _drive(ac.args_of(name, inputs), tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rh = _drive(ac.args_of(name, inputs), tmp_path, out="h", env=env)
    assert rh.returncode == 0, rh.stdout[-3000:] + rh.stderr[-3000:]
    assert _files(tmp_path, "h") == _files(tmp_path)


@pytest.mark.parametrize("name", ["a_bed", "f_bgen"])
def test_cli_without_the_option_writes_what_it_wrote_before(inputs, tmp_path, name):
    """The same command without --af-cc: regenie's file of that command (what the driver wrote before the option existed), byte for byte, and the
    --af-cc file minus its four columns."""
    r = _drive(ac.args_of(name, inputs, af_cc=False), tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    got = _files(tmp_path)
    _compare(got, name + "_plain")
    r = _drive(ac.args_of(name, inputs), tmp_path, out="w")
    assert r.returncode == 0
    assert [ac.strip_afcc(f) for f in _files(tmp_path, "w")] == got


def test_cli_afcc_other_combinations(inputs, tmp_path):
    """--gz, --write-null-firth / --use-null-firth and a dominant test on BGEN (the general rows: the device decoder's rows hold coded values) keep
    the columns of the plain run: they depend on the additive calls, the masks and the phenotypes alone."""
    import gzip
    base = ac.args_of("a_bed", inputs)
    r = _drive(base + ["--gz"], tmp_path, out="z")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for k in range(1, ac.P + 1):
        assert gzip.open(str(tmp_path / ("z_Y%d.regenie.gz" % k)), "rt").read().splitlines() == ac.golden("a_bed", k)
    r = _drive(ac.args_of("b_bed_firth", inputs) + ["--write-null-firth"], tmp_path, out="wn")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = _drive(ac.args_of("b_bed_firth", inputs) + ["--use-null-firth", str(tmp_path / "wn_firth.list")], tmp_path, out="un")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    cols = lambda f: [[t for k, t in enumerate(ln.split(" ")) if k in (2, 6, 7, 9, 10)] for ln in f]      # ID and the four columns
    want = [cols(ac.golden("a_bed", k)) for k in range(1, ac.P + 1)]
    assert [cols(f) for f in _files(tmp_path, "wn")] == want and [cols(f) for f in _files(tmp_path, "un")] == want
    r = _drive(ac.args_of("f_bgen", inputs) + ["--test", "dominant"], tmp_path, out="dom")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ref = {k: {ln.split(" ")[2]: ln.split(" ") for ln in ac.golden("f_bgen", k)} for k in range(1, ac.P + 1)}
    for k, f in enumerate(_files(tmp_path, "dom"), 1):
        assert len(f) > 100
        for ln in f[1:]:
            t = ln.split(" ")
            assert [t[6], t[7], t[10], t[11]] == [ref[k][t[2]][i] for i in (6, 7, 10, 11)] and t[12] == "DOM", ln


def test_cli_afcc_control_case_coded_1_2(inputs, tmp_path):
    """--1: the same phenotypes coded 1 = control, 2 = case give regenie's files of the 0 / 1 coding, byte for byte (y_p of update_af_cc is the
    0 / 1 phenotype after --1)."""
    y, miss = ac.phenotypes()
    with open(os.path.join(inputs, "a12.pheno"), "w") as f:
        f.write("FID IID Y1 Y2 Y3\n")
        for i in range(ac.N):
            f.write("%d %d %s\n" % (i + 1, i + 1, " ".join("NA" if miss[i, k] else str(y[i, k] + 1) for k in range(ac.P))))
    args = [os.path.join(inputs, "a12.pheno") if a.endswith("a.pheno") else a for a in ac.args_of("a_bed", inputs)] + ["--1"]
    r = _drive(args, tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    _compare(_files(tmp_path), "a_bed")


def test_cli_afcc_min_case_count_drops_a_trait(inputs, tmp_path):
    """--minCaseCount 20 drops Y3 (15 cases): no file for it, and the four columns of the traits that stay are those of the NumPy restatement of
    update_af_cc / compute_aaf_info for THEIR cases and masks, as text, on every line."""
    r = _drive(ac.args_of("a_bed", inputs) + ["--minCaseCount", "20"], tmp_path, out="mc")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert not os.path.exists(str(tmp_path / "mc_Y3.regenie"))
    q, scale = ac.genotypes_of("a_bed", ac.calls())
    y, miss = ac.phenotypes()
    want = ac.afcc_columns(q, scale, y, ~miss)
    for k in (0, 1):
        f = open(str(tmp_path / ("mc_Y%d.regenie" % (k + 1)))).read().splitlines()
        assert f[0].split(" ")[6:11] == ["A1FREQ_CASES", "A1FREQ_CONTROLS", "N", "N_CASES", "N_CONTROLS"] and len(f) > 100
        for ln in f[1:]:
            t = ln.split(" ")
            j = int(t[2][1:])
            assert [t[6], t[7], t[9], t[10]] == [w[j, k] for w in want], ln
