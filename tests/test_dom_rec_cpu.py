"""`--test dominant|recessive [--minHOMs N]` without a GPU: what the host driver decides before any device is touched (the options and the
reference's error texts, tests/golden/ref_outputs/dom_rec/*/meta.json), the host BGEN decode mode against a NumPy decode of the example's file,
and the NumPy restatement of tests/dom_rec_cases.py against the lines regenie itself printed for the quantitative-trait .bed cases -- which keeps
the fixtures and the restatement the GPU library test relies on honest."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import dom_rec_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "regenie_amd", "bin", "regenie-amd")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from regenie_amd import build
    build.build()
    d = str(tmp_path_factory.mktemp("dom_rec"))
    dc.write_inputs(d)
    return d


def _drive(args, cwd):
    return subprocess.run([BIN] + args + ["--out", "o"], cwd=str(cwd), capture_output=True, text=True, timeout=120)


def _meta(name):
    return json.load(open(os.path.join(dc.REF, name, "meta.json")))


@pytest.mark.parametrize("name", dc.ERROR_CASES)
def test_option_errors_of_the_reference(inputs, tmp_path, name):
    meta = _meta(name)
    assert meta["returncode"] == 1 and len(meta["error"]) == 1
    r = _drive(dc.args_of(name, inputs), tmp_path)
    assert r.returncode == 1, r.stdout[-2000:]
    assert meta["error"][0] in (r.stdout + r.stderr).splitlines(), r.stdout[-2000:]
    assert not [fn for fn in os.listdir(str(tmp_path)) if fn.endswith(".regenie")]


def test_option_needs_a_value_and_compute_corr_is_refused(inputs, tmp_path):
    a = dc.args_of("a_qt_dom_bed", inputs)
    r = subprocess.run([BIN] + a[:a.index("--test") + 1], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)      # `--test` as the last word
    assert r.returncode == 1 and "option '--test' needs a value" in r.stdout + r.stderr
    r = _drive(["--step", "2", "--bed", os.path.join(dc.EX, "example_3chr"), "--compute-corr", "--test", "recessive", "--bsize", "100"], tmp_path)
    assert r.returncode == 1 and "--test dominant / recessive with --compute-corr" in r.stdout + r.stderr


def test_min_homs_must_be_a_number_and_pgen_dosage_tracks_are_refused(inputs, tmp_path):
    """`--minHOMs abc`: regenie's option parser says `Argument 'abc' failed to parse` (typographic quotes; checked with its binary).  A .pgen with a
    dosage track under a coding is refused before any device is touched: regenie rounds it to hard calls but keeps the additive zero count of
    check_sparse_G, which the integer-dosage entries do not carry."""
    from tests.util import synth_dosages, write_synth_pgen
    a = dc.args_of("b_qt_rec_minhoms", inputs)
    a[a.index("--minHOMs") + 1] = "abc"
    r = _drive(a, tmp_path)
    assert r.returncode == 1 and "ERROR: Argument \u2018abc\u2019 failed to parse" in (r.stdout + r.stderr).splitlines(), r.stdout[-2000:]
    g = dc.synthetic_calls()
    write_synth_pgen(os.path.join(inputs, "syn_soft"), g, [1] * g.shape[0], seed=3, soft=0.3)
    b = dc.args_of("c_qt_dom_missing", inputs)
    b[b.index("--bed"):b.index("--bed") + 2] = ["--pgen", os.path.join(inputs, "syn_soft")]
    r = _drive(b, tmp_path)
    assert r.returncode == 1 and "on a .pgen file with dosages is not built" in r.stdout + r.stderr, (r.stdout + r.stderr)[-2000:]
    assert not [fn for fn in os.listdir(str(tmp_path)) if fn.endswith(".regenie")]


@pytest.mark.parametrize("name", ["a_qt_dom_bed", "b_qt_rec_minhoms", "d_qt_rec_bgen", "l_qt_additive"])
def test_options_are_known_and_the_log_lines_are_the_reference_s(inputs, tmp_path, name):
    """The run ends at the device (without one: the driver's "no MI355X" error), after the options are read."""
    r = _drive(dc.args_of(name, inputs), tmp_path)
    out = r.stdout + r.stderr
    assert "unrecognised option" not in out, out[-2000:]
    assert r.returncode == 0 or "ERROR: no MI355X" in out, out[-2000:]
    if r.returncode == 0:
        for ln in _meta(name)["log"]:
            assert ln in out.splitlines(), (ln, out[-2000:])


@pytest.fixture(scope="module")
def soft_bgen(tmp_path_factory):
    """The example's file holds hard calls only (probabilities 0 / 1): a small file with genuine probabilities beside it."""
    from tests.util import synth_dosages, write_synth_bgen
    prefix = str(tmp_path_factory.mktemp("dom_rec_bgen") / "soft")
    write_synth_bgen(prefix, synth_dosages(40, 203, miss_rate=0.03, seed=5), [1] * 40, seed=5, soft=0.5)
    return prefix + ".bgen"


@pytest.mark.parametrize("ref_first", [False, True])
@pytest.mark.parametrize("which", ["example", "soft"])
def test_host_bgen_decode_mode(soft_bgen, which, ref_first):
    """rg_bgen_read_dosages_coded against a decode of the file's probability bytes written here (prob = byte / 255, prob2 = max(1 - p0 - p1, 0))."""
    from regenie_amd.bgen import BgenFile
    with BgenFile(os.path.join(dc.EX, "example.bgen") if which == "example" else soft_bgen) as b:
        idx = np.arange(0, b.n_variants, 7)
        blocks = b.read_blocks(idx)
        N = b.n_samples
        miss = (blocks[:, 8:8 + N] & 0x80) != 0
        pr = blocks[:, 10 + N:10 + 3 * N].reshape(len(idx), N, 2).astype(np.float64) / 255.0
        p0, p1 = pr[:, :, 0], pr[:, :, 1]
        p2 = np.maximum(1.0 - p0 - p1, 0.0)
        dos = np.where(miss, -3.0, p1 + 2 * p2 if ref_first else p1 + 2 * p0)
        want = {0: dos, 1: np.where(miss, -3.0, p1 + p2 if ref_first else p0 + p1), 2: np.where(miss, -3.0, p2 if ref_first else p0)}
        assert which == "example" or (((p1 > 0) & (p1 < 1)).any() and miss.any())         # genuine probabilities and missing samples
        for coding in (0, 1, 2):
            rows, coded = b.read_dosages_coded(idx, coding, ref_first=ref_first)
            assert np.array_equal(rows, b.read_dosages(idx, ref_first=ref_first)) and np.array_equal(rows, dos)
            assert np.array_equal(coded, want[coding]), coding
            assert coded[~miss].max() <= 1.0 + 1e-12 or coding == 0


@pytest.fixture(scope="module")
def example_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dom_rec_restate"))
    dc.write_inputs(d)
    return d


def _hold_to_regenie(name, ids, res):
    for k in (1, 2):
        rows = [ln.split(" ") for ln in dc.golden(name, k)]
        c = {h: i for i, h in enumerate(rows[0])}
        printed = ~np.isnan(res["beta"][:, k - 1])
        assert [r[c["ID"]] for r in rows[1:]] == [v for v, p in zip(ids, printed) if p], (name, k)
        for r, j in zip(rows[1:], np.nonzero(printed)[0]):
            assert r[c["A1FREQ"]] == "%g" % res["a1freq"][j, k - 1] and int(r[c["N"]]) == res["n"][j, k - 1], (name, r)
            for col, key in (("BETA", "beta"), ("SE", "se"), ("CHISQ", "chisq")):
                assert float(r[c[col]]) == pytest.approx(res[key][j, k - 1], rel=1e-5, abs=1e-9), (name, col, r)


@pytest.mark.parametrize("name", ["b_qt_rec_minhoms", "c_qt_dom_missing"])
def test_restatement_reproduces_regenie_lines_on_the_synthetic_set(example_dir, name):
    """The cases with missing calls (imputation with the recoded mean), traits that differ in their missing values (per-trait A1FREQ, N and MAC
    filter from additive counts, masked denominators) and `--minHOMs` on both sides of its threshold.  Bound as below."""
    ids, res = dc.restate_synthetic_bed(name, example_dir)
    _hold_to_regenie(name, ids, res)
    printed = {v for v, p in zip(ids, ~np.isnan(res["beta"]).all(axis=1)) if p}
    for row, nhom in dc.HOM_ROWS.items():
        assert (("s%d" % row) in printed) == (name == "c_qt_dom_missing" or nhom >= dc.MIN_HOMS), (row, nhom)
    assert len({tuple(r) for r in res["n"][~np.isnan(res["n"]).any(axis=1)]}) > 1 and (res["counts"][:, 2] > 0).any()      # N differs by trait and row


@pytest.mark.parametrize("name", ["a_qt_dom_bed", "i_qt_rec_ref_first", "l_qt_additive"])
def test_restatement_reproduces_regenie_lines(example_dir, name):
    """Which variants and traits are printed, A1FREQ and N as text, BETA / SE / CHISQ to the printed digits: the files carry 6 significant digits,
    so an exact evaluation sits within 5e-6 of a printed value; 1e-5 leaves the restatement's own rounding a second half-digit."""
    from tests.ld_cases import read_bed
    res = dc.restate_example_bed(name, example_dir)
    _, ids, chrom, _, _ = read_bed(os.path.join(dc.EX, "example_3chr"))
    ids = [v for v, c in zip(ids, chrom) if str(c) == "2"]
    for k in (1, 2):
        rows = [ln.split(" ") for ln in dc.golden(name, k)]
        c = {h: i for i, h in enumerate(rows[0])}
        printed = ~np.isnan(res["beta"][:, k - 1])
        assert [r[c["ID"]] for r in rows[1:]] == [v for v, p in zip(ids, printed) if p], (name, k)
        for r, j in zip(rows[1:], np.nonzero(printed)[0]):
            assert r[c["A1FREQ"]] == "%g" % res["a1freq"][j, k - 1] and int(r[c["N"]]) == res["n"][j, k - 1], (name, r)
            for col, key in (("BETA", "beta"), ("SE", "se"), ("CHISQ", "chisq")):
                assert float(r[c[col]]) == pytest.approx(res[key][j, k - 1], rel=1e-5, abs=1e-9), (name, col, r)
    if name != "l_qt_additive":      # the coding changes the answer: the cases are not the additive test under another name
        add = dc.restate_example_bed("l_qt_additive", example_dir)
        both = ~np.isnan(res["chisq"][:, 0]) & ~np.isnan(add["chisq"][:, 0])
        assert np.median(np.abs(res["chisq"][both, 0] - add["chisq"][both, 0]) / add["chisq"][both, 0]) > 1e-3
