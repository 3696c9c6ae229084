#!/usr/bin/env python
"""TEST INFRASTRUCTURE.  Generates tests/golden/ref_outputs/chrx/: the output FILES of regenie v4.1.2 itself (oracle/_ref/regenie, built by
oracle/Makefile) for the chromosome-X cases of tests/chrx_cases.py, every one with an explicit `--par-region`, gzipped, with the command line, the
exit status and the variants its het-male warning names in meta.json.  It also checks what the inputs are built to exercise and records it
(meta.json "conditions"; tests/test_chrx_cpu.py asserts the same from the inputs):
  - in every case with sex codes at least 10 non-PAR variants are kept by the autosomal rule and absent from regenie's files;
  - in the differing-missingness cases at least 5 (variant, trait) tests are absent while their variant is printed for the other trait;
  - in the Firth case a flagged sparse (variant, trait) pair has an autosomal per-trait MAC >= 50 and a sex-aware one < 50;
  - at least 10 PAR variants and all of chromosome 22 are printed, byte-identical to the run on the same genotypes without sex codes.

  python tests/golden/make_chrx_ref_outputs.py      # needs oracle/_ref/regenie (make -C oracle)
"""
import gzip
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import chrx_cases as xc      # noqa: E402

REGENIE = os.path.join(ROOT, "oracle", "_ref", "regenie")
CHI2 = {0.9: 0.0157908, 0.05: 3.8414588}


def store(dst, name, data):
    with open(os.path.join(dst, name + ".gz"), "wb") as f:
        f.write(gzip.compress(data, 9, mtime=0))


def conditions(name, tmp, g, gh):
    """What the case shows, from regenie's files and the inputs."""
    r = xc.expected_sets(name, tmp, g, gh)
    npar = xc.non_par(xc.build_of(name))
    ids = [{ln.split(" ")[2] for ln in xc.golden(name, k + 1)[1:]} for k in range(xc.P)]
    c = {"lines": [len(s) for s in ids]}
    if name not in ("g_qt_rec",):      # (the recessive test has filters of its own on top)
        for k in range(xc.P):
            assert ids[k] == r["keep"][k], (name, k, sorted(ids[k] ^ r["keep"][k]))
    dropped = [j for j in range(xc.M) if npar[j] and r["auto_all"][j, 0] >= xc.MIN_MAC and r["sex_all"][j, 0] < xc.MIN_MAC]
    if name[1] == "_":
        assert len(dropped) >= 10 and not any(("s%d" % j) in ids[0] | ids[1] for j in dropped), (name, dropped)
        c["dropped_variants"] = ["s%d" % j for j in dropped]
        flipped = [("s%d" % j, k + 1) for j in range(xc.M) for k in range(xc.P)
                   if r["sex_all"][j, 0] >= xc.MIN_MAC and r["auto_trait"][j, k] >= xc.MIN_MAC and r["sex_trait"][j, k] < xc.MIN_MAC]
        if "xq.pheno" in " ".join(xc.CASES[name]) and name != "g_qt_rec":
            assert len(flipped) >= 5 and all(v not in ids[k - 1] and v in ids[2 - k] for v, k in flipped), (name, flipped)
        c["flipped_tests"] = flipped
    if name in xc.NOSEX_OF:
        twin = xc.NOSEX_OF[name]
        same = 0
        for k in range(xc.P):
            other = {ln.split(" ")[2]: ln for ln in xc.golden(twin, k + 1)[1:]}
            for ln in xc.golden(name, k + 1)[1:]:
                v = ln.split(" ")[2]
                if not npar[int(v[1:])]:
                    assert other[v] == ln, (name, ln, other[v])
                    same += 1
        par = [j for j in range(xc.M) if xc.CHROMS[j] == 23 and not npar[j] and ("s%d" % j) in ids[0]]
        c22 = [j for j in range(xc.M) if xc.CHROMS[j] == 22]
        assert len(par) >= 10 and all(("s%d" % j) in ids[0] for j in c22), name
        c["par_variants_tested"], c["chr22_variants_tested"], c["lines_identical_to_nosex_run"] = len(par), len(c22), same
    if name == "d_bt_firth":
        score = [{ln.split(" ")[2]: ln.split(" ") for ln in xc.golden(xc.SCORE_OF[name], k + 1)[1:]} for k in range(xc.P)]
        pairs = []
        for j in xc.F50:
            for k in range(xc.P):
                t = score[k].get("s%d" % j)
                nz = int((g[j] > 0).sum())
                if t and t[-3] != "NA" and float(t[-3]) > CHI2[xc.PTHRESH[name]] and nz <= xc.N * 0.5 and r["auto_trait"][j, k] >= 50 and r["sex_trait"][j, k] < 50:
                    pairs.append(("s%d" % j, k + 1, float(r["auto_trait"][j, k]), float(r["sex_trait"][j, k])))
        assert pairs, name
        c["firth_pairs_autosomal_ge_50_sex_aware_lt_50"] = pairs
    return c


def main():
    with tempfile.TemporaryDirectory() as tmp:
        g, gh = xc.write_inputs(tmp)
        metas = {}
        for name in xc.CASES:
            dst = os.path.join(xc.REF, name)
            os.makedirs(dst, exist_ok=True)
            args = xc.args_of(name, tmp) + ["--threads", "2", "--out", os.path.join(tmp, name)]
            r = subprocess.run([REGENIE] + args, capture_output=True, text=True)
            assert r.returncode == 0, (name, r.stdout[-2000:], r.stderr[-2000:])
            het = sorted(set(re.findall(r"male on chrX at (\S+) \(males", r.stderr)), key=lambda v: int(v[1:]))
            for m in re.findall(r"at variants \[([^\]]*)\]", r.stderr):
                het = sorted(set(het) | set(m.split(";")), key=lambda v: int(v[1:]))
            metas[name] = {"cmd": [a.replace(tmp, "{D}") for a in args], "returncode": r.returncode, "par_region": xc.build_of(name),
                           "bounds": list(xc.par_bounds(xc.build_of(name))), "het_male_variants": het}
            for k in range(1, xc.P + 1):
                store(dst, "out_Y%d.regenie" % k, open(os.path.join(tmp, "%s_Y%d.regenie" % (name, k)), "rb").read())
        for name in xc.CASES:
            metas[name]["conditions"] = conditions(name, tmp, g, gh)
            json.dump(metas[name], open(os.path.join(xc.REF, name, "meta.json"), "w"), indent=1)
            print(name, json.dumps(metas[name]["conditions"])[:300], metas[name]["het_male_variants"])
        assert metas["i_qt_het_male"]["het_male_variants"] == ["s%d" % j for j in xc.HET_MALE]
        assert all(not metas[n]["het_male_variants"] for n in xc.CASES if n != "i_qt_het_male")


if __name__ == "__main__":
    main()
