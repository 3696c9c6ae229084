#!/usr/bin/env python
"""TEST INFRASTRUCTURE.  Generates tests/golden/ref_outputs/mcc/: the output FILES of regenie v4.1.2 itself (oracle/_ref/regenie, built by
oracle/Makefile) for the `--mcc` cases of tests/mcc_cases.py, gzipped, with the command line, the exit status, the skewness line of the log and
(failed runs) the ERROR lines in meta.json.  With the NumPy restatement (tests/mcc_restate.py) it asserts that no row of cases (a) and (d) has a
non-positive skewness of D or a p-value of exactly 0 or 1 (the driver reports such rows as NA / TEST_FAIL, which regenie's files do not have).

  python tests/golden/make_mcc_ref_outputs.py      # needs oracle/_ref/regenie (make -C oracle)
"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import mcc_cases as mc      # noqa: E402

REGENIE = os.path.join(ROOT, "oracle", "_ref", "regenie")


def store(dst, name, data):
    with open(os.path.join(dst, name + ".gz"), "wb") as f:
        f.write(gzip.compress(data, 9, mtime=0))


def main():
    with tempfile.TemporaryDirectory() as tmp:
        mc.write_inputs(tmp)
        for name in mc.CASES:
            dst = os.path.join(mc.REF, name)
            os.makedirs(dst, exist_ok=True)
            args = mc.args_of(name, tmp) + ["--threads", "2", "--out", os.path.join(tmp, name)]
            r = subprocess.run([REGENIE] + args, capture_output=True, text=True)
            text = (r.stdout + r.stderr).replace(tmp, "{D}")
            meta = {"cmd": [a.replace(mc.EX, "{E}").replace(tmp, "{D}") for a in args], "returncode": r.returncode,
                    "log": [ln for ln in text.splitlines() if "phenotypic skewness" in ln]}
            if r.returncode != 0:
                meta["error"] = [ln for ln in text.splitlines() if ln.startswith("ERROR")]
            for k in (1, 2):
                fn = os.path.join(tmp, "%s_Y%d.regenie" % (name, k))
                if os.path.exists(fn) and r.returncode == 0:
                    store(dst, "out_Y%d.regenie" % k, open(fn, "rb").read())
            json.dump(meta, open(os.path.join(dst, "meta.json"), "w"), indent=1)
            print(name, r.returncode, meta.get("error", ""), meta["log"])
    from tests import mcc_restate as mr
    for name in ("a_bed_all", "d_bgen_all"):
        for k, res in enumerate(mr.restate_case(name)):
            assert (res["skew"] > 0).all() and ((res["p"] > 0) & (res["p"] < 1)).all(), (name, k)


if __name__ == "__main__":
    main()
