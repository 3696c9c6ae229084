#!/usr/bin/env python
"""TEST INFRASTRUCTURE.  Generates tests/golden/ref_outputs/rerint/: the output FILES of regenie v4.1.2 itself (oracle/_ref/regenie, built by
oracle/Makefile) for the `--apply-rerint` / `--apply-rerint-cov` cases of tests/rerint_cases.py, gzipped, with the command line and the exit status
in meta.json.  It asserts that regenie's files of `--bt --apply-rerint` are those of the run without the option, and -- with the NumPy restatement
(tests/rerint_restate.py) -- that every restated case prints the same six digits as regenie in every row (the cap of the GPU CLI test is zero
differing rows, so the cases must meet it on the CPU first), and records the number of tied values of case (h) in its meta.json.

  python tests/golden/make_rerint_ref_outputs.py      # needs oracle/_ref/regenie (make -C oracle)
"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import rerint_cases as rc      # noqa: E402

REGENIE = os.path.join(ROOT, "oracle", "_ref", "regenie")


def store(dst, name, data):
    with open(os.path.join(dst, name + ".gz"), "wb") as f:
        f.write(gzip.compress(data, 9, mtime=0))


def main():
    with tempfile.TemporaryDirectory() as tmp:
        rc.write_inputs(tmp)
        for name in rc.CASES:
            dst = os.path.join(rc.REF, name)
            os.makedirs(dst, exist_ok=True)
            args = rc.args_of(name, tmp) + ["--threads", "2", "--out", os.path.join(tmp, name)]
            r = subprocess.run([REGENIE] + args, capture_output=True, text=True)
            text = (r.stdout + r.stderr).replace(tmp, "{D}")
            assert r.returncode == 0, text[-3000:]
            meta = {"cmd": [a.replace(rc.EX, "{E}").replace(tmp, "{D}") for a in args], "returncode": r.returncode}      # (regenie logs no line for the options)
            if name == "h_bed_ties":
                ids, Y = rc.tied_phenotypes()
                meta["ties"] = ("the Step-2 residuals tie exactly: no covariate but the intercept, LOCO predictions of zero, phenotypes on grids of %d and %d "
                                "values over %d and %d observed samples" % (rc.TIE_LEVELS + tuple(int((~np.isnan(Y[:, k])).sum()) for k in range(2))))
            for k in (1, 2):
                store(dst, "out_Y%d.regenie" % k, open(os.path.join(tmp, "%s_Y%d.regenie" % (name, k)), "rb").read())
            json.dump(meta, open(os.path.join(dst, "meta.json"), "w"), indent=1)
            print(name, r.returncode)
    for k in (1, 2):
        a, b = (gzip.open(os.path.join(rc.REF, n, "out_Y%d.regenie.gz" % k), "rb").read() for n in ("g_bt_ignored", "g0_bt_plain"))
        assert a == b and a.count(b"\n") == 401
    from tests import rerint_restate as rr
    for name in rc.RESTATED:
        d = rr.differing_rows(name)
        print(name, "rows whose printed digits differ between the restatement and regenie:", d)
        assert d == 0, name


if __name__ == "__main__":
    main()
