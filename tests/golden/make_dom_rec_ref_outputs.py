#!/usr/bin/env python
"""TEST INFRASTRUCTURE.  Generates tests/golden/ref_outputs/dom_rec/: the output FILES of regenie v4.1.2 itself (oracle/_ref/regenie, built by
oracle/Makefile) for the `--test dominant|recessive` cases of tests/dom_rec_cases.py, gzipped, with the command line, the exit status, the log
lines about the coding and (failed runs) the ERROR lines in meta.json.  It also asserts what the cases are built to exercise: the five synthetic
variants with 0, 1, MIN_HOMS - 1, MIN_HOMS and MIN_HOMS + 1 homozygotes fall on the expected side of `--minHOMs`, and every TEST column carries
the coding's name.

  python tests/golden/make_dom_rec_ref_outputs.py      # needs oracle/_ref/regenie (make -C oracle)
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
from tests import dom_rec_cases as dc      # noqa: E402

REGENIE = os.path.join(ROOT, "oracle", "_ref", "regenie")


def store(dst, name, data):
    with open(os.path.join(dst, name + ".gz"), "wb") as f:
        f.write(gzip.compress(data, 9, mtime=0))


def main():
    with tempfile.TemporaryDirectory() as tmp:
        dc.write_inputs(tmp)
        for name in dc.CASES:
            dst = os.path.join(dc.REF, name)
            os.makedirs(dst, exist_ok=True)
            args = dc.args_of(name, tmp) + ["--threads", "2", "--out", os.path.join(tmp, name)]
            r = subprocess.run([REGENIE] + args, capture_output=True, text=True)
            text = (r.stdout + r.stderr).replace(tmp, "{D}")
            meta = {"cmd": [a.replace(dc.EX, "{E}").replace(tmp, "{D}") for a in args], "returncode": r.returncode,
                    "log": [ln for ln in text.splitlines() if any(m in ln for m in dc.LOG_MARKS)]}
            if r.returncode != 0:
                meta["error"] = [ln for ln in text.splitlines() if ln.startswith("ERROR")]
            for k in (1, 2):
                fn = os.path.join(tmp, "%s_Y%d.regenie" % (name, k))
                if os.path.exists(fn) and r.returncode == 0:
                    store(dst, "out_Y%d.regenie" % k, open(fn, "rb").read())
            json.dump(meta, open(os.path.join(dst, "meta.json"), "w"), indent=1)
            print(name, r.returncode, meta.get("error", ""), meta["log"])
    for name in dc.FILE_CASES:
        a = dc.CASES[name]
        want = {"additive": "ADD", "dominant": "DOM", "recessive": "REC"}[a[a.index("--test") + 1]]
        for k in (1, 2):
            rows = [ln.split(" ") for ln in dc.golden(name, k)]
            c = rows[0].index("TEST")
            assert len(rows) > 151 and all(r[c] == want for r in rows[1:]), (name, k, len(rows))
    for name, kept in (("b_qt_rec_minhoms", {0: False, 1: False, dc.MIN_HOMS - 1: False, dc.MIN_HOMS: True, dc.MIN_HOMS + 1: True}),
                       ("c_qt_dom_missing", {h: True for h in dc.HOM_ROWS.values()})):
        ids = {ln.split(" ")[2] for ln in dc.golden(name, 1)[1:]}
        for row, nhom in dc.HOM_ROWS.items():
            assert (("s%d" % row) in ids) == kept[nhom], (name, row, nhom)


if __name__ == "__main__":
    main()
