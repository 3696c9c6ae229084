#!/usr/bin/env python
"""TEST INFRASTRUCTURE.  Generates tests/golden/ref_outputs/ld_dosage/: the output FILES of regenie v4.1.2 itself (oracle/_ref/regenie,
built by oracle/Makefile) in LD mode on dosage input, `--step 2 --compute-corr --bgen`, for the cases of tests/ld_dosage_cases.py,
gzipped, with the command line in meta.json.

  python tests/golden/make_ld_dosage_ref_outputs.py      # needs oracle/_ref/regenie (make -C oracle)
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
from tests import ld_cases as lc              # noqa: E402
from tests import ld_dosage_cases as dc       # noqa: E402

REGENIE = os.path.join(ROOT, "oracle", "_ref", "regenie")


def store(dst, name, data):
    with open(os.path.join(dst, name + ".gz"), "wb") as f:
        f.write(gzip.compress(data, 9, mtime=0))


def main():
    with tempfile.TemporaryDirectory() as tmp:
        S = os.path.join(tmp, "synth")
        dc.write_synth(S)
        dc.write_synth_pgen(S + "_pgen")
        lc.write_lists(tmp)
        dc.write_cond(tmp)
        for name in dc.CASES:
            dst = os.path.join(dc.REF, name)
            os.makedirs(dst, exist_ok=True)
            args = dc.args_of(name, S, tmp) + ["--threads", "2", "--out", os.path.join(tmp, name)]
            r = subprocess.run([REGENIE] + args, capture_output=True, text=True)
            meta = {"cmd": [a.replace(dc.EX, "{E}").replace(tmp, "{T}") for a in args], "returncode": r.returncode,
                    "dosage_mode": "computing correlation matrix in dosage mode" in r.stdout}
            if r.returncode != 0:
                meta["error"] = [ln for ln in (r.stdout + r.stderr).splitlines() if ln.startswith("ERROR")]
            for ext in (".corr", ".corr.snplist", ".corr.forcedIn.snplist"):
                fn = os.path.join(tmp, name + ext)
                if os.path.exists(fn) and r.returncode == 0:
                    store(dst, "out" + ext, open(fn, "rb").read())
            json.dump(meta, open(os.path.join(dst, "meta.json"), "w"), indent=1)
            print(name, r.returncode, meta.get("error", ""))


if __name__ == "__main__":
    main()
