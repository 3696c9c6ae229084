#!/usr/bin/env python
"""TEST INFRASTRUCTURE.  Generates tests/golden/ref_outputs/ld_gtg/: the output FILES of regenie v4.1.2 itself (oracle/_ref/regenie, built by
oracle/Makefile) for `--step 2 --output-corr-text --skip-scaleG [--sparse-thr t]`, for the cases of tests/ld_gtg_cases.py, gzipped, with the
command line in meta.json.

  python tests/golden/make_ld_gtg_ref_outputs.py      # needs oracle/_ref/regenie (make -C oracle)
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
from tests import ld_cases as lc           # noqa: E402
from tests import ld_gtg_cases as gc       # noqa: E402

REGENIE = os.path.join(ROOT, "oracle", "_ref", "regenie")


def store(dst, name, data):
    with open(os.path.join(dst, name + ".gz"), "wb") as f:
        f.write(gzip.compress(data, 9, mtime=0))


def main():
    with tempfile.TemporaryDirectory() as tmp:
        S = os.path.join(tmp, "synth")
        lc.write_synth(S)
        lc.write_lists(tmp)
        for name in gc.CASES:
            dst = os.path.join(gc.REF, name)
            os.makedirs(dst, exist_ok=True)
            args = gc.args_of(name, S, tmp) + ["--threads", "2", "--out", os.path.join(tmp, name)]
            r = subprocess.run([REGENIE] + args, capture_output=True, text=True)
            assert r.returncode == 0, r.stdout + r.stderr
            assert "(=GtG)" in r.stdout
            meta = {"cmd": [a.replace(lc.EX, "{E}").replace(tmp, "{T}") for a in args], "returncode": r.returncode}
            for ext in (".corr", ".corr.snplist", ".corr.forcedIn.snplist"):
                fn = os.path.join(tmp, name + ext)
                if os.path.exists(fn):
                    store(dst, "out" + ext, open(fn, "rb").read())
            json.dump(meta, open(os.path.join(dst, "meta.json"), "w"), indent=1)
            print(name, r.returncode, os.path.getsize(os.path.join(dst, "out.corr.gz")), "bytes")


if __name__ == "__main__":
    main()
