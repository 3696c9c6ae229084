#!/usr/bin/env python
"""TEST INFRASTRUCTURE.  Generates tests/golden/ref_outputs/condtl/: the output FILES of regenie v4.1.2 itself (oracle/_ref/regenie, built by
oracle/Makefile) for the conditional-analysis cases of tests/condtl_cases.py, gzipped, with the command line, the exit status, the
`+conditioning on variants` lines of the log and (failed runs) the ERROR lines in meta.json.

  python tests/golden/make_condtl_ref_outputs.py      # needs oracle/_ref/regenie (make -C oracle)
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
from tests import condtl_cases as cc      # noqa: E402

REGENIE = os.path.join(ROOT, "oracle", "_ref", "regenie")


def store(dst, name, data):
    with open(os.path.join(dst, name + ".gz"), "wb") as f:
        f.write(gzip.compress(data, 9, mtime=0))


def main():
    with tempfile.TemporaryDirectory() as tmp:
        cc.write_inputs(tmp)
        for name in cc.CASES:
            dst = os.path.join(cc.REF, name)
            os.makedirs(dst, exist_ok=True)
            args = cc.args_of(name, tmp) + ["--threads", "2", "--out", os.path.join(tmp, name)]
            r = subprocess.run([REGENIE] + args, capture_output=True, text=True)
            text = (r.stdout + r.stderr).replace(tmp, "{D}")
            meta = {"cmd": [a.replace(cc.EX, "{E}").replace(tmp, "{D}") for a in args], "returncode": r.returncode,
                    "log": [ln for ln in text.splitlines() if "conditioning on variants" in ln or "-n_used" in ln or "-extracting variants" in ln
                            or "specified by --exclude" in ln or "variants remaining" in ln]}
            if r.returncode != 0:
                meta["error"] = [ln for ln in text.splitlines() if ln.startswith("ERROR")]
            for k in range(1, cc.traits_of(name) + 1):
                fn = os.path.join(tmp, "%s_Y%d.regenie" % (name, k))
                if os.path.exists(fn) and r.returncode == 0:
                    store(dst, "out_Y%d.regenie" % k, open(fn, "rb").read())
            fn = os.path.join(tmp, name + ".corr.snplist")
            if os.path.exists(fn) and r.returncode == 0:
                store(dst, "out.corr.snplist", open(fn, "rb").read())
            json.dump(meta, open(os.path.join(dst, "meta.json"), "w"), indent=1)
            print(name, r.returncode, meta.get("error", ""), meta["log"])


if __name__ == "__main__":
    main()
