#!/usr/bin/env python
"""TEST INFRASTRUCTURE.  Generates tests/golden/ref_outputs/ld/: the output FILES of regenie v4.1.2 itself (oracle/_ref/regenie, built by
oracle/Makefile) in LD mode, `--step 2 --compute-corr`, for the cases of tests/ld_cases.py, gzipped, with the command line in meta.json;
and the .regenie files of `--step 2 --qt --chr 2` (the --chr filter outside LD mode).

  python tests/golden/make_ld_ref_outputs.py      # needs oracle/_ref/regenie (make -C oracle)
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
from tests import ld_cases as lc      # noqa: E402

REGENIE = os.path.join(ROOT, "oracle", "_ref", "regenie")


def store(dst, name, data):
    with open(os.path.join(dst, name + ".gz"), "wb") as f:
        f.write(gzip.compress(data, 9, mtime=0))


def main():
    with tempfile.TemporaryDirectory() as tmp:
        S = os.path.join(tmp, "synth")
        lc.write_synth(S)
        lc.write_lists(tmp)
        for name in lc.CASES:
            dst = os.path.join(lc.REF, name)
            os.makedirs(dst, exist_ok=True)
            args = lc.args_of(name, S, tmp) + ["--threads", "2", "--out", os.path.join(tmp, name)]
            r = subprocess.run([REGENIE] + args, capture_output=True, text=True)
            meta = {"cmd": [a.replace(lc.EX, "{E}").replace(tmp, "{T}") for a in args], "returncode": r.returncode}
            if r.returncode != 0:
                meta["error"] = [ln for ln in (r.stdout + r.stderr).splitlines() if ln.startswith("ERROR")]
            for ext in (".corr", ".corr.snplist", ".corr.forcedIn.snplist"):
                fn = os.path.join(tmp, name + ext)
                if os.path.exists(fn) and r.returncode == 0 and not (name.startswith("c4") and ext == ".corr"):
                    store(dst, "out" + ext, open(fn, "rb").read())
            json.dump(meta, open(os.path.join(dst, "meta.json"), "w"), indent=1)
            print(name, r.returncode, meta.get("error", ""))
        # case 5: --step 2 --qt --chr 2 with the LOCO files of qt_kfold_3chr
        name, dst = "c5_qt_chr2", os.path.join(lc.REF, "c5_qt_chr2")
        os.makedirs(dst, exist_ok=True)
        R = os.path.join(HERE, "ref_outputs", "qt_kfold_3chr")
        with open(os.path.join(tmp, "pred.list"), "w") as pl:
            for k in (1, 2):
                fn = os.path.join(tmp, "ref_%d.loco" % k)
                open(fn, "wb").write(gzip.open(os.path.join(R, "out_%d.loco.gz" % k), "rb").read())
                pl.write("Y%d %s\n" % (k, fn))
        args = ["--step", "2", "--bed", lc.EX + "/example_3chr", "--phenoFile", lc.EX + "/phenotype.txt", "--covarFile", lc.EX + "/covariates.txt", "--qt",
                "--pred", os.path.join(tmp, "pred.list"), "--bsize", "200", "--chr", "2", "--threads", "2", "--out", os.path.join(tmp, name)]
        r = subprocess.run([REGENIE] + args, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        for k in (1, 2):
            store(dst, "out_Y%d.regenie" % k, open(os.path.join(tmp, "%s_Y%d.regenie" % (name, k)), "rb").read())
        json.dump({"cmd": [a.replace(lc.EX, "{E}").replace(tmp, "{T}") for a in args], "returncode": 0}, open(os.path.join(dst, "meta.json"), "w"), indent=1)
        print(name, r.returncode)


if __name__ == "__main__":
    main()
