#!/usr/bin/env python
"""TEST INFRASTRUCTURE.  Generates tests/golden/ref_outputs/af_cc/: the output FILES of regenie v4.1.2 itself (oracle/_ref/regenie, built by
oracle/Makefile) for the `--af-cc` cases of tests/afcc_cases.py, gzipped, with the command line, the exit status and whether the log carries the
disabling warning in meta.json.  For the cases of afcc_cases.TWINS regenie is also run without the option (<name>_plain).  It checks what the
fixtures are for:
  - every active case's header has the four columns where print_header_output_single puts them, and every line has as many fields as the header;
  - no line of an active case prints `nan` (the generator keeps observed cases and controls in every kept test);
  - the disabled cases log the warning and equal their twin without the option byte for byte.

  python tests/golden/make_afcc_ref_outputs.py      # needs oracle/_ref/regenie (make -C oracle)
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
from tests import afcc_cases as ac      # noqa: E402

REGENIE = os.path.join(ROOT, "oracle", "_ref", "regenie")


def store(dst, name, data):
    with open(os.path.join(dst, name + ".gz"), "wb") as f:
        f.write(gzip.compress(data, 9, mtime=0))


def run(name, tmp, af_cc):
    tag = name if af_cc else name + "_plain"
    dst = os.path.join(ac.REF, tag)
    os.makedirs(dst, exist_ok=True)
    args = ac.args_of(name, tmp, af_cc) + ["--threads", "2", "--out", os.path.join(tmp, tag)]
    r = subprocess.run([REGENIE] + args, capture_output=True, text=True)
    assert r.returncode == 0, (tag, r.stdout[-2000:], r.stderr[-2000:])
    for k in range(1, ac.P + 1):
        store(dst, "out_Y%d.regenie" % k, open(os.path.join(tmp, "%s_Y%d.regenie" % (tag, k)), "rb").read())
    m = {"cmd": [a.replace(tmp, "{D}") for a in args], "returncode": r.returncode, "warning": ac.WARNING in r.stdout,
         "lines": [len(ac.golden(tag, k)) - 1 for k in range(1, ac.P + 1)]}
    json.dump(m, open(os.path.join(dst, "meta.json"), "w"), indent=1)
    print(tag, m["warning"], m["lines"])
    return m


def main():
    with tempfile.TemporaryDirectory() as tmp:
        ac.write_inputs(tmp)
        for name in ac.CASES:
            m = run(name, tmp, True)
            assert m["warning"] == (name in ac.DISABLED), name
            if name in ac.TWINS:
                assert not run(name, tmp, False)["warning"]
        for name in ac.ACTIVE:
            for k in range(1, ac.P + 1):
                lines = ac.golden(name, k)
                h = lines[0].split(" ")
                assert h[h.index("A1FREQ") + 1:h.index("A1FREQ") + 3] == list(ac.AFCC_COLS[:2]) and h[h.index("N") + 1:h.index("N") + 3] == list(ac.AFCC_COLS[2:]), h
                assert len(lines) > 100 and all(len(ln.split(" ")) == len(h) for ln in lines) and not any("nan" in ln for ln in lines), (name, k)
        for name in ac.DISABLED:
            for k in range(1, ac.P + 1):
                assert ac.golden(name, k) == ac.golden(name + "_plain", k) and not set(ac.AFCC_COLS) & set(ac.golden(name, k)[0].split(" ")), name
        for name in ("a_bed", "f_bgen"):
            for k in range(1, ac.P + 1):
                assert ac.strip_afcc(ac.golden(name, k)) == ac.golden(name + "_plain", k), name


if __name__ == "__main__":
    main()
