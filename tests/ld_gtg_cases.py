"""The reference cases of `--compute-corr --output-corr-text --skip-scaleG [--sparse-thr t]` (the unscaled LD matrix and its sparse form):
the command lines -- one definition for tests/golden/make_ld_gtg_ref_outputs.py (which runs regenie itself on them), for
tests/test_ld_gtg_restate_cpu.py (the fp64 restatement against regenie's files) and for tests/test_ld_gtg_cli_gpu.py (the driver).
The inputs are those of tests/ld_cases.py (write_synth, write_lists), used by import.  The synthetic cases take the first 150 variants
of chromosome 2: its two degenerate columns come later (tests/ld_cases.py says why they cannot be pinned)."""
import os

from tests import ld_cases as lc
from tests import ld_dosage_cases as dc

ROOT = lc.ROOT
EX = lc.EX
REF = os.path.join(ROOT, "tests", "golden", "ref_outputs", "ld_gtg")

_SYNTH = ["--bed", "{S}", "--covarFile", "{S}.covar", "--remove", "{S}.remove", "--chr", "2", "--extract", "{S}.extract150", "--output-corr-text", "--skip-scaleG"]

# name -> arguments ({E} example dir, {S} synthetic prefix, {D} the directory of the lists); every case runs with --step 2 --bsize 100
CASES = {
    "a_example400_gtg": ["--bed", "{E}/example", "--covarFile", "{E}/covariates.txt", "--extract", "{D}/first400.txt", "--output-corr-text", "--skip-scaleG"],
    "b_forced153_thr20": ["--bed", "{E}/example", "--covarFile", "{E}/covariates.txt", "--extract", "{D}/forced153.txt", "--forcein-vars", "--output-corr-text",
                          "--skip-scaleG", "--sparse-thr", "0.2"],
    "c_synth_chr2_thr05": _SYNTH + ["--sparse-thr", "0.05"],
    "d_synth_chr2_thr90": _SYNTH + ["--sparse-thr", "0.9"],
    "e_bgen400_thr20": ["--bgen", "{E}/example.bgen", "--covarFile", "{E}/covariates.txt", "--extract", "{D}/first400.txt", "--output-corr-text", "--skip-scaleG",
                        "--sparse-thr", "0.2"],
}
SPARSE = {"b_forced153_thr20": 0.2, "c_synth_chr2_thr05": 0.05, "d_synth_chr2_thr90": 0.9, "e_bgen400_thr20": 0.2}
DRIVER_EXTRA = {"e_bgen400_thr20": ["--ld-dosages"]}      # the driver's own switch for dosage input in LD mode; regenie needs none


def args_of(name, S, D):
    return ["--step", "2", "--bsize", "100"] + [a.replace("{E}", EX).replace("{S}", S).replace("{D}", D) for a in CASES[name]]


def dense_case(name, S, D):
    """The dense inputs of print_ld for a case (tests/ld_cases.py / tests/ld_dosage_cases.py: dense_case): G [n][M] (nan = missing, a
    forced-in column zero), X [n][C], params.n_samples, the column ids."""
    src, saved = (dc, dc.CASES) if "--bgen" in CASES[name] else (lc, lc.CASES)
    try:      # the readers look the command line up by name in their own table
        src.CASES = dict(saved, **{name: CASES[name]})
        return src.dense_case(name, S, D)
    finally:
        src.CASES = saved
