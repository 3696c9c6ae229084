"""The pure pieces of the LD driver (regenie_amd/host/driver_ld.h, driver_step2.h), compiled with g++ into a small harness
(tests/ld_plan_harness.cpp; no GPU involved):
  plan_ld_columns      which variant takes which column of the LD matrix, in file order or in the order of --extract --forcein-vars;
  SampleMap            the analysed samples among the kept ones and their place in the genotype file;
  bgen_dosage_255      8-bit .bgen probabilities -> the integer dosage in units of 1/255 (Geno.cpp:2286-2290), both allele orders;
  pgen_dosage_16384    a .pgen dosage -> the integer in units of 1/16384.
Every expected value is worked out here in Python."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("ldplan") / "libldplan.so"
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "regenie_amd", "host"),
                        os.path.join(ROOT, "tests", "ld_plan_harness.cpp"), "-o", str(so), "-lz", "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lb = C.CDLL(str(so))
    lb.sample_map.restype = C.c_int64
    lb.pgen_rule.restype = C.c_uint32
    lb.pgen_rule.argtypes = [C.c_double]
    lb.not_integral.restype = C.c_uint32
    return lb


def _plan(lib, ids, forced=None):
    blob = lambda v: "".join(s + "\n" for s in v).encode()      # noqa: E731
    nv = len(ids)
    cov = np.full(nv, -7, np.int32); absent = np.full(nv + len(forced or []), 9, np.uint8); present = np.full(nv, -7, np.int64)
    npres = C.c_int32(-1)
    out = C.create_string_buffer(4096)
    M = lib.ld_plan(blob(ids), nv, blob(forced) if forced is not None else None, len(forced) if forced is not None else -1, P(cov), P(absent), P(present),
                    C.byref(npres), out, 4096)
    assert M >= 0
    col_ids = out.raw.decode().split("\n")[:M]
    return col_ids, list(cov), list(absent[:M]), list(present[:npres.value])


def _want_default(ids):
    col_ids, cov = [], []
    for v in ids:
        if v in col_ids:
            cov.append(-1)
        else:
            cov.append(len(col_ids))
            col_ids.append(v)
    return col_ids, cov, [0] * len(col_ids), [j for j, c in enumerate(cov) if c >= 0]


def _want_forced(ids, lines):
    col_ids = []
    for ln in lines:
        ln = ln[:-1] if ln.endswith("\r") else ln
        if ln not in col_ids:
            col_ids.append(ln)
    absent, cov = [1] * len(col_ids), []
    for v in ids:
        c = col_ids.index(v) if v in col_ids else -1
        if c >= 0 and not absent[c]:
            c = -1                                   # a second variant with a placed ID
        if c >= 0:
            absent[c] = 0
        cov.append(c)
    return col_ids, cov, absent, [j for j, c in enumerate(cov) if c >= 0]


@pytest.mark.parametrize("ids", [["rs5", "rs1", "rs9", "rs1", "rs2", "rs5", "rs7"], ["a"], ["x", "x", "x"]], ids=["repeats", "one", "all_same"])
def test_plan_default_mode(lib, ids):
    """File order; a repeated variant ID takes one column and its later occurrences none."""
    got = _plan(lib, ids)
    assert got == _want_default(ids)
    if ids[0] == "rs5":
        assert got[0] == ["rs5", "rs1", "rs9", "rs2", "rs7"] and got[1] == [0, 1, 2, -1, 3, -1, 4] and got[3] == [0, 1, 2, 4, 6]


def test_plan_forced_in_mode(lib):
    """The order of the extract file; duplicate lines ignored (one of them only after its trailing '\\r' is dropped); IDs the genotype file
    does not have become absent columns; the second variant with an already-placed ID takes no column."""
    ids = ["rs5", "rs1", "rs9", "rs1", "rs2", "rs7"]
    lines = ["rs2\r", "gone1", "rs1", "rs2", "rs5\r", "gone2\r", "rs1", "gone1"]
    got = _plan(lib, ids, lines)
    assert got == _want_forced(ids, lines)
    col_ids, cov, absent, present = got
    assert col_ids == ["rs2", "gone1", "rs1", "rs5", "gone2"]
    assert cov == [3, 2, -1, -1, 0, -1] and absent == [0, 1, 0, 0, 1] and present == [0, 1, 4]
    # nothing of the file in the list: every column is absent, no variant is read
    got = _plan(lib, ["a", "b"], ["c", "d\r"])
    assert got == (["c", "d"], [-1, -1], [1, 1], [])


@pytest.mark.parametrize("case", ["identity", "ignored", "dropped", "both", "reordered_none"])
def test_sample_map(lib, case):
    """ind_ignore marks samples of the file that are not kept; ain marks the kept samples that are analysed.  file_idx[k] is the place in the
    file of analysed sample k; identity only when every sample of the file is analysed."""
    rng = np.random.default_rng(7)
    n_file = 41
    ign = np.zeros(n_file, np.uint8)
    if case in ("ignored", "both"):
        ign[rng.choice(n_file, 6, replace=False)] = 1
        ign[0] = 1
    N = int(n_file - ign.sum())
    ain = np.ones(N, np.uint8)
    if case in ("dropped", "both"):
        ain[rng.choice(N, 5, replace=False)] = 0
        ain[N - 1] = 0
    if case == "reordered_none":
        ain[:] = 0
        ain[3] = 1
    kept = [i for i in range(n_file) if not ign[i]]
    want_an = [k for k in range(N) if ain[k]]
    want_idx = [kept[k] for k in want_an]
    an = np.full(N, -1, np.int64); fidx = np.full(N, -1, np.int64)
    ident = C.c_int32(-1)
    n = lib.sample_map(P(ign), C.c_int64(n_file), P(ain), C.c_int64(N), P(an), P(fidx), C.byref(ident))
    assert n == len(want_an)
    assert list(an[:n]) == want_an and list(fidx[:n]) == want_idx
    assert ident.value == int(n == n_file and want_idx == list(range(n_file)))
    assert ident.value == int(case == "identity")


@pytest.mark.parametrize("ref_first", [0, 1])
def test_bgen_dosage_rule(lib, ref_first):
    """All 256 x 256 byte pairs: G * 255 = b1 + 2 b0, or with --ref-first b1 + 2 max(255 - b0 - b1, 0); above 510 it is not integral."""
    q = np.zeros((256, 256), np.uint32); ok = np.zeros((256, 256), np.uint8)
    lib.bgen_rule(ref_first, P(q), P(ok))
    b0, b1 = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    want = b1 + 2 * np.maximum(255 - b0 - b1, 0) if ref_first else b1 + 2 * b0
    assert np.array_equal(q, want)
    assert np.array_equal(ok != 0, want <= 510)
    if ref_first:
        assert ok.all()                                  # max(., 0) keeps it at b1 <= 255 when the probabilities add up to more than 1
    else:
        assert not ok[255, 1] and not ok[200, 200] and ok[255, 0] and ok[0, 255] and (~(ok != 0)).sum() == (want > 510).sum() > 0


def test_pgen_dosage_rule(lib):
    bad = lib.not_integral()
    assert bad > 0xFFFF
    assert lib.pgen_rule(-3.0) == 0xFFFF                                  # missing
    for k in (0, 1, 2, 8191, 16384, 16385, 32767, 32768):
        assert lib.pgen_rule(k / 16384.0) == k                            # exact multiples of 1/16384 (exact in binary)
    assert lib.pgen_rule(1.25 + 1e-12) == int(1.25 * 16384)               # inside the 1e-6 rule (in units of 1/16384)
    for g in (0.5 + 1e-5, 1.0 - 1e-5, -1.0 / 16384.0, -0.5, 2.0 + 1.0 / 16384.0, 2.5):
        assert lib.pgen_rule(g) == bad, g
