"""The coded branch of regenie_amd/csrc/step2_bt.hip (`--test dominant | recessive`: rg_s2_bt_score_packed under rg_s2_set_coding) EXECUTED IN THIS
CONTAINER, as tests/test_step2_bt_emulated_cpu.py runs the additive one: the source compiled for the host against tests/hipcpu, with
tests/hipcpu/s2_contract_coded_host.cpp as the plain-loop stand-in of the hard-call contraction and of the relabelling of the staged rows.  What
runs is the library's own score_from_sums on the relabelled counts, the additive total_p / n_obs_p rewrite, and k_bt_prep / k_bt_firth1 / k_bt_spa
reading a relabelled staged row with no flip, in the full and the carriers-only form -- held to the oracle by the body of the GPU test
(tests/test_step2_coding_gpu.py), at its sizes and tolerances."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emulated(tmp_path_factory):
    d = tmp_path_factory.mktemp("s2emu_coded")
    so = str(d / "libs2emu_coded.so")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-w", "-shared", "-x", "c++", "-I" + os.path.join(ROOT, "tests", "hipcpu"),
                        os.path.join(ROOT, "regenie_amd", "csrc", "step2_bt.hip"), os.path.join(ROOT, "tests", "hipcpu", "s2_contract_coded_host.cpp"), "-o", so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(so)
    lib.rg_s2_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int64, C.c_int32, C.c_int32]
    lib.rg_s2_destroy.argtypes = [C.c_void_p]
    lib.rg_s2_destroy.restype = None
    lib.rg_s2_last_error.argtypes = [C.c_void_p]
    lib.rg_s2_last_error.restype = C.c_char_p
    lib.rg_s2_set_sparse_rule.argtypes = [C.c_void_p, C.c_int64, C.c_double, C.c_int32]
    lib.rg_s2_set_coding.argtypes = [C.c_void_p, C.c_int32]
    lib.rg_s2_bt_set_null.argtypes = [C.c_void_p, C.c_void_p]
    lib.rg_s2_bt_score_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p]
    lib.rg_s2_bt_correct.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.rg_s2_last_kernel_ms.argtypes = [C.c_void_p]
    lib.rg_s2_last_kernel_ms.restype = C.c_double
    return lib


@pytest.mark.parametrize("coding", [1, 2])
def test_coded_score_and_corrections_on_the_emulated_device(emulated, monkeypatch, coding):
    import regenie_amd.step2 as step2
    monkeypatch.setattr(step2, "load_library", lambda: emulated)
    from tests import test_step2_coding_gpu as t
    t.test_bt_score_and_corrections_under_a_coding(coding)
