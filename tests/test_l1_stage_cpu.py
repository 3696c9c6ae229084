"""regenie_amd/csrc/l1_stage.h -- the host code that owns the K-fold level 1's page-locked staging area (work-item table of the fold Gram,
chromosome column table, LOCO chromosome ids, ridge values, results) -- as a stand-alone program (tests/hipcpu/l1_stage_host.cpp, its own main,
malloc / free as the allocators) under AddressSanitizer and UBSan: the tables are complete and lie inside their sections, the same shape is
not rebuilt, a changed shape is, the area grows and never leaks, an allocation failure leaves a released, reusable stage."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_l1_stage_under_sanitizers(tmp_path):
    exe = str(tmp_path / "l1_stage_host")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
                    os.path.join(HERE, "hipcpu", "l1_stage_host.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "l1_stage ok" in r.stdout
