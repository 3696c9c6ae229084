"""Step1Ingest (regenie_amd/host/driver_step1_ingest.cpp) under AddressSanitizer and UBSan, host code only: tests/asan/step1_ingest_main.cpp is a
stand-alone program that drives the ingest over a small .bed with malloc-backed stand-ins for the device library, through the orders of start,
give-up, release and context teardown a run can take."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step1_ingest_teardown_orders_are_clean(tmp_path):
    host, csrc = os.path.join(ROOT, "regenie_amd", "host"), os.path.join(ROOT, "regenie_amd", "csrc")
    exe = str(tmp_path / "ingest_main")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I" + host,
                        os.path.join(ROOT, "tests", "asan", "step1_ingest_main.cpp"), os.path.join(host, "driver_step1_ingest.cpp"), os.path.join(host, "driver_common.cpp"),
                        os.path.join(csrc, "pgen_api.cpp"), os.path.join(csrc, "bgen_api.cpp"), "-o", exe, "-lz", "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("RG_")}      # (the sanitizer runtimes are linked statically: their place among the libraries does not matter)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "four sequences clean" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count("is not kept in device memory") == 1      # the stage that was given up; none where no stage was started
