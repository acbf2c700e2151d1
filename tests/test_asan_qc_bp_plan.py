"""The quasi-cyclic sum-product plan builder under AddressSanitizer + UBSan on the
CPU: tests/asan/qc_bp_plan_check.cpp is compiled together with csrc/ldpc_plan.cpp
alone (no HIP, no library) into a stand-alone program and run directly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "asan")
CLANGXX = os.environ.get("CLANGXX", "/opt/rocm/lib/llvm/bin/clang++")


@pytest.mark.skipif(not os.path.exists(CLANGXX) and shutil.which("clang++") is None, reason="needs clang++")
def test_qc_bp_planner_under_asan():
    cxx = CLANGXX if os.path.exists(CLANGXX) else shutil.which("clang++")
    build = os.path.join(HERE, "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "qc_bp_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "qc_bp_plan_check.cpp"),
                    os.path.join(ROOT, "polarcode_and_ldpc_amd", "csrc", "ldpc_plan.cpp"), "-o", exe],
                   check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "all checks passed" in p.stdout
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr
