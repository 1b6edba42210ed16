"""Host-side C++ test of the lean-instantiation chooser of the GEMM launcher (csrc/gemm_lean.h: the
default step's launches get their lean kernel, everything else the general one), built with
AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_gemm_lean.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_gemm_lean_chooser_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "test_gemm_lean")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
