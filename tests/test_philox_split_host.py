"""csrc/philox.h's split form on the host (CPU only): tests/philox_split_host.cpp is built from the header with the host
compiler into a program of its own — with AddressSanitizer and UBSan where the compiler links them — and must find
philox_prefix + philox_uniform + philox_tail equal to philox4x32_10 on the Random123 known-answer vectors and on 10^5
random (counter, key) pairs that include c1 = 0, c1 = 0x80000000, c0 >= 1024 and c2 = 0xFFFFFFFF."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "philox_split_host.cpp")
INC = os.path.join(ROOT, "fl_scaling_sc_ldpc_amd", "csrc")
PAIRS = 100000


def _cxx():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


@pytest.mark.skipif(_cxx() is None, reason="needs a host C++ compiler")
def test_split_equals_philox4x32_10(tmp_path):
    exe = str(tmp_path / "philox_split_host")
    base = [_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", INC, SRC, "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    built = subprocess.run(base + san, capture_output=True, text=True)
    if built.returncode != 0:                                           # a compiler without the sanitizers' runtimes
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe, str(PAIRS)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok %d" % PAIRS
