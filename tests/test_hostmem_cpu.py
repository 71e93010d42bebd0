"""csrc/hostmem.h on the host: the owners, the replace helpers and the guard, run over a
counting heap by tests/cpp/hostmem_test.cpp under AddressSanitizer and UBSan.  The program is a
stand-alone child process; its exit status is its failed checks plus its live allocations."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "hostmem_test.cpp")


def test_hostmem_owners_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no system C++ compiler (c++, g++ or clang++) on PATH")
    exe = str(tmp_path / "hostmem_test")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "0 failed checks, 0 live allocations" in run.stdout, run.stdout
