"""csrc/popmem.h on the host: what the population handle's setters replace (dataset, env model,
ensemble, synthetic-transition rings, collect workspace, start-row stage) and the step's
streams, run over a counting heap by tests/cpp/popmem_test.cpp under AddressSanitizer and
UBSan, with every allocation of every builder failing in turn.  The program is a stand-alone
child process; its exit status is its failed checks plus its live allocations plus its double
frees."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "popmem_test.cpp")


def test_popmem_setters_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no system C++ compiler (c++, g++ or clang++) on PATH")
    exe = str(tmp_path / "popmem_test")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "0 failed checks, 0 live allocations" in run.stdout, run.stdout
    assert "0 double frees" in run.stdout, run.stdout
