"""csrc/symeig.h (the projected symmetric eigenproblem of dcfm_sigma_eigs: Householder
tridiagonalisation + implicit QL, plain C++) checked by the stand-alone program tests/symeig_main.cpp:
a diagonal matrix, a 2 x 2 with a closed form, a 64 x 64 Q D Q' with a repeated eigenvalue and a
1 x 1, each to ||A V - V D||_max <= 64 n eps ||A|| and V orthonormal to the same order.  The program is
built with the host compiler and -fsanitize=address,undefined and run as a child process."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "a-divide-and-conquer-strategy-for-high-dimensional-bayesian-factor-models_amd" / "csrc"


def test_symeig_under_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = tmp_path / "symeig_main"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", f"-I{CSRC}", str(ROOT / "tests" / "symeig_main.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 4 and all(ln.rstrip().endswith("ok") for ln in lines), r.stdout
    assert [ln.split()[0] for ln in lines] == ["diagonal", "2x2", "1x1", "householder"]
