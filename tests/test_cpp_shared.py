"""Shared item tables (JitResidual's shared_scalars) through the header-only C++ adaptor: compiles with plain g++
against the C-ABI (CPU check), solves a dyadic quadratic whose rows sit in ONE table for two problems in one Gauss-Newton step on the
GPU, keeps a residual model on the same table inside its box, and checks that the refusals throw."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_header_shared.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_test_header_shared")


def _compile():
    libdir = os.path.join(ROOT, "tinyopt_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE,
                    "-L", libdir, "-ltinyopt_amd", "-pthread", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_header_shared_compiles_with_plain_gxx(built):
    _compile()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_header_shared_runs(built):
    _compile()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
