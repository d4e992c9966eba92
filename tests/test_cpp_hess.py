"""A second-order scalar cost (TOA_JIT_COST_HESS) through the header-only C++ adaptor: compiles with plain g++ against the C-ABI (CPU check), runs
Rosenbrock as text (tests/optimize_easy.cpp:35-79) through tinyopt_amd::Optimize under LM on the GPU; GradientDescent on it throws."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_header_hess.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_test_header_hess")


def _compile():
    libdir = os.path.join(ROOT, "tinyopt_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE,
                    "-L", libdir, "-ltinyopt_amd", "-pthread", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_header_hess_compiles_with_plain_gxx(built):
    _compile()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_header_hess_runs(built):
    _compile()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
