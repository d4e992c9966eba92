"""A multi-output second-order scalar cost (TOA_JIT_COST_GGN_MULTI) through the header-only C++ adaptor: compiles with plain g++ against the C-ABI
(CPU check), runs a dyadic quadratic through tinyopt_amd::Optimize under GaussNewton on the GPU — the minimiser in one Newton step, with and without with_prior; GradientDescent,
L-BFGS, bounds and a ragged batch on it throw."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_header_ggn_multi.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_test_header_ggn_multi")


def _compile():
    libdir = os.path.join(ROOT, "tinyopt_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE,
                    "-L", libdir, "-ltinyopt_amd", "-pthread", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_header_ggn_multi_compiles_with_plain_gxx(built):
    _compile()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_header_ggn_multi_runs(built):
    _compile()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
