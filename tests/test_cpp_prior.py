"""A Gaussian prior through the header-only C++ adaptor (JitResidual::bind(...).with_prior): compiles with plain g++ against the C-ABI
(CPU check); on the GPU a circle-fit batch with a diagonal prior — a huge W pins x to mu, as the Python path's does."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_header_prior.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_test_header_prior")


def _compile():
    libdir = os.path.join(ROOT, "tinyopt_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE,
                    "-L", libdir, "-ltinyopt_amd", "-pthread", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_header_prior_compiles_with_plain_gxx(built):
    _compile()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_header_prior_runs(built):
    _compile()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
