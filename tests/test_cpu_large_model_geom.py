"""csrc/large_model_geom.hpp — the LDS geometry that large_model_rows_kernel and its host launcher share — swept by a stand-alone
program (plain g++, no HIP): element sizes 4 and 8, n = 1 .. 1024 (fp64: 512), kR = 1 .. 8, kD in {0, 1, n + 1, 2048}, with and
without the J image."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_large_model_geom.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_test_large_model_geom")


def test_large_model_geometry_fits_is_aligned_and_keeps_the_image_off_the_items():
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", SRC, "-o", EXE], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    lines = r.stdout.splitlines()
    for line in lines[:40]:
        print(line)
    assert r.returncode == 0 and lines[-1].endswith(" violations 0"), "\n".join(lines[:60])
    assert int(lines[-1].split()[1]) == (1024 + 512) * 8 * 4 * 2
