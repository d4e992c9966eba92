"""csrc/large_route.hpp — who factorises the n >= 64 systems — against the five hand-written predicates it replaced: a stand-alone
program (plain g++, no HIP) restates them literally from commit 68b07ee and sweeps n = 64 .. 1100, P in {1, 65535, 65536}, both
element sizes, force_library, use_ldlt and max_lds in {65536, 163840} through both."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_large_route.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_test_large_route")


def test_large_route_takes_the_routes_of_the_five_predicates_it_replaced():
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", SRC, "-o", EXE], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    lines = r.stdout.splitlines()
    for line in lines[:-1][:40]:
        print(line)
    print(lines[-1])
    assert r.returncode == 0 and " unexpected 0" in lines[-1], "\n".join(l for l in lines if l.startswith("UNEXPECTED"))[:4000]
    # what large_route.hpp declares unreachable, and nothing else: the LM loop beyond grid.y = 65 535 problems (it is entered
    # slice by slice), and n <= 128 on a device whose LDS does not hold the image (none this library is built for)
    for line in lines[:-1]:
        assert line.startswith("declared large_lm_run_t") and " P=65536 " in line and line.endswith("chol -> library") or \
            line.startswith(("declared toa_large_solve_each", "declared toa_ba_lists_run")) and "max_lds=65536 " in line and line.endswith("ours -> library"), line
