"""csrc/small_route.hpp — who runs a solve or a data pass of a compiled-in model family — against the two ladders it replaced: a
stand-alone program (plain g++, no HIP) restates the tail of lm_run_impl and the ladder of toa_accumulate literally from commit
b6c408d and sweeps both and the route functions over every compiled-in model tag, both dtypes, n = 1 .. 63, m in {1, 2, 255, 256,
511, 512, 513, 1000, 2000, 4096, 4097} and the two m either side of m (n + 1) = 20 000, num_cus in {64, 256}, eight batch sizes
around num_cus / 4, num_cus and 2 num_cus, a loss set or not, narrow_mfma_pass, wide_no_autosplit, wide_team_max_per_cu in
{0, 1, 3}, splits in {-1, 0, 1, 7} and mode in {0, 1, 2, 3}: family, splits and refusal (code and text)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_small_route.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_test_small_route")


def test_small_route_takes_the_routes_of_the_two_ladders_it_replaced():
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", SRC, "-o", EXE], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    lines = r.stdout.splitlines()
    for line in lines[:-1][:40]:
        print(line)
    print(lines[-1])
    assert r.returncode == 0 and lines[-1].endswith(" declared 0 unexpected 0"), "\n".join(lines[:40])
    # small_route.hpp declares no branch unreachable: no difference of either kind is printed, and the sweep did run
    assert lines[:-1] == []
    assert int(lines[-1].split()[1]) > 50_000_000
