"""The launch builders of the tile-product kernels (causalgpslc.jl_amd/csrc/tile_launch.h), compiled with g++ against the HIP stub
and exercised by tests/c/tile_launch_test.cpp: at every launch site of the host files, over tile counts 1..9, 17 and 34, panel widths
1, 4 and 8, up to two augmented tile rows, 0..128 live rows, with and without the skipped augmented diagonal tile, row counts
other than the tile count for the pair workspaces and one or two tile rows of MVN vectors, the builder's GemmArgs equals field by
field what api.hip assigned by hand before, ntiles is the number of tiles the kernel's decode visits and every one of them lies
in the launch's rectangle; the profiler's flop count equals the former arithmetic bit for bit and the counts worked out by hand."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_builders_equal_the_hand_written_launches_and_keep_their_invariants(tmp_path):
    exe = str(tmp_path / "tile_launch_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-attributes", "-I", os.path.join(ROOT, "tests", "c", "hip_stub"),
                           "-o", exe, os.path.join(ROOT, "tests", "c", "tile_launch_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    verdict, n = r.stdout.strip().splitlines()[-1].split()
    assert verdict == "OK" and int(n) > 10000, r.stdout[-2000:]
